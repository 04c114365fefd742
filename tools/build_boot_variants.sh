#!/bin/bash
# A/B variants that differ only in macros of some HIP files: each file of SRC recompiled with the flags, linked with
# the other objects of the current build (fhe_amd/_build, make first) into abv/<name>.so.  The variants build in
# parallel; the script fails if any of them does.
# SRC is a list.  Its default is bootstrap and every boot_*.hip, since a -D may reach several units (FHE_FWD_TIGHT
# reaches K1, K1m and K1w), so by default every unit is recompiled for every variant even where one unit reads the
# knob: name that unit in SRC to save the time.
# The wrong-result ablations (FHE_X_ABL, FHE_LMK_ABL) need -DFHE_ALLOW_WRONG_RESULTS as well.
#   [SRC="bootstrap"] tools/build_boot_variants.sh name1 "-DFOO=1" name2 "-DBAR=2" ...
set -e
cd "$(dirname "$0")/.."
srcs=${SRC:-$(cd fhe_amd/csrc && ls bootstrap.hip boot_*.hip | sed 's/\.hip$//')}
mkdir -p abv
pids=()
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  mkdir -p abv/obj_$name
  rm -f abv/obj_$name/*.o abv/$name.so  # a unit that fails to compile must not link as a stale object
  (others=$(ls fhe_amd/_build/*.o)
   for src in $srcs; do
     /opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics $flags \
       -c fhe_amd/csrc/$src.hip -o abv/obj_$name/$src.o &
     others=$(echo "$others" | grep -v "/$src.o\$")
   done
   wait
   for src in $srcs; do [ -f abv/obj_$name/$src.o ] || { echo "FAILED abv/$name.so: $src.hip ($flags)"; exit 1; }; done
   /opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o abv/$name.so $(for src in $srcs; do echo abv/obj_$name/$src.o; done) \
     $others -lgomp && echo "built abv/$name.so ($flags)") &
  pids+=($!)
done
rc=0
for p in "${pids[@]}"; do wait $p || rc=1; done
exit $rc
