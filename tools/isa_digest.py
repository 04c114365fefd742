"""Per-kernel comparison of gfx950 assembly listings (hipcc --cuda-device-only -S): does moving kernels between
translation units change their code?
    python tools/isa_digest.py --base old.s [..] --new unit1.s unit2.s [..] [--must-match REGEX]
For every kernel of the base listings: a digest of its instruction text (comments and assembler directives
dropped, the function index in local labels removed) and its register / LDS / scratch directives, in the base and
in the new listing that holds it.  Exit status 1 if a base kernel is missing from the new listings or appears in
more than one, or if a kernel whose name matches --must-match differs."""
import argparse
import hashlib
import os
import re
import sys

DIRECTIVES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size",
              "accum_offset")


def kernels(path):
    """{symbol: (digest, instruction count, {directive: value})} of the listing's kernels"""
    out = {}
    for f in re.split(r'\n(?=_Z\S+:)', open(path).read()):
        m = re.match(r'(_Z\S+):', f)
        if not m or '.amdhsa_kernel ' + m.group(1) not in f:
            continue
        text = []
        for ln in f.split('\n')[1:]:
            ln = ln.split(';')[0].rstrip()
            s = ln.strip()
            if not s or (s.startswith('.') and not s.endswith(':')):
                continue  # comment or directive (labels kept)
            if s.startswith('.Lfunc_end'):
                break
            text.append(re.sub(r'\.L([A-Za-z]+)\d+_', r'.L\1_', s))
        d = {k: re.search(r'\.amdhsa_' + k + r'\s+(\S+)', f).group(1) for k in DIRECTIVES}
        n = sum(1 for t in text if not t.endswith(':'))
        out[m.group(1)] = (hashlib.sha256('\n'.join(text).encode()).hexdigest()[:16], n, d)
    return out


def res(k):
    return "insn {:6d} vgpr {:>3s} sgpr {:>3s} lds {:>6s} scratch {:>4s} accum {:>3s}".format(
        k[1], *(k[2][d] for d in DIRECTIVES))


ap = argparse.ArgumentParser()
ap.add_argument("--base", nargs="+", required=True)
ap.add_argument("--new", nargs="+", required=True)
ap.add_argument("--must-match", default=r"k_blind_rotate_|k_prep_")
a = ap.parse_args()

base = {}
for p in a.base:
    base.update(kernels(p))
new = {}
for p in a.new:
    for sym, k in kernels(p).items():
        new.setdefault(sym, []).append((os.path.basename(p), k))

same = diff = bad = 0
for sym in sorted(base):
    b, hits = base[sym], new.get(sym, [])
    if len(hits) != 1:
        print(f"{'MISSING' if not hits else 'DUPLICATE':9s} {sym}  {' '.join(h[0] for h in hits)}")
        bad += 1
        continue
    unit, k = hits[0]
    if k[0] == b[0] and k[2] == b[2]:
        print(f"same      {k[0]} {res(k)}  {unit:24s} {sym}")
        same += 1
        continue
    diff += 1
    must = re.search(a.must_match, sym) is not None
    bad += must
    print(f"{'DIFFERS!' if must else 'differs':9s} {sym}  ({unit})")
    print(f"    base  {b[0]} {res(b)}")
    print(f"    new   {k[0]} {res(k)}")
extra = sorted(set(new) - set(base))
print(f"# {len(base)} base kernels: {same} identical, {diff} differ, {len(base) - same - diff} missing or duplicated; "
      f"{len(extra)} kernels only in the new listings")
sys.exit(1 if bad else 0)
