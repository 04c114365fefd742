"""Device BTKeyGen timing: GateEngine.keygen_device (no export) against the path it replaces, the host generator
and the upload (binfhe.keygen() then load_keys()), for one parameter set per resident-layout class and the
large-precision STD128 set (logQ = 29, n = 1305: a 4.8 GB key-switching key).  A host clock around each call;
keygen_device and load_keys end in a stream synchronise.  The two paths alternate in one process.
    python tools/keygen_time.py [--out profiles/keygen_dev_time.txt] [--reps 3] [--sets std128q ...]
Writes median [min .. max] of the repetitions after one warm-up of each path.  On the large-precision set the
AND / XOR outputs on the device keys are also checked against tests/golden/large_std29.npz where it exists."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from fhe_amd import binfhe as bf  # noqa: E402
from make_golden import LARGE_SETS, WIDER_SETS  # noqa: E402

CLASSES = {"std128q": "g3 GINX", "lpf_std128q_lmkcdey": "g3 LMKCDEY", "std256q": "n2k GINX",
           "std256q_3_lmkcdey": "n2k LMKCDEY", "std256_lmkcdey": "A32, no second layout", "std192q": "A64",
           "signed_mod_test": "prime qKS", "std29": "large-precision STD128, logQ = 29"}
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/keygen_dev_time.txt")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sets", nargs="+", default=list(CLASSES))
args = ap.parse_args()
SEED = 1234
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def stat(ts):
    return f"{np.median(ts) * 1e3:10.1f} [{min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}]"


def check_std29(e, ps, sk, seed):
    """the gates of tests/golden/large_std29.npz on the resident device keys (make_golden.large_inputs' inputs)"""
    path = os.path.join(ROOT, "tests", "golden", "large_std29.npz")
    if not os.path.exists(path):
        return "fixture absent"
    g = np.load(path)
    rng = np.random.default_rng(seed)
    bits1, bits2 = rng.integers(0, 2, 2), rng.integers(0, 2, 2)
    a1, b1 = bf.encrypt(ps, bf.GINX, sk, bits1, seed + 1)
    a2, b2 = bf.encrypt(ps, bf.GINX, sk, bits2, seed + 2)
    ok = True
    for gname, gate in (("AND", 1), ("XOR", 4)):
        ao, bo = e.eval_gate(gate, a1, b1, a2, b2)
        ok = ok and np.array_equal(ao, g[f"{gname}_a"]) and np.array_equal(bo, g[f"{gname}_b"])
    return f"AND / XOR == large_std29.npz: {ok}"


slower = []
for name in args.sets:
    if name == "std29":
        st, arb, logQ = LARGE_SETS[name][:3]
        ps, m = bf.large_paramset(st, arb, logQ), bf.GINX
        seed = 0xB1600000 + logQ + (st << 8) + (int(arb) << 7)   # the fixture's key seed (make_golden.large_inputs)
    else:
        (ps, m), seed = WIDER_SETS[name], SEED
    P, plan = bf.params(ps, m), bf.keygen_plan(ps, m)
    sk = bf.keygen_secret(ps, m, seed)
    dev, host, note = [], [], ""
    for r in range(args.reps + 1):   # r = 0: the warm-up of each path
        e = bf.GateEngine(ps, m)
        t = time.perf_counter()
        e.keygen_device(sk, seed)
        dev.append(time.perf_counter() - t)
        if r == 0 and name == "std29":
            note = "  " + check_std29(e, ps, sk, seed)
        e.close()
        e = bf.GateEngine(ps, m)
        t = time.perf_counter()
        keys = bf.keygen(ps, m, seed)
        e.load_keys(keys.bsk, keys.kskA, keys.kskB)
        host.append(time.perf_counter() - t)
        del keys
        e.close()
    dev, host = dev[1:], host[1:]
    emit(f"{name:20s} {CLASSES.get(name, ''):34s} n {P.n:4d} N {P.N} logQ {P.Q.bit_length():2d} kernel {P.kernel} "
         f"row pairs {plan.row_pairs:6d} ksk rows {plan.ksk_rows:6d}  device {stat(dev)} ms  "
         f"host keygen + load {stat(host)} ms  x{np.median(host) / np.median(dev):.1f}{note}")
    if np.median(dev) > np.median(host):
        slower.append(name)
emit("# device slower than host keygen + load on: " + (", ".join(slower) if slower else "none"))
with open(args.out, "w") as fh:
    fh.write("# tools/keygen_time.py: median [min .. max] of %d repetitions after one warm-up, milliseconds, host clock\n"
             % args.reps)
    fh.write("\n".join(lines) + "\n")
