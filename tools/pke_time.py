"""Public-key encryption timing: Encrypt(pk) batches on the device (LARGE_DIM, SMALL_DIM, outputs device-resident),
the host EncryptN (fhe_hip_encrypt_pk, OpenMP) and one AND batch of the same count (tools/gate_time.py's method:
wall clock around the launches and a device synchronise).
    python tools/pke_time.py [--out profiles/pke_time] [--reps 7] [--counts 1 256 4096 65536] [--sets ginx std256q]
Writes <out>.txt and <out>.json: median, min and max of the repetitions after one warm-up call."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from fhe_amd import binfhe as bf  # noqa: E402
from fhe_amd._lib import check, lib, ptr, vp  # noqa: E402

SETS = {"ginx": ("STD128 GINX", bf.STD128, bf.GINX), "std256q": ("STD256Q GINX", bf.PARAMSETS.index("STD256Q"), bf.GINX)}
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/pke_time")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--counts", type=int, nargs="+", default=[1, 256, 4096, 65536])
ap.add_argument("--sets", nargs="+", default=["ginx", "std256q"])
ap.add_argument("--host-limit", type=float, default=60.0, help="skip a host run estimated above this many seconds")
args = ap.parse_args()
SEED = 1234


def dalloc(nbytes):
    d = vp()
    check(lib().fhe_hip_alloc(0, max(nbytes, 8), ctypes.byref(d)))
    return d.value


def timed(fn, reps, sync=True):
    """seconds of `reps` calls after one warm-up: (median, min, max)"""
    fn()
    if sync:
        check(lib().fhe_hip_synchronize(0))
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        if sync:
            check(lib().fhe_hip_synchronize(0))
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), min(ts), max(ts)


rows, lines = [], []


def emit(s):
    print(s, flush=True)
    lines.append(s)


for key in args.sets:
    label, ps, m = SETS[key]
    e = bf.GateEngine(ps, m)
    P = e.params
    t0 = time.time()
    sk = bf.keygen_secret(ps, m, SEED)
    e.keygen_device(sk, SEED)
    skN = bf.keygen_ring_secret(ps, m, SEED)
    A, v = e.pubkeygen_device(skN, SEED, export=True)
    emit(f"# {label}: n {P.n} N {P.N} Q {P.Q}; keys and public key in {time.time() - t0:.1f} s; "
         f"kernel tile {bf.encrypt_pk_tile()} ciphertexts")
    host_rate = None   # seconds per ciphertext of the last host run
    for B in args.counts:
        x1, x2 = (np.arange(B) % 2).astype(np.int32), ((np.arange(B) // 2) % 2).astype(np.int32)
        d1, d2 = dalloc(B * 4), dalloc(B * 4)
        check(lib().fhe_hip_copy_to_device(vp(d1), ptr(x1), x1.nbytes))
        check(lib().fhe_hip_copy_to_device(vp(d2), ptr(x2), x2.nbytes))
        dla, dlb = dalloc(B * P.N * 8), dalloc(B * 8)
        sa = [dalloc(B * P.n * 8) for _ in range(3)]
        sb = [dalloc(B * 8) for _ in range(3)]
        large = timed(lambda: e.encrypt_pk_device(d1, B, SEED + 1, dla, dlb, 4, bf.LARGE_DIM), args.reps)
        small = timed(lambda: e.encrypt_pk_device(d1, B, SEED + 1, sa[0], sb[0], 4, bf.SMALL_DIM), args.reps)
        e.encrypt_pk_device(d2, B, SEED + 2, sa[1], sb[1], 4, bf.SMALL_DIM)
        gate = timed(lambda: e.eval_gate_device(bf.AND, B, sa[0], sb[0], sa[1], sb[1], sa[2], sb[2]), args.reps)
        k = min(B, 64)   # the gate's outputs decrypt to the truth table (first ciphertexts)
        ao, bo = np.zeros((k, P.n), np.uint64), np.zeros(k, np.uint64)
        check(lib().fhe_hip_copy_to_host(ptr(ao), vp(sa[2]), ao.nbytes))
        check(lib().fhe_hip_copy_to_host(ptr(bo), vp(sb[2]), bo.nbytes))
        ok = bool(np.array_equal(bf.decrypt(ps, m, sk, ao, bo), (x1 & x2)[:k]))
        for d in [d1, d2, dla, dlb] + sa + sb:
            check(lib().fhe_hip_free(vp(d)))
        host, hreps = None, args.reps if B <= 4096 else 3
        if host_rate is None or host_rate * B <= args.host_limit:
            host = timed(lambda: bf.encrypt_pk(ps, m, A, v, x1, SEED + 1, 4), hreps, sync=False)
            host_rate = host[0] / B
        row = {"set": label, "count": B, "reps": args.reps, "device_large_ms": [t * 1e3 for t in large],
               "device_small_ms": [t * 1e3 for t in small], "and_gate_ms": [t * 1e3 for t in gate],
               "host_ms": [t * 1e3 for t in host] if host else None, "host_reps": hreps if host else 0,
               "gate_correct": ok}
        rows.append(row)
        f = lambda t: f"{t[0] * 1e3:10.3f} [{t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f}]"  # noqa: E731
        emit(f"{label:13s} count {B:6d}  LARGE_DIM {f(large)} ms  SMALL_DIM {f(small)} ms  AND {f(gate)} ms  "
             f"host {(f(host) + f' ms ({hreps} reps)') if host else 'skipped (estimated above the limit)'}  "
             f"gate correct={ok}")
    e.close()

with open(args.out + ".txt", "w") as fh:
    fh.write("# tools/pke_time.py: median [min .. max] of the repetitions after one warm-up, milliseconds\n")
    fh.write("\n".join(lines) + "\n")
with open(args.out + ".json", "w") as fh:
    json.dump(rows, fh, indent=1)
