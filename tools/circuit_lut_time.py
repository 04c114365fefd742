"""A LUT circuit over B independent instances, device resident, two ways.  The workload: `chains` independent chains
(16), each from two inputs, each `steps` (3) steps of s = LINEAR(u + w + c), u = FUNC(s, lutA), w = FUNC(s, lutB) with
two periodic LUTs (digit arithmetic's shape: a sum, then several LUTs of it).

  arm A  GateEngine.eval_circuit_device: per step one LINEAR launch, one launch for the shared first stages
         (chains slots x B) and one for the second stages (2 chains slots x B)
  arm B  one eval_func_device(count = B) per FUNC node (2 chains per step, two bootstraps each, its table built and
         uploaded per call), the sums on the device.  The library has no other public device entry for an LWE sum, so
         arm B's sums are a LINEAR-only circuit, one call per step over all chains: arm B therefore runs in this
         tree only, on a context of its own (same keys) so that neither arm evicts the other's resident descriptors.

Both arms run in one process, alternating, and arm A's outputs must equal arm B's bit for bit.  Times are a host
clock around the enqueue of one whole evaluation ending in a device synchronise; every (arm, B) is warmed up first.
The spread of a series is (max - min) / median over its repetitions.

    python tools/circuit_lut_time.py [--B 1 16 256] [--reps 7] [--chains 16] [--steps 3] [--out f.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from fhe_amd import binfhe as bf  # noqa: E402
from fhe_amd._lib import check, lib, lib_path, ptr, vp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ps, m = bf.STD128, bf.GINX
    L = lib()
    sk = bf.keygen_secret(ps, m, 1234)
    engines = []
    for _ in range(2):      # one context per arm, identical keys
        e = bf.GateEngine(ps, m)
        e.keygen_device(sk, 1234)
        engines.append(e)
    ea, eb = engines
    n, q, C, S = ea.params.n, ea.params.q, args.chains, args.steps
    x = np.arange(q, dtype=np.uint64)
    lut_a = ((x % (q // 2)) // (q // 8) * (q // 8)).astype(np.uint64)           # periodic
    lut_b = (((x + q // 16) % (q // 2)) // (q // 8) * (q // 8)).astype(np.uint64)
    const = q // 16

    # arm A: the whole workload as one circuit; outputs u_0..u_(C-1), w_0..w_(C-1) of the last step
    big = bf.Circuit()
    u = [big.input() for _ in range(C)]
    w = [big.input() for _ in range(C)]
    for _ in range(S):
        s = [big.linear([u[j], w[j]], None, const) for j in range(C)]
        u = [big.func(s[j], lut_a) for j in range(C)]
        w = [big.func(s[j], lut_b) for j in range(C)]
    for o in u + w:
        big.output(o)
    big.finalize()
    # arm B's sums: inputs u_0.., w_0.. -> s_j
    lin = bf.Circuit()
    lu = [lin.input() for _ in range(C)]
    lw = [lin.input() for _ in range(C)]
    for j in range(C):
        lin.output(lin.linear([lu[j], lw[j]], None, const))
    lin.finalize()
    levels = [big.level_classes(i) for i in range(big.num_levels + 1)]
    held = []

    def dalloc(nbytes):
        d = vp()
        check(L.fhe_hip_alloc(0, nbytes, ctypes.byref(d)))
        held.append(d)
        return d.value

    def fetch(d, shape):
        out = np.zeros(shape, np.uint64)
        check(L.fhe_hip_copy_to_host(ptr(out), vp(d), out.nbytes))
        return out

    record = {"set": "ginx", "chains": C, "steps": S, "func_nodes": 2 * C * S, "bootstraps_a": big.num_bootstraps,
              "bootstraps_b": 4 * C * S, "level_classes": levels, "reps": args.reps, "lib": os.path.basename(lib_path), "rows": []}
    for B in args.B:
        bits = np.random.default_rng(B).integers(0, 2, (2 * C, B))
        a_in, b_in = bf.encrypt(ps, m, sk, bits.reshape(-1), 99)
        d_ain, d_bin = dalloc(a_in.nbytes), dalloc(b_in.nbytes)          # [2C][B][n], [2C][B]: both arms read it
        check(L.fhe_hip_copy_to_device(vp(d_ain), ptr(a_in), a_in.nbytes))
        check(L.fhe_hip_copy_to_device(vp(d_bin), ptr(b_in), b_in.nbytes))
        d_ao, d_bo = dalloc(2 * C * B * n * 8), dalloc(2 * C * B * 8)    # arm A's outputs
        d_sa, d_sb = dalloc(C * B * n * 8), dalloc(C * B * 8)            # arm B: the step's sums
        d_ua, d_ub = dalloc(2 * C * B * n * 8), dalloc(2 * C * B * 8)    # arm B: the step's u_j, w_j
        kernels = {"first stages": ea.gate_kernel(C * B), "second stages": ea.gate_kernel(2 * C * B),
                   "arm B": eb.gate_kernel(B)}

        def arm_a():
            ea.eval_circuit_device(big, B, d_ain, d_bin, d_ao, d_bo)

        def arm_b():
            src_a, src_b = d_ain, d_bin
            for _ in range(S):
                eb.eval_circuit_device(lin, B, src_a, src_b, d_sa, d_sb)
                for j in range(C):
                    for k, lut in enumerate((lut_a, lut_b)):
                        row = k * C + j
                        check(L.fhe_hip_eval_func_batch_device(eb._h, B, vp(d_sa + j * B * n * 8), vp(d_sb + j * B * 8), q,
                                                               ptr(lut), lut.size, vp(d_ua + row * B * n * 8),
                                                               vp(d_ub + row * B * 8), None))
                src_a, src_b = d_ua, d_ub

        run = {"a": arm_a, "b": arm_b}
        for arm in "ab":       # warm-up: code objects, workspaces, descriptors
            run[arm]()
        check(L.fhe_hip_synchronize(0))
        assert np.array_equal(fetch(d_ao, (2 * C, B, n)), fetch(d_ua, (2 * C, B, n))), B      # bit for bit
        assert np.array_equal(fetch(d_bo, (2 * C, B)), fetch(d_ub, (2 * C, B))), B
        times = {arm: [] for arm in "ab"}
        for _ in range(args.reps):      # alternating arms
            for arm in "ab":
                t = time.perf_counter()
                run[arm]()
                check(L.fhe_hip_synchronize(0))
                times[arm].append(time.perf_counter() - t)
        row = {"B": B, "identical": True, "kernels": kernels}
        for arm in "ab":
            t = np.array(times[arm])
            med = float(np.median(t))
            row[arm] = {"median_ms": 1e3 * med, "min_ms": 1e3 * float(t.min()), "max_ms": 1e3 * float(t.max()),
                        "spread": float((t.max() - t.min()) / med)}
        row["b_over_a"] = row["b"]["median_ms"] / row["a"]["median_ms"]
        record["rows"].append(row)
        print(json.dumps(row), flush=True)
        for d in held:
            check(L.fhe_hip_free(d))
        held.clear()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
