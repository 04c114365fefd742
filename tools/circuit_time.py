"""A k-bit ripple-carry adder (XOR, AND, OR) over B independent instances, device resident, two ways:

  arm A  GateEngine.eval_circuit_device: one prep + blind rotation + key switch per LEVEL of the DAG
  arm B  what a caller could do before circuits existed: one eval_gate_device(count = B) per gate node, on
         per-node device columns (entry points of the parent commit only)

Both arms run in one process, alternating, and arm A's outputs must equal arm B's bit for bit; the sums are also
decrypted, and the instances whose sum is wrong (decryption failures of the scheme) are counted.  Times are a host
clock around the enqueue of one whole adder ending in a device synchronise; every (arm, B) is warmed up first.

    python tools/circuit_time.py [--set ginx|lmk] [--k 16] [--B 1 16 256 4096] [--reps 7] [--arms a b] [--out f.json]
                                 [--carry andor|majority]

--carry majority builds the adder with carry = MAJORITY(x, y, carry) at plaintext modulus 4 instead (3k - 1 gates on k
levels against 5k - 3 on 2k - 1); arm B is then one eval_gate_device / eval_gate_multi_device per node.  With arm A
selected, the AND/OR adder's circuit runs as a third arm "a_andor" alternating with the others, on the same inputs,
so that both carry forms are timed in one process; its wrong sums are counted separately.  Three-operand sums
carry more noise than two-operand ones: the wrong-sum counts are a property of the parameter set, recorded here.

Arm B alone also runs from a checkout and build of the parent commit (--arms b, which touches no circuit entry
point): its time THERE is the baseline arm A is held against, not arm B's time in the tree under test.  The spread of a series is
(max - min) / median over its repetitions; --series N repeats the whole measurement N times to show the
run-to-run spread of the medians."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from fhe_amd import binfhe as bf  # noqa: E402
from fhe_amd._lib import check, lib, lib_path, ptr, vp  # noqa: E402

SETS = {"ginx": (bf.STD128, bf.GINX), "lmk": (bf.STD128_LMKCDEY, bf.LMKCDEY)}


def adder(k, form="andor"):
    """(ops, outs): ops[i] = None (input), (gate, x, y) or (MAJORITY, x, y, z); inputs x0..x(k-1), y0..y(k-1); outs
    s0..s(k-1), carry"""
    ops = [None] * (2 * k)
    add = lambda *op: (ops.append(op), len(ops) - 1)[1]   # noqa: E731
    outs, carry = [], None
    for j in range(k):
        t = add(bf.XOR, j, k + j)
        g = add(bf.AND, j, k + j) if form == "andor" or carry is None else None
        if carry is None:
            outs.append(t)
            carry = g
        else:
            outs.append(add(bf.XOR, t, carry))
            carry = add(bf.OR, g, add(bf.AND, t, carry)) if form == "andor" else add(bf.MAJORITY, j, k + j, carry)
    return ops, outs + [carry]


def circuit(ops, outs):
    circ = bf.Circuit()
    for op in ops:
        if not op:
            circ.input()
        elif len(op) == 3:
            circ.gate(*op)
        else:
            circ.gate_multi(op[0], op[1:], 4)
    for o in outs:
        circ.output(o)
    return circ.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="ginx", choices=list(SETS))
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--series", type=int, default=1)
    ap.add_argument("--arms", nargs="+", default=["a", "b"], choices=["a", "b"])
    ap.add_argument("--carry", default="andor", choices=["andor", "majority"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ps, m = SETS[args.set]
    L = lib()
    e = bf.GateEngine(ps, m)
    sk = bf.keygen_secret(ps, m, 1234)
    e.keygen_device(sk, 1234)
    n, k = e.params.n, args.k
    ops, outs = adder(k, args.carry)
    gates = [i for i, op in enumerate(ops) if op]
    circ = circuit(ops, outs) if "a" in args.arms else None
    # the other carry form's circuit, timed alongside
    other = circuit(*adder(k)) if circ and args.carry == "majority" else None
    arms = args.arms + (["a_andor"] if other else [])
    ngates = {"a": len(gates), "b": len(gates), "a_andor": 5 * k - 3}
    held = []

    def dalloc(nbytes):
        d = vp()
        check(L.fhe_hip_alloc(0, nbytes, ctypes.byref(d)))
        held.append(d)
        return d.value

    def fetch(d, shape):
        x = np.zeros(shape, np.uint64)
        check(L.fhe_hip_copy_to_host(ptr(x), vp(d), x.nbytes))
        return x

    record = {"set": args.set, "k": k, "gates": len(gates), "levels": circ.num_levels if circ else None,
              "reps": args.reps, "arms": args.arms, "lib": lib_path, "rows": []}
    if args.carry != "andor":
        record["carry"] = args.carry
        record["andor"] = {"gates": ngates["a_andor"], "levels": other.num_levels} if other else None
    for B in args.B:
        rng = np.random.default_rng(B)
        bits = rng.integers(0, 2, (2 * k, B))
        a_in, b_in = bf.encrypt(ps, m, sk, bits.reshape(-1), 99)
        d_ain, d_bin = dalloc(a_in.nbytes), dalloc(b_in.nbytes)          # [2k][B][n], [2k][B]: both arms read it
        check(L.fhe_hip_copy_to_device(vp(d_ain), ptr(a_in), a_in.nbytes))
        check(L.fhe_hip_copy_to_device(vp(d_bin), ptr(b_in), b_in.nbytes))
        # arm B's per-node columns: inputs are slices of the input arrays, every gate node gets its own column
        col = {i: (d_ain + i * B * n * 8, d_bin + i * B * 8) for i in range(2 * k)}
        if "b" in args.arms:
            for i in gates:
                col[i] = (dalloc(B * n * 8), dalloc(B * 8))
        d_ao, d_bo = dalloc(len(outs) * B * n * 8), dalloc(len(outs) * B * 8)
        d_ao2, d_bo2 = (dalloc(len(outs) * B * n * 8), dalloc(len(outs) * B * 8)) if other else (None, None)

        def arm_a():
            e.eval_circuit_device(circ, B, d_ain, d_bin, d_ao, d_bo)

        def arm_b():
            for i in gates:
                if len(ops[i]) == 3:
                    g, x, y = ops[i]
                    e.eval_gate_device(g, B, *col[x], *col[y], *col[i])
                else:
                    xs = ops[i][1:]
                    e.eval_gate_multi_device(ops[i][0], B, 4, [col[x][0] for x in xs], [col[x][1] for x in xs], *col[i])

        def arm_a_andor():
            e.eval_circuit_device(other, B, d_ain, d_bin, d_ao2, d_bo2)

        run = {"a": arm_a, "b": arm_b, "a_andor": arm_a_andor}
        for arm in arms:            # warm-up: code objects, workspaces, the circuit's descriptors
            run[arm]()
        check(L.fhe_hip_synchronize(0))
        if len(args.arms) == 2:     # bit for bit, at the size that is timed
            for j, o in enumerate(outs):
                assert np.array_equal(fetch(d_ao + j * B * n * 8, (B, n)), fetch(col[o][0], (B, n))), (B, j)
                assert np.array_equal(fetch(d_bo + j * B * 8, (B,)), fetch(col[o][1], (B,))), (B, j)
        last = "a" if "a" in args.arms else "b"
        oa = fetch(d_ao, (len(outs), B, n)) if last == "a" else np.stack([fetch(col[o][0], (B, n)) for o in outs])
        ob = fetch(d_bo, (len(outs), B)) if last == "a" else np.stack([fetch(col[o][1], (B,)) for o in outs])
        dec = np.stack([bf.decrypt(ps, m, sk, oa[j], ob[j]) for j in range(len(outs))])
        w = 1 << np.arange(k, dtype=object)
        x, y = (bits[:k] * w[:, None]).sum(0), (bits[k:] * w[:, None]).sum(0)
        wsum = (1 << np.arange(k + 1, dtype=object))[:, None]
        got = (dec * wsum).sum(0)
        # decryption failures are the scheme's (XOR doubles the noise of its input sum; the reference computes the
        # same ciphertexts): counted, not hidden -- but a circuit that is wrong everywhere is a bug
        wrong = int(np.sum(got != x + y))
        assert wrong * 100 <= B, f"adder is wrong for {wrong} of {B} instances"
        wrong2 = None
        if other:
            o2a, o2b = fetch(d_ao2, (len(outs), B, n)), fetch(d_bo2, (len(outs), B))
            dec2 = np.stack([bf.decrypt(ps, m, sk, o2a[j], o2b[j]) for j in range(len(outs))])
            wrong2 = int(np.sum((dec2 * wsum).sum(0) != x + y))
        for series in range(args.series):
            times = {arm: [] for arm in arms}
            for _ in range(args.reps):      # alternating arms
                for arm in arms:
                    t = time.perf_counter()
                    run[arm]()
                    check(L.fhe_hip_synchronize(0))
                    times[arm].append(time.perf_counter() - t)
            row = {"B": B, "series": series, "identical": len(args.arms) == 2, "wrong_sums": wrong}
            if other:
                row["wrong_sums_andor"] = wrong2
            for arm in arms:
                t = np.array(times[arm])
                med = float(np.median(t))
                row[arm] = {"median_ms": 1e3 * med, "min_ms": 1e3 * float(t.min()), "max_ms": 1e3 * float(t.max()),
                            "spread": float((t.max() - t.min()) / med), "gates_per_s": ngates[arm] * B / med}
            if other:
                row["andor_over_majority"] = row["a_andor"]["median_ms"] / row["a"]["median_ms"]
            record["rows"].append(row)
            print(json.dumps(row), flush=True)
        for d in held:
            check(L.fhe_hip_free(d))
        held.clear()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    e.close()


if __name__ == "__main__":
    main()
