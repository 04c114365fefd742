"""Circuits on the GPU (Engine::eval_circuit_device): every level of a DAG of mixed gate types as one indexed
prep + blind rotation + key switch.  All comparisons are bit for bit against the same nodes evaluated one by
one through the existing, golden-pinned entry points (eval_gate, eval_cmux, bootstrap) and host EvalNOT."""
import ctypes

import numpy as np
import pytest

from fhe_amd import binfhe as bf
from oracle_lib import Ref, ref_available

OR, AND, NOR, NAND, XOR, XNOR = bf.OR, bf.AND, bf.NOR, bf.NAND, bf.XOR, bf.XNOR
TRUTH = {OR: lambda x, y: x | y, AND: lambda x, y: x & y, NOR: lambda x, y: 1 - (x | y), NAND: lambda x, y: 1 - (x & y),
         XOR: lambda x, y: x ^ y, XNOR: lambda x, y: 1 - (x ^ y)}
STD128_3 = 4   # digitsG = 4, qKS = 2^16: the 64-bit path with the split in-register kernel (fhe_hip_params.kernel 2)
SETS = {"ginx": (bf.STD128, bf.GINX), "lmkcdey": (bf.STD128_LMKCDEY, bf.LMKCDEY), "ap": (bf.STD128_AP, bf.AP),
        "std128_3": (STD128_3, bf.GINX)}

_ctx = {}


def context(name):
    """(engine, sk, raw keys or None), one per parameter set for the whole module"""
    if name not in _ctx:
        ps, m = SETS[name]
        seed = 0xC1AC0000 + ps
        e = bf.GateEngine(ps, m)
        if name == "ginx":   # the raw keys too: the reference is run on them
            keys = bf.keygen(ps, m, seed)
            e.load_keys(keys.bsk, keys.kskA, keys.kskB)
            _ctx[name] = (e, keys.sk, keys)
        else:
            sk = bf.keygen_secret(ps, m, seed)
            e.keygen_device(sk, seed)
            _ctx[name] = (e, sk, None)
    return _ctx[name]


# ---- a circuit as a list of ops, so that one description builds the Circuit, evaluates it node by node through
# the existing entry points, and evaluates it in the clear
def build(ops, outs):
    c = bf.Circuit()
    for op in ops:
        kind, args = op[0], op[1:]
        {"in": c.input, "not": c.not_, "gate": c.gate, "cmux": c.cmux, "boot": c.bootstrap}[kind](*args)
    for o in outs:
        c.output(o)
    return c.finalize()


def host_not(a, b, q):
    """EvalNOT (binfhe-base-scheme.cpp:223-236)"""
    return (q - a) % q, ((q >> 2) + q - b) % q


def node_by_node(e, ops, a_in, b_in, gate_fn=None):
    q = e.params.q
    gate_fn = gate_fn or e.eval_gate
    vals, k = [], 0
    for op in ops:
        kind, args = op[0], op[1:]
        if kind == "in":
            vals.append((a_in[k].copy(), b_in[k].copy()))
            k += 1
        elif kind == "not":
            vals.append(host_not(*vals[args[0]], q))
        elif kind == "gate":
            vals.append(gate_fn(args[0], *vals[args[1]], *vals[args[2]]))
        elif kind == "cmux":
            vals.append(e.eval_cmux(*vals[args[0]], *vals[args[1]], *vals[args[2]]))
        else:
            vals.append(e.bootstrap(*vals[args[0]]))
    return vals


def in_clear(ops, bits):
    vals, k = [], 0
    for op in ops:
        kind, args = op[0], op[1:]
        if kind == "in":
            vals.append(bits[k])
            k += 1
        elif kind == "not":
            vals.append(1 - vals[args[0]])
        elif kind == "gate":
            vals.append(TRUTH[args[0]](vals[args[1]], vals[args[2]]))
        elif kind == "cmux":
            vals.append(np.where(vals[args[2]] == 1, vals[args[1]], vals[args[0]]))
        else:
            vals.append(vals[args[0]])
    return vals


def encrypt_inputs(name, n_in, B, seed):
    ps, m = SETS[name]
    _, sk, _ = context(name)
    bits = np.random.default_rng(seed).integers(0, 2, (n_in, B))
    a, b = bf.encrypt(ps, m, sk, bits.reshape(-1), seed)
    return bits, a.reshape(n_in, B, -1), b.reshape(n_in, B)


def check_outputs(name, ops, outs, got, want_nodes, bits):
    ps, m = SETS[name]
    _, sk, _ = context(name)
    ao, bo = got
    clear = in_clear(ops, bits)
    for j, o in enumerate(outs):
        wa, wb = want_nodes[o]
        assert np.array_equal(ao[j], wa) and np.array_equal(bo[j], wb), f"output {j} (node {o}: {ops[o]})"
        assert np.array_equal(bf.decrypt(ps, m, sk, ao[j], bo[j]), clear[o]), f"output {j} decrypts wrong"


def mixed_circuit():
    """8 inputs; level 1: one gate of each of the six types on distinct pairs, XOR and AND with the first, the second
    and both operands negated, a BOOTSTRAP, the CMUX's first two NANDs (15 slots per instance); level 2: level-1
    outputs mixed with raw inputs, g_or used twice, the CMUX's last NAND (6); level 3: one gate"""
    ops = [("in",)] * 8
    add = lambda *op: (ops.append(op), len(ops) - 1)[1]   # noqa: E731
    i = list(range(8))
    g_or, g_and = add("gate", OR, i[0], i[1]), add("gate", AND, i[2], i[3])
    g_nor, g_nand = add("gate", NOR, i[4], i[5]), add("gate", NAND, i[6], i[7])
    g_xor, g_xnor = add("gate", XOR, i[0], i[2]), add("gate", XNOR, i[1], i[3])
    nt = [add("not", x) for x in i]
    add("gate", XOR, nt[4], i[6]), add("gate", XOR, i[5], nt[7]), add("gate", XOR, nt[4], nt[7])
    add("gate", AND, nt[0], i[5]), add("gate", AND, i[1], nt[6]), add("gate", AND, nt[2], nt[7])
    bt = add("boot", i[3])
    mx = add("cmux", i[0], i[1], i[2])
    add("gate", AND, g_or, i[4])
    h2 = add("gate", XOR, g_or, g_and)
    h3 = add("gate", OR, add("not", g_nor), i[7])
    add("gate", NOR, bt, g_nand)
    add("gate", NAND, g_xor, add("not", g_xnor))
    last = add("gate", XNOR, h2, mx)
    outs = [i[6], nt[1], add("not", g_nand), h3, last]   # a raw input, NOT input, NOT gate, a mid-level node, the last
    return ops, outs


_mixed = {}


def mixed_case(name, B):
    """circuit 1 on one parameter set: inputs, the circuit's outputs, and the node-by-node reference (computed once,
    shared by the tests that need it)"""
    if (name, B) not in _mixed:
        e, _, _ = context(name)
        ops, outs = mixed_circuit()
        bits, a_in, b_in = encrypt_inputs(name, 8, B, 0xC1 + B)
        c = build(ops, outs)
        assert (c.num_levels, c.level(1)[0], c.level(2)[0], c.level(3)[0], c.num_bootstraps) == (3, 15, 6, 1, 22)
        got = e.eval_circuit(c, a_in, b_in)
        want = node_by_node(e, ops, a_in, b_in)
        _mixed[(name, B)] = (c, ops, outs, bits, a_in, b_in, got, want)
    return _mixed[(name, B)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(SETS))
def test_gpu_mixed_levels_equal_the_per_gate_path(name, B):
    c, ops, outs, bits, a_in, b_in, got, want = mixed_case(name, B)
    check_outputs(name, ops, outs, got, want, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ginx", "lmkcdey"])
def test_gpu_level_past_one_prep_block(name):
    """one level of 7 mixed gates x 10 instances = 70 slots: past one 64-thread block's worth of slots, and past
    the first workgroups of the wave-per-gate op-list prep (4 gates each)"""
    e, _, _ = context(name)
    ops = [("in",)] * 6
    ops += [("gate", OR, 0, 1), ("gate", XOR, 2, 3), ("not", 4), ("gate", AND, 8, 5), ("gate", NOR, 1, 2),
            ("boot", 3), ("gate", XNOR, 8, 0), ("gate", NAND, 5, 2)]
    outs = [6, 7, 9, 10, 11, 12, 13]
    bits, a_in, b_in = encrypt_inputs(name, 6, 10, 0xC2)
    c = build(ops, outs)
    assert (c.num_levels, c.level(1)[0]) == (1, 7)
    check_outputs(name, ops, outs, e.eval_circuit(c, a_in, b_in), node_by_node(e, ops, a_in, b_in), bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ginx", "lmkcdey"])
def test_gpu_chunked_levels_give_the_same_outputs(name):
    """set_max_slots(4): level 1's 45 slots run as 12 launches (the last of 1 slot), cut across nodes and instances"""
    c, ops, outs, bits, a_in, b_in, got, want = mixed_case(name, 3)
    e, _, _ = context(name)
    c.set_max_slots(4)
    try:
        ao, bo = e.eval_circuit(c, a_in, b_in)
    finally:
        c.set_max_slots(0)
    assert np.array_equal(ao, got[0]) and np.array_equal(bo, got[1])
    check_outputs(name, ops, outs, (ao, bo), want, bits)


def adder(k):
    """k-bit ripple-carry adder from XOR, AND and OR: inputs x0..x(k-1), y0..y(k-1); outputs s0..s(k-1), carry"""
    ops = [("in",)] * (2 * k)
    add = lambda *op: (ops.append(op), len(ops) - 1)[1]   # noqa: E731
    outs, carry = [], None
    for j in range(k):
        x, y = j, k + j
        t = add("gate", XOR, x, y)
        g = add("gate", AND, x, y)
        if carry is None:
            outs.append(t)
            carry = g
        else:
            outs.append(add("gate", XOR, t, carry))
            carry = add("gate", OR, g, add("gate", AND, t, carry))
    return ops, outs + [carry]


@pytest.mark.gpu
@pytest.mark.skipif(not ref_available(), reason="reference oracle not built")
def test_gpu_two_bit_adder_equals_the_reference_node_by_node():
    e, _, keys = context("ginx")
    ref = Ref(*SETS["ginx"])
    ref.load_keys(keys.bsk, keys.kskA, keys.kskB)
    ops, outs = adder(2)
    every = [i for i, op in enumerate(ops) if op[0] == "gate"]
    bits, a_in, b_in = encrypt_inputs("ginx", 4, 2, 0xC4)
    want = node_by_node(e, ops, a_in, b_in, gate_fn=ref.eval_gate)
    check_outputs("ginx", ops, every, e.eval_circuit(build(ops, every), a_in, b_in), want, bits)


@pytest.mark.gpu
def test_gpu_four_bit_adder_and_batchdag_mirror():
    e, sk, _ = context("ginx")
    ps, m = SETS["ginx"]
    ops, outs = adder(4)
    B = 5
    bits, a_in, b_in = encrypt_inputs("ginx", 8, B, 0xC5)
    ao, bo = e.eval_circuit(build(ops, outs), a_in, b_in)
    dec = np.stack([bf.decrypt(ps, m, sk, ao[j], bo[j]) for j in range(5)])
    w = 1 << np.arange(4)
    x, y = (bits[:4] * w[:, None]).sum(0), (bits[4:] * w[:, None]).sum(0)
    assert np.array_equal((dec * (1 << np.arange(5))[:, None]).sum(0), (x + y) % 32)
    # the BatchDAG mirror, on instance 0
    cc = bf.BinFHEContext()
    cc.paramset, cc.method, cc.params, cc.engine = ps, m, e.params, e
    dag = bf.BatchDAG(cc)
    ids = []
    for op in ops:
        if op[0] == "in":
            k = len(ids)
            ids.append(dag.AddCiphertext(bf.LWECiphertext(a_in[k, 0], int(b_in[k, 0]), e.params.q)))
        else:
            ids.append(dag.AddBinGate(op[1], ids[op[2]], ids[op[3]]))
    assert dag.Execute()
    for j, o in enumerate(outs):
        r = dag.GetResult(ids[o])
        assert np.array_equal(r.a, ao[j, 0]) and r.b == int(bo[j, 0])
    cc.engine = None


@pytest.mark.gpu
def test_gpu_device_entry_queued_twice_without_synchronising():
    from fhe_amd._lib import check, lib, ptr, vp
    e, _, _ = context("ginx")
    L = lib()
    ops, outs = adder(2)
    c = build(ops, outs)
    n, B = e.params.n, 3
    cases = [encrypt_inputs("ginx", 4, B, s) for s in (0xC6, 0xC7)]
    want = [e.eval_circuit(c, a, b) for _, a, b in cases]
    ptrs = []

    def dev(nbytes, x=None):
        d = vp()
        check(L.fhe_hip_alloc(0, nbytes, ctypes.byref(d)))
        ptrs.append(d)
        if x is not None:
            check(L.fhe_hip_copy_to_device(d, ptr(np.ascontiguousarray(x)), nbytes))
        return d.value

    try:
        bufs = [(dev(a.nbytes, a), dev(b.nbytes, b), dev(len(outs) * B * n * 8), dev(len(outs) * B * 8))
                for _, a, b in cases]
        for da, db, dao, dbo in bufs:   # both queued on the context's stream, no synchronisation in between
            e.eval_circuit_device(c, B, da, db, dao, dbo)
        check(L.fhe_hip_synchronize(0))
        for (_, _, dao, dbo), (wa, wb) in zip(bufs, want):
            ga, gb = np.zeros_like(wa), np.zeros_like(wb)
            check(L.fhe_hip_copy_to_host(ptr(ga), vp(dao), ga.nbytes))
            check(L.fhe_hip_copy_to_host(ptr(gb), vp(dbo), gb.nbytes))
            assert np.array_equal(ga, wa) and np.array_equal(gb, wb)
        assert not np.array_equal(want[0][0], want[1][0])
    finally:
        for d in ptrs:
            L.fhe_hip_free(d)
