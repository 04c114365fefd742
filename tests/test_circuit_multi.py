"""Multi-input gates inside circuits on the GPU: MAJORITY at p = 4 in the level's one gate launch, AND3 / OR3 (p = 6)
and AND4 / OR4 (p = 8) in one more launch per plaintext modulus.  Pinned to the reference's goldens one node at a
time, and bit for bit to the same nodes evaluated one by one through eval_gate, eval_gate_multi, eval_cmux and
host EvalNOT."""
import ctypes

import numpy as np
import pytest

from fhe_amd import binfhe as bf
from fhe_amd._lib import FheHipError
import test_circuit as tc          # its contexts (one per parameter set and session) and helpers
import test_multi_gates as tm      # the goldens of the per-gate path and the engines loaded with their keys

MAJ, AND3, OR3, AND4, OR4 = bf.MAJORITY, bf.AND3, bf.OR3, bf.AND4, bf.OR4
TRUTH_MULTI = {MAJ: lambda v: (sum(v) >= 2).astype(np.int64), AND3: lambda v: np.prod(v, 0), AND4: lambda v: np.prod(v, 0),
               OR3: lambda v: (sum(v) >= 1).astype(np.int64), OR4: lambda v: (sum(v) >= 1).astype(np.int64)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", tm.SETS)
def test_gpu_single_node_circuits_equal_the_reference_goldens(name):
    """k inputs and one node, B = every input combination of the golden: the reference's own outputs, bit for bit"""
    g, keys, cases = tm.fixture(name)
    e = tm.engine(name)
    seen = set()
    for gname, (gate, k, p, bits, A, B) in cases.items():
        if gname == "CMUX":
            continue
        c = bf.Circuit()
        c.output(c.gate_multi(gate, [c.input() for _ in range(k)], p))
        c.finalize()
        assert len(B[0]) == 2 ** k
        assert c.level_classes(1)[0] == (p == 4) and c.level_gate_classes(1) == ([] if p == 4 else [(p, 1)])
        ao, bo = e.eval_circuit(c, np.stack(A), np.stack(B))
        assert np.array_equal(ao[0], g[f"{gname}_out_a"]), gname
        assert np.array_equal(bo[0], g[f"{gname}_out_b"]), gname
        seen.add(gate)
    assert seen == {MAJ, AND3, OR3, AND4, OR4}


# ---- the mixed circuit: tc's op lists with one more kind, ("multi", gate, [operands], p); every node's plaintext
# modulus is tracked so that each output is decrypted at its own
IN_P = [4, 4, 4, 4, 6, 6, 6, 8, 8, 8, 8]


def mixed_multi_circuit():
    """11 inputs: x0..x3 at p = 4, u0..u2 at p = 6, v0..v3 at p = 8.
    level 1: AND, XNOR, MAJORITY(x0, NOT x1, x2), AND3 and OR3 (p = 6), AND4 (p = 8), MAJORITY with k = 2
    level 2: MAJORITY of three level-1 outputs (one negated), the first NANDs of a CMUX whose selector is a
             MAJORITY, OR4 over the level-1 AND4 and three inputs (p = 8), a NAND of two MAJORITY outputs
    level 3: XOR of two level-2 nodes, the CMUX's last NAND"""
    ops = [("in",)] * 11
    add = lambda *op: (ops.append(op), len(ops) - 1)[1]   # noqa: E731
    x, u, v = [0, 1, 2, 3], [4, 5, 6], [7, 8, 9, 10]
    g_and, g_xnor = add("gate", bf.AND, x[0], x[1]), add("gate", bf.XNOR, x[2], x[3])
    m1 = add("multi", MAJ, [x[0], add("not", x[1]), x[2]], 4)
    a3, o3 = add("multi", AND3, u, 6), add("multi", OR3, [u[2], u[0], u[1]], 6)
    a4 = add("multi", AND4, v, 8)
    m2 = add("multi", MAJ, [x[1], x[3]], 4)
    m3 = add("multi", MAJ, [g_and, add("not", g_xnor), m1], 4)
    mx = add("cmux", x[0], x[1], m1)
    o4 = add("multi", OR4, [a4, v[0], v[1], v[2]], 8)
    n2 = add("gate", bf.NAND, m1, m2)
    last = add("gate", bf.XOR, m3, n2)
    outs = [g_and, add("not", m1), a3, o3, a4, m2, m3, mx, o4, last]
    return ops, outs


def build(ops, outs):
    c = bf.Circuit()
    for op in ops:
        kind, args = op[0], op[1:]
        {"in": c.input, "not": c.not_, "gate": c.gate, "cmux": c.cmux, "multi": c.gate_multi}[kind](*args)
    for o in outs:
        c.output(o)
    return c.finalize()


def node_by_node(e, ops, a_in, b_in):
    q = e.params.q
    vals, k = [], 0
    for op in ops:
        kind, args = op[0], op[1:]
        if kind == "in":
            vals.append((a_in[k].copy(), b_in[k].copy()))
            k += 1
        elif kind == "not":
            vals.append(tc.host_not(*vals[args[0]], q))
        elif kind == "gate":
            vals.append(e.eval_gate(args[0], *vals[args[1]], *vals[args[2]]))
        elif kind == "cmux":
            vals.append(e.eval_cmux(*vals[args[0]], *vals[args[1]], *vals[args[2]]))
        else:
            vals.append(e.eval_gate_multi(args[0], [vals[j][0] for j in args[1]], [vals[j][1] for j in args[1]], args[2]))
    return vals


def in_clear(ops, bits, in_p):
    """(value, plaintext modulus) per node; in_p: the inputs' plaintext moduli"""
    vals, k = [], 0
    for op in ops:
        kind, args = op[0], op[1:]
        if kind == "in":
            vals.append((bits[k], in_p[k]))
            k += 1
        elif kind == "not":
            assert vals[args[0]][1] == 4
            vals.append((1 - vals[args[0]][0], 4))
        elif kind == "gate":
            vals.append((tc.TRUTH[args[0]](vals[args[1]][0], vals[args[2]][0]), 4))
        elif kind == "cmux":
            vals.append((np.where(vals[args[2]][0] == 1, vals[args[1]][0], vals[args[0]][0]), 4))
        else:
            assert all(vals[j][1] == args[2] for j in args[1])          # the test wires consistent encodings
            vals.append((TRUTH_MULTI[args[0]]([vals[j][0] for j in args[1]]), args[2]))
    return vals


def encrypt_mixed(name, B, seed):
    ps, m = tc.SETS[name]
    _, sk, _ = tc.context(name)
    bits = np.random.default_rng(seed).integers(0, 2, (len(IN_P), B))
    cts = [bf.encrypt(ps, m, sk, bits[j], seed + j, IN_P[j]) for j in range(len(IN_P))]
    return bits, np.stack([c[0] for c in cts]), np.stack([c[1] for c in cts])


def check_outputs(name, ops, outs, got, want_nodes, bits, in_p=IN_P):
    ps, m = tc.SETS[name]
    _, sk, _ = tc.context(name)
    ao, bo = got
    clear = in_clear(ops, bits, in_p)
    for j, o in enumerate(outs):
        wa, wb = want_nodes[o]
        assert np.array_equal(ao[j], wa) and np.array_equal(bo[j], wb), f"output {j} (node {o}: {ops[o]})"
        assert np.array_equal(bf.decrypt(ps, m, sk, ao[j], bo[j], p=clear[o][1]), clear[o][0]), f"output {j} decrypts wrong"


_mixed = {}


def mixed_case(name, B):
    """the mixed circuit on one parameter set: inputs, its outputs and the node-by-node yardstick, computed once"""
    if (name, B) not in _mixed:
        e, _, _ = tc.context(name)
        ops, outs = mixed_multi_circuit()
        bits, a_in, b_in = encrypt_mixed(name, B, 0xD100 + B)
        c = build(ops, outs)
        assert (c.num_levels, c.num_bootstraps) == (3, 14)
        assert [c.level_classes(i) for i in (1, 2, 3)] == [(4, 0, 0, 0), (4, 0, 0, 0), (2, 0, 0, 0)]
        assert [c.level_gate_classes(i) for i in (1, 2, 3)] == [[(6, 2), (8, 1)], [(8, 1)], []]
        got = e.eval_circuit(c, a_in, b_in)
        want = node_by_node(e, ops, a_in, b_in)
        _mixed[(name, B)] = (c, ops, outs, bits, a_in, b_in, got, want)
    return _mixed[(name, B)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(tc.SETS))
def test_gpu_mixed_circuit_equals_the_per_node_path(name, B):
    c, ops, outs, bits, a_in, b_in, got, want = mixed_case(name, B)
    check_outputs(name, ops, outs, got, want, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tc.SETS))
def test_gpu_chunked_classes_give_the_same_outputs(name):
    """set_max_slots(4) at B = 3: class 0's 12 slots run as 3 launches and the p = 6 class's 6 slots as 2, cut inside
    a node's instances and between nodes"""
    c, ops, outs, bits, a_in, b_in, got, want = mixed_case(name, 3)
    e, _, _ = tc.context(name)
    c.set_max_slots(4)
    try:
        ao, bo = e.eval_circuit(c, a_in, b_in)
    finally:
        c.set_max_slots(0)
    assert np.array_equal(ao, got[0]) and np.array_equal(bo, got[1])
    check_outputs(name, ops, outs, (ao, bo), want, bits)


def majority_adder(k):
    """k-bit ripple-carry adder with carry = MAJORITY(x, y, carry): 3k - 1 gates on k levels; inputs x0..x(k-1),
    y0..y(k-1); outputs s0..s(k-1), carry"""
    ops = [("in",)] * (2 * k)
    add = lambda *op: (ops.append(op), len(ops) - 1)[1]   # noqa: E731
    outs, carry = [], None
    for j in range(k):
        t = add("gate", bf.XOR, j, k + j)
        if carry is None:
            outs.append(t)
            carry = add("gate", bf.AND, j, k + j)
        else:
            outs.append(add("gate", bf.XOR, t, carry))
            carry = add("multi", MAJ, [j, k + j, carry], 4)
    return ops, outs + [carry]


@pytest.mark.gpu
def test_gpu_four_bit_majority_adder():
    e, sk, _ = tc.context("ginx")
    ps, m = tc.SETS["ginx"]
    ops, outs = majority_adder(4)
    B = 3
    bits, a_in, b_in = tc.encrypt_inputs("ginx", 8, B, 0xD2)
    c = build(ops, outs)
    assert (c.num_levels, c.num_bootstraps) == (4, 11) and all(c.level_gate_classes(i) == [] for i in range(5))
    got = e.eval_circuit(c, a_in, b_in)
    want = node_by_node(e, ops, a_in, b_in)
    check_outputs("ginx", ops, outs, got, want, bits, in_p=[4] * 8)
    w = 1 << np.arange(4)
    x, y = (bits[:4] * w[:, None]).sum(0), (bits[4:] * w[:, None]).sum(0)
    for ao, bo in (got, ([want[o][0] for o in outs], [want[o][1] for o in outs])):   # the circuit; node by node
        dec = np.stack([bf.decrypt(ps, m, sk, ao[j], bo[j]) for j in range(5)])
        assert np.array_equal((dec * (1 << np.arange(5))[:, None]).sum(0), x + y)


@pytest.mark.gpu
def test_gpu_device_entry_queued_twice_then_another_circuit():
    """two device evaluations of the mixed circuit queued on one stream with no synchronise in between; then a
    circuit without multi-input nodes on the same context, which replaces the descriptor cache"""
    from fhe_amd._lib import check, lib, ptr, vp
    e, _, _ = tc.context("ginx")
    L = lib()
    ops, outs = mixed_multi_circuit()
    c = build(ops, outs)
    n, B = e.params.n, 3
    cases = [encrypt_mixed("ginx", B, s)[1:] for s in (0xD300, 0xD400)]
    want = [node_by_node(e, ops, a, b) for a, b in cases]
    ptrs = []

    def dev(nbytes, x=None):
        d = vp()
        check(L.fhe_hip_alloc(0, nbytes, ctypes.byref(d)))
        ptrs.append(d)
        if x is not None:
            check(L.fhe_hip_copy_to_device(d, ptr(np.ascontiguousarray(x)), nbytes))
        return d.value

    try:
        bufs = [(dev(a.nbytes, a), dev(b.nbytes, b), dev(len(outs) * B * n * 8), dev(len(outs) * B * 8)) for a, b in cases]
        for da, db, dao, dbo in bufs:   # both queued on the context's stream, no synchronisation in between
            e.eval_circuit_device(c, B, da, db, dao, dbo)
        check(L.fhe_hip_synchronize(0))
        for (_, _, dao, dbo), w in zip(bufs, want):
            ga, gb = np.zeros((len(outs), B, n), np.uint64), np.zeros((len(outs), B), np.uint64)
            check(L.fhe_hip_copy_to_host(ptr(ga), vp(dao), ga.nbytes))
            check(L.fhe_hip_copy_to_host(ptr(gb), vp(dbo), gb.nbytes))
            for j, o in enumerate(outs):
                assert np.array_equal(ga[j], w[o][0]) and np.array_equal(gb[j], w[o][1]), j
        assert not np.array_equal(want[0][outs[-1]][0], want[1][outs[-1]][0])
    finally:
        for d in ptrs:
            L.fhe_hip_free(d)
    # another circuit, no multi-input node: the descriptor cache is replaced
    ops2, outs2 = tc.adder(2)
    bits, a_in, b_in = tc.encrypt_inputs("ginx", 4, B, 0xD5)
    tc.check_outputs("ginx", ops2, outs2, e.eval_circuit(tc.build(ops2, outs2), a_in, b_in),
                     tc.node_by_node(e, ops2, a_in, b_in), bits)
    # and the mixed circuit again after it
    a, b = cases[0]
    ao, bo = e.eval_circuit(c, a, b)
    for j, o in enumerate(outs):
        assert np.array_equal(ao[j], want[0][o][0]) and np.array_equal(bo[j], want[0][o][1]), j


@pytest.mark.gpu
def test_gpu_plaintext_modulus_past_q_is_refused_at_evaluation():
    e, _, _ = tc.context("ginx")
    q, n = e.params.q, e.params.n
    c = bf.Circuit()
    c.output(c.gate_multi(AND3, [c.input(), c.input(), c.input()], q // 2 + 1))
    c.finalize()
    with pytest.raises(FheHipError) as err:
        e.eval_circuit(c, np.zeros((3, 1, n), np.uint64), np.zeros((3, 1), np.uint64))
    assert err.value.code == -2
