"""Circuits with FUNC (EvalFunc) and LINEAR nodes on the GPU: table launch classes next to the gate class in one
level, the per-slot table index in the high half of the prep's b word, LINEAR rows.  Every comparison is bit for bit:
against the reference's own EvalFunc goldens, and against the same nodes evaluated one by one through eval_gate,
bootstrap, eval_func and numpy sums mod q."""
import ctypes
import os
import sys

import numpy as np
import pytest

from fhe_amd import binfhe as bf
from fhe_amd._lib import FheHipError
import test_circuit as tc          # its contexts (one per parameter set and session) and helpers

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OR, AND, NOR, NAND, XOR, XNOR = bf.OR, bf.AND, bf.NOR, bf.NAND, bf.XOR, bf.XNOR
INVALID = -2
SETS = tc.SETS


def has_arbitrary(name):
    ps, m = SETS[name]
    P = bf.params(ps, m)
    return P.q <= P.N and m != bf.AP


def make_luts(q):
    x = np.arange(q, dtype=np.uint64)
    return {"neg": np.where(x < q // 2, q // 4, q - q // 4).astype(np.uint64),
            "neg2": np.where(x < q // 2, q // 8, q - q // 8).astype(np.uint64),
            "neg3": np.where(x < q // 2, 3 * q // 8, q - 3 * q // 8).astype(np.uint64),
            "per": ((x % (q // 2)) // (q // 8) * (q // 8)).astype(np.uint64),
            "per2": ((x % (q // 2)) // (q // 16) * (q // 16)).astype(np.uint64),
            "arb": (x * x * x % q).astype(np.uint64),
            "arb2": (x // (q // 4) * (q // 4)).astype(np.uint64)}


# ---- reference goldens -------------------------------------------------------------------------------------------
_fb = {}


def fb_fixture(name):
    if name not in _fb:
        sys.path.insert(0, GOLD)
        from make_golden import fb_inputs, fb_luts
        g = np.load(os.path.join(GOLD, f"fb_{name}.npz"))
        ps, m = int(g["paramset"]), int(g["method"])
        keys, q, p, ms, sa, sb = fb_inputs(ps, m, int(g["key_seed"]))[:6]
        e = bf.GateEngine(ps, m)
        e.load_keys(keys.bsk, keys.kskA, keys.kskB)
        _fb[name] = (g, e, sa, sb, fb_luts(q, p, e.params.N))
    return _fb[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["std128", "lmkcdey"])
def test_gpu_func_nodes_equal_the_reference_goldens(name):
    """one input, B = every golden ciphertext, one FUNC node per LUT of fb_luts (negacyclic, periodic, and the
    arbitrary cube on STD128): all classes in one circuit == the reference's EvalFunc outputs"""
    g, e, sa, sb, luts = fb_fixture(name)
    assert set(luts) == ({"neg", "per", "cube"} if name == "std128" else {"neg", "per"})
    c = bf.Circuit()
    x = c.input()
    for lut in luts.values():
        c.output(c.func(x, lut))
    c.finalize()
    assert c.num_bootstraps == (5 if name == "std128" else 3)
    B = len(sb)
    assert B in (8, 16)
    ao, bo = e.eval_circuit(c, sa.reshape(1, B, -1), sb.reshape(1, B))
    for j, lname in enumerate(luts):
        assert np.array_equal(ao[j], g[f"func_{lname}_a"].astype(np.uint64)), lname
        assert np.array_equal(bo[j], g[f"func_{lname}_b"].astype(np.uint64)), lname


# ---- node by node ------------------------------------------------------------------------------------------------
def build(ops, outs):
    c = bf.Circuit()
    for op in ops:
        kind, args = op[0], op[1:]
        if kind == "func":
            c.func(args[0], args[1])
        elif kind == "lin":
            c.linear(args[0], args[1], args[2])
        else:
            {"in": c.input, "not": c.not_, "gate": c.gate, "boot": c.bootstrap}[kind](*args)
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
        elif kind == "boot":
            vals.append(e.bootstrap(*vals[args[0]]))
        elif kind == "func":
            vals.append(e.eval_func(*vals[args[0]], q, args[1]))
        else:   # EvalAddEq / EvalSubEq / EvalAddConstEq (lwe-pke.cpp:230-246)
            xs, signs, const = args
            signs = signs or [1] * len(xs)
            a = sum(s * vals[x][0].astype(np.int64) for x, s in zip(xs, signs)) % q
            b = (sum(s * vals[x][1].astype(np.int64) for x, s in zip(xs, signs)) + const) % q
            vals.append((a.astype(np.uint64), b.astype(np.uint64)))
    return vals


def func_circuit(name):
    """6 inputs.  Level 1: six gate types and a BOOTSTRAP (7 class-0 slots), FUNC on inputs: two negacyclic LUTs and
    the shared first stage of two periodic ones (3 class-1 slots with 3 distinct tables), the first stage of an
    arbitrary one (class 2) -- all three launch classes in one level -- and a LINEAR row of three operands (one
    subtracted, one a NOT alias, a constant).  Level 2: the second stages, FUNC on gate outputs, FUNC of both
    two-stage classes and a gate on the LINEAR row.  The last level: a gate of two FUNC outputs."""
    ps, m = SETS[name]
    q = bf.params(ps, m).q
    L = make_luts(q)
    arb = has_arbitrary(name)
    ops = [("in",)] * 6
    add = lambda *op: (ops.append(op), len(ops) - 1)[1]   # noqa: E731
    g_or, g_and, g_nor = add("gate", OR, 0, 1), add("gate", AND, 2, 3), add("gate", NOR, 4, 5)
    g_nand, g_xor, g_xnor = add("gate", NAND, 0, 2), add("gate", XOR, 1, 3), add("gate", XNOR, 2, 4)
    bt = add("boot", 5)
    f = [add("func", 0, L["neg"]), add("func", 3, L["neg2"]), add("func", 1, L["per"]), add("func", 1, L["per2"])]
    if arb:
        f.append(add("func", 2, L["arb"]))
    lin = add("lin", [g_or, g_and, add("not", g_nor)], [1, -1, 1], 37)
    f.append(add("func", g_xor, L["neg3"]))
    if arb:
        f.append(add("func", g_nand, L["arb2"]))
    f_lin_per = add("func", lin, L["per"])
    f_lin_2 = add("func", lin, L["arb"] if arb else L["neg"])
    g_lin = add("gate", AND, lin, g_xnor)
    g_bt = add("gate", NOR, bt, add("not", f[0]))
    last = add("gate", XOR, f_lin_per, f_lin_2)
    outs = f + [lin, add("not", lin), f_lin_per, f_lin_2, g_lin, g_bt, last]
    return ops, outs, arb


_cases = {}


def func_case(name, B):
    if (name, B) not in _cases:
        e, _, _ = tc.context(name)
        ops, outs, arb = func_circuit(name)
        _, a_in, b_in = tc.encrypt_inputs(name, 6, B, 0xF0 + B)
        c = build(ops, outs)
        assert c.level_classes(1) == ((7, 3, 1, 1) if arb else (7, 3, 0, 1))     # all launch classes in one level
        assert c.level_classes(2)[:3] == ((2, 4, 3) if arb else (2, 5, 0))
        assert c.tables(*SETS[name], 1).shape[0] >= 3
        got = e.eval_circuit(c, a_in, b_in)
        want = node_by_node(e, ops, a_in, b_in)
        _cases[(name, B)] = (c, ops, outs, a_in, b_in, got, want)
    return _cases[(name, B)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(SETS))
def test_gpu_func_and_linear_levels_equal_node_by_node(name, B):
    c, ops, outs, a_in, b_in, (ao, bo), want = func_case(name, B)
    for j, o in enumerate(outs):
        wa, wb = want[o]
        assert np.array_equal(ao[j], wa) and np.array_equal(bo[j], wb), f"output {j} (node {o}: {ops[o][0]})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ginx", "lmkcdey"])
def test_gpu_chunked_classes_give_the_same_outputs(name):
    """set_max_slots(4) at B = 3: every class of 3 k slots is cut in mid-node (21 = 5 x 4 + 1, 9 = 2 x 4 + 1, ...)"""
    c, ops, outs, a_in, b_in, got, want = func_case(name, 3)
    e, _, _ = tc.context(name)
    c.set_max_slots(4)
    try:
        ao, bo = e.eval_circuit(c, a_in, b_in)
    finally:
        c.set_max_slots(0)
    assert np.array_equal(ao, got[0]) and np.array_equal(bo, got[1])


# ---- pinned kernels ----------------------------------------------------------------------------------------------
PINS = [("ginx", "FHE_HIP_GINX_KERNEL", "wave", "k_blind_rotate_ginx"),
        ("ginx", "FHE_HIP_GINX_KERNEL", "xsplit", "k_blind_rotate_ginx2x"),
        ("ginx", "FHE_HIP_GINX_KERNEL", "qsplit", "k_blind_rotate_ginx4x"),
        ("lmkcdey", "FHE_HIP_LMK_KERNEL", "wave", "k_blind_rotate_lmk"),
        ("lmkcdey", "FHE_HIP_LMK_KERNEL", "split", "k_blind_rotate_lmk3"),
        ("lmkcdey", "FHE_HIP_LMK_KERNEL", "qsplit", "k_blind_rotate_lmk4x")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,var,kind,kernel", PINS)
def test_gpu_pinned_kernels_select_the_slot_table(name, var, kind, kernel):
    """one level of 5 FUNC slots over 3 tables at B = 3 (15 launch slots) on each accumulator kernel == eval_func per
    node on the same context: a kernel that ignores the high half of the b word, or takes the table by instance
    instead of by node, differs"""
    ps, m = SETS[name]
    os.environ[var] = kind
    try:
        e = bf.GateEngine(ps, m, device=0)
    finally:
        del os.environ[var]
    try:
        seed = 0xF1AC0000 + ps
        sk = bf.keygen_secret(ps, m, seed)
        e.keygen_device(sk, seed)
        assert e.gate_kernel(15) == kernel
        q, B = e.params.q, 3
        L = make_luts(q)
        bits = np.random.default_rng(7).integers(0, 2, 3 * B)
        a, b = bf.encrypt(ps, m, sk, bits, 0xF2)
        a_in, b_in = a.reshape(3, B, -1), b.reshape(3, B)
        nodes = [(0, "neg"), (0, "neg2"), (1, "neg3"), (2, "neg"), (2, "neg2")]
        c = bf.Circuit()
        xs = [c.input() for _ in range(3)]
        for x, l in nodes:
            c.output(c.func(xs[x], L[l]))
        c.finalize()
        assert (c.num_levels, c.level_classes(1)) == (1, (0, 5, 0, 0)) and c.tables(ps, m, 1).shape[0] == 3
        ao, bo = e.eval_circuit(c, a_in, b_in)
        for j, (x, l) in enumerate(nodes):
            wa, wb = e.eval_func(a_in[x], b_in[x], q, L[l])
            assert np.array_equal(ao[j], wa) and np.array_equal(bo[j], wb), (j, l)
        assert not np.array_equal(bo[0], bo[1])
    finally:
        e.close()


# ---- refusals at evaluation --------------------------------------------------------------------------------------
def gate_circuit_still_right(name):
    e, _, _ = tc.context(name)
    _, a_in, b_in = tc.encrypt_inputs(name, 2, 2, 0xF3)
    c = bf.Circuit()
    x, y = c.input(), c.input()
    c.output(c.gate(NAND, x, y))
    c.finalize()
    ao, bo = e.eval_circuit(c, a_in, b_in)
    wa, wb = e.eval_gate(NAND, a_in[0], b_in[0], a_in[1], b_in[1])
    assert np.array_equal(ao[0], wa) and np.array_equal(bo[0], wb)


def refused(name, lut):
    e, _, _ = tc.context(name)
    _, a_in, b_in = tc.encrypt_inputs(name, 1, 2, 0xF4)
    c = bf.Circuit()
    c.output(c.func(c.input(), lut))
    c.finalize()
    with pytest.raises(FheHipError) as err:
        e.eval_circuit(c, a_in, b_in)
    return err.value


@pytest.mark.gpu
def test_gpu_refusals_at_evaluation_leave_the_context_usable():
    q = bf.params(*SETS["ginx"]).q
    gate_circuit_still_right("ginx")
    assert refused("ginx", make_luts(q // 2)["per"]).code == INVALID            # len != q
    gate_circuit_still_right("ginx")
    for name in ("lmkcdey", "ap"):                                               # the arbitrary class
        err = refused(name, make_luts(bf.params(*SETS[name]).q)["arb"])
        assert err.code == INVALID
        if name == "lmkcdey":
            assert "ciphertext modulus q needs to be <= ring dimension" in str(err)
        gate_circuit_still_right(name)


# ---- queued calls, descriptor and table cache --------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_queued_twice_and_a_second_circuit_replaces_the_tables():
    from fhe_amd._lib import check, lib, ptr, vp
    e, _, _ = tc.context("ginx")
    Lb = lib()
    q, n, B = e.params.q, e.params.n, 3
    L = make_luts(q)

    def circ(l1, l2):
        c = bf.Circuit()
        x, y = c.input(), c.input()
        s = c.linear([x, y], [1, -1], 11)
        c.output(c.func(s, L[l1]))
        c.output(c.func(x, L[l2]))
        return c.finalize()

    def want(l1, l2, a, b):
        sa = (a[0].astype(np.int64) - a[1].astype(np.int64)) % q
        sb = (b[0].astype(np.int64) - b[1].astype(np.int64) + 11) % q
        r1 = e.eval_func(sa.astype(np.uint64), sb.astype(np.uint64), q, L[l1])
        r2 = e.eval_func(a[0], b[0], q, L[l2])
        return np.stack([r1[0], r2[0]]), np.stack([r1[1], r2[1]])

    c1, c2 = circ("per", "arb"), circ("per2", "arb2")
    cases = [tc.encrypt_inputs("ginx", 2, B, s)[1:] for s in (0xF6, 0xF7)]
    wants = [want("per", "arb", a, b) for a, b in cases]
    ptrs = []

    def dev(nbytes, x=None):
        d = vp()
        check(Lb.fhe_hip_alloc(0, nbytes, ctypes.byref(d)))
        ptrs.append(d)
        if x is not None:
            check(Lb.fhe_hip_copy_to_device(d, ptr(np.ascontiguousarray(x)), nbytes))
        return d.value

    try:
        bufs = [(dev(a.nbytes, a), dev(b.nbytes, b), dev(2 * B * n * 8), dev(2 * B * 8)) for a, b in cases]
        for da, db, dao, dbo in bufs:   # both queued on the context's stream, no synchronisation in between
            e.eval_circuit_device(c1, B, da, db, dao, dbo)
        check(Lb.fhe_hip_synchronize(0))
        for (_, _, dao, dbo), (wa, wb) in zip(bufs, wants):
            ga, gb = np.zeros_like(wa), np.zeros_like(wb)
            check(Lb.fhe_hip_copy_to_host(ptr(ga), vp(dao), ga.nbytes))
            check(Lb.fhe_hip_copy_to_host(ptr(gb), vp(dbo), gb.nbytes))
            assert np.array_equal(ga, wa) and np.array_equal(gb, wb)
    finally:
        for d in ptrs:
            Lb.fhe_hip_free(d)
    # another circuit with other tables on the same context, then the first one again
    a, b = cases[0]
    w2 = want("per2", "arb2", a, b)
    g2 = e.eval_circuit(c2, a, b)
    assert np.array_equal(g2[0], w2[0]) and np.array_equal(g2[1], w2[1])
    g1 = e.eval_circuit(c1, a, b)
    assert np.array_equal(g1[0], wants[0][0]) and np.array_equal(g1[1], wants[0][1])
    assert not np.array_equal(g1[1], g2[1])
