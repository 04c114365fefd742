"""Circuits (include/fhe_hip.h, "boolean circuits"): the host side -- DAG, level plan, error codes, the gate
fold that lets one launch serve a level of mixed gate types, and the Python object model.  No GPU."""
import ctypes

import numpy as np
import pytest

from fhe_amd import binfhe as bf
from fhe_amd._lib import FheHipError

INVALID, NOT_INIT = -2, -11
TWO_INPUT = (bf.OR, bf.AND, bf.NOR, bf.NAND, bf.XOR, bf.XNOR, bf.XOR_FAST, bf.XNOR_FAST)


def code(fn, *args):
    with pytest.raises(FheHipError) as e:
        fn(*args)
    return e.value.code


def dag12():
    """12 nodes: fan-out (g1 feeds g2, g3, g4), g1 (level 1) consumed three levels later by g4 (level 4), a NOT
    chain (n2 = NOT NOT g1 is g1), a CMUX, a BOOTSTRAP"""
    c = bf.Circuit()
    a, b, x = c.input(), c.input(), c.input()
    g1 = c.gate(bf.AND, a, b)        # level 1
    n1 = c.not_(g1)
    n2 = c.not_(n1)
    g2 = c.gate(bf.XOR, n2, x)       # level 2
    g3 = c.gate(bf.OR, g2, n1)       # level 3
    bt = c.bootstrap(x)              # level 1
    mx = c.cmux(a, b, x)             # NANDs at level 1, 1, 2
    g4 = c.gate(bf.NAND, g3, g1)     # level 4
    g5 = c.gate(bf.XNOR, mx, bt)     # level 3
    assert [a, b, x, g1, n1, n2, g2, g3, bt, mx, g4, g5] == list(range(12))
    return c, dict(a=a, b=b, x=x, g1=g1, n1=n1, n2=n2, g2=g2, g3=g3, bt=bt, mx=mx, g4=g4, g5=g5)


def test_plan_levels_widths_and_contiguous_rows():
    c, n = dag12()
    for k in ("n1", "g4", "a", "g5"):
        c.output(n[k])
    assert code(lambda: c.num_levels) == NOT_INIT       # a plan query before finalize
    c.finalize()
    assert (c.num_inputs, c.num_outputs, c.num_levels, c.num_bootstraps) == (3, 4, 4, 9)
    # level 1: g1, bt, CMUX's two first NANDs; 2: g2, CMUX's last NAND; 3: g3, g5; 4: g4
    assert [c.level(i)[0] for i in range(5)] == [3, 4, 2, 2, 1]
    # every level's rows are one block, the blocks in level order, inputs first
    row = 0
    for i in range(5):
        w, first = c.level(i)
        assert first == row
        row += w
    assert row == 3 + 9
    assert code(c.level, 5) == INVALID
    rows = {k: c.node_row(v) for k, v in n.items()}
    assert [rows[k] for k in "abx"] == [(0, False), (1, False), (2, False)]
    assert rows["g1"] == (3, False) and rows["n1"] == (3, True) and rows["n2"] == (3, False)   # NOT NOT x is x
    assert rows["bt"] == (4, False)
    assert rows["g2"] == (7, False) and rows["mx"] == (8, False)        # CMUX = its last NAND, level 2
    assert sorted(r for r, _ in (rows["g3"], rows["g5"])) == [9, 10] and rows["g4"] == (11, False)
    # rows 5 and 6 (level 1) belong to no user node: CMUX's NAND(c0, NOT sel) and NAND(c1, sel)
    assert {5, 6}.isdisjoint(r for r, _ in rows.values())
    in_level = lambda r, i: c.level(i)[1] <= r < c.level(i)[1] + c.level(i)[0]   # noqa: E731
    assert in_level(rows["g1"][0], 1) and in_level(rows["g3"][0], 3) and in_level(rows["g4"][0], 4)


def test_cmux_is_three_nands_on_two_levels():
    c = bf.Circuit()
    c0, c1, s = c.input(), c.input(), c.input()
    c.output(c.cmux(c0, c1, s))
    c.finalize()
    assert (c.num_levels, c.num_bootstraps) == (2, 3)
    assert [c.level(i)[0] for i in (1, 2)] == [2, 1]


def test_errors_have_their_documented_codes():
    c = bf.Circuit()
    x, y = c.input(), c.input()
    assert code(c.gate, bf.AND, x, 7) == INVALID              # unknown id
    assert code(c.not_, 2) == INVALID
    assert code(c.output, 9) == INVALID
    assert code(c.gate, bf.AND, x, x) == INVALID              # ct1 == ct2
    nx = c.not_(x)
    assert code(c.gate, bf.XOR, nx, c.not_(c.not_(nx))) == INVALID   # the same (node, negation) through aliases
    g = c.gate(bf.AND, x, nx)                                 # AND(x, NOT x): two different ciphertexts
    assert code(c.cmux, x, y, nx) == INVALID                  # its NAND(c0, NOT sel) would be NAND(x, x)
    for multi in (bf.MAJORITY, bf.AND3, bf.OR3, bf.AND4, bf.OR4, bf.CMUX, 99, -1):
        assert code(c.gate, multi, x, y) == INVALID
    c.output(g)
    L = bf.L()
    out = np.zeros((1, 1, 8), np.uint64)
    # evaluation before finalize: the circuit is checked before the context, so no device is needed
    assert L.fhe_hip_eval_circuit_batch(None, c._h, 1, 2, None, None, 1, None, None) == NOT_INIT
    assert L.fhe_hip_eval_circuit_batch_device(None, c._h, 1, 2, None, None, 1, None, None, None) == NOT_INIT
    c.finalize()
    assert (c.num_levels, c.num_bootstraps) == (1, 1)         # the refused nodes left nothing behind
    for add in (c.input, lambda: c.not_(x), lambda: c.gate(bf.OR, x, y), lambda: c.cmux(x, y, g),
                lambda: c.bootstrap(x), lambda: c.output(x), c.finalize):
        assert code(add) == INVALID                           # add after finalize
    assert L.fhe_hip_eval_circuit_batch(None, c._h, 1, 3, None, None, 1, None, None) == INVALID   # 2 inputs, not 3
    assert L.fhe_hip_eval_circuit_batch(None, c._h, 1, 2, None, None, 2, None, None) == INVALID   # 1 output, not 2
    assert L.fhe_hip_eval_circuit_batch_device(None, c._h, 1, 1, None, None, 1, None, None, None) == INVALID
    assert L.fhe_hip_eval_circuit_batch(None, c._h, 1, 2, None, None, 1, out.ctypes.data, None) == -1   # no context
    assert L.fhe_hip_eval_circuit_batch(None, None, 1, 2, None, None, 1, None, None) == -1


def table_rows():
    return [(ps, m) for ps in range(len(bf.PARAMSETS)) for m in (bf.AP, bf.GINX, bf.LMKCDEY)
            if bf.method_compatible(ps, m)]


def window(q, q1):
    """BootstrapGateCore's window (binfhe-base-scheme.cpp:535-553) as arrays over x in [0, q): True where the
    test vector takes lv; and whether lv is Q2p (swap) or Q2pNeg"""
    q2 = (q1 + q // 2) % q
    swap = q1 >= q2
    lb, ub = (q2, q1) if swap else (q1, q2)
    x = np.arange(q)
    return (x >= lb) & (x < ub), swap


def tv_signs(q, q1, b):
    """sign pattern of m[i], i = 0, factor, 2 factor, .. (:564-567): +1 where the value is Q2p, -1 where Q2pNeg,
    for every b of the array `b` -> [len(b)][q/2]"""
    inside, swap = window(q, q1)
    bx = (b[:, None] - np.arange(q // 2)[None, :]) % q       # b.ModSubFastEq(1, q) per step
    takes_lv = inside[bx]
    return np.where(takes_lv == swap, 1, -1).astype(np.int8)    # lv = swap ? Q2p : Q2pNeg; uv the other


def test_gate_fold_constants_for_every_parameter_row():
    k = {bf.OR: 5, bf.AND: 7, bf.NOR: 1, bf.NAND: 3, bf.XOR: 6, bf.XNOR: 2, bf.XOR_FAST: 6, bf.XNOR_FAST: 2}
    seen = set()
    for ps, m in table_rows():
        q = bf.params(ps, m).q
        seen.add(q)
        for g in TWO_INPUT:
            q1, dbl, bshift = bf.gate_fold(ps, m, g, bf.AND)
            assert q1 == k[g] * (q // 8)                                  # params.cpp gate_const
            assert dbl == (g in (bf.XOR, bf.XNOR, bf.XOR_FAST, bf.XNOR_FAST))
            assert bshift == (7 * (q // 8) - q1) % q
    assert seen >= {512, 1024, 2048, 4096}
    for bad in (bf.MAJORITY, bf.AND3, bf.OR3, bf.AND4, bf.OR4, bf.CMUX):
        assert code(bf.gate_fold, bf.STD128, bf.GINX, bad, bf.AND) == INVALID
        assert code(bf.gate_fold, bf.STD128, bf.GINX, bf.AND, bad) == INVALID


@pytest.mark.parametrize("ps,m", [(bf.TOY, bf.GINX), (bf.STD128, bf.GINX), (bf.STD128_LMKCDEY, bf.LMKCDEY),
                                  (17, bf.GINX)])   # q = 512, 1024, 2048, 4096: every q of the table
def test_gate_fold_builds_the_same_test_vector(ps, m):
    """gate G with its own window at b and the level's reference gate R = AND with its window at b + bshift give
    the same test vector, for every b in [0, q) (and every pair (G, R), not only R = AND)"""
    q = bf.params(ps, m).q
    assert q == {bf.TOY: 512, bf.STD128: 1024, bf.STD128_LMKCDEY: 2048, 17: 4096}[ps]
    b = np.arange(q)
    for R in TWO_INPUT if q <= 1024 else (bf.AND,):
        ref = {}
        for G in TWO_INPUT:
            q1, _, bshift = bf.gate_fold(ps, m, G, R)
            if bshift not in ref:
                ref[bshift] = tv_signs(q, bf.gate_fold(ps, m, R, R)[0], (b + bshift) % q)
            own = tv_signs(q, q1, b)
            assert np.array_equal(own, ref[bshift]), (G, R)
    # and the windows differ: without the shift AND's vector is not OR's
    assert not np.array_equal(tv_signs(q, 5 * (q // 8), b), tv_signs(q, 7 * (q // 8), b))



def test_batchdag_object_model():
    cc = bf.BinFHEContext()
    cc.paramset, cc.method = bf.STD128, bf.GINX
    cc.params = bf.params(bf.STD128, bf.GINX)          # the parameters only: no device context
    n, q = cc.params.n, cc.params.q
    ct = lambda v: bf.LWECiphertext(np.full(n, v, np.uint64), v, q)   # noqa: E731
    dag = bf.BatchDAG(cc)
    i0, i1, i2 = dag.AddCiphertext(ct(1)), dag.AddCiphertext(ct(2)), dag.AddCiphertext(ct(3))
    g = dag.AddBinGate(bf.XOR, i0, i1)
    m = dag.AddCMUX(i0, i1, i2)
    r = dag.AddBootstrap(g)
    assert [i0, i1, i2, g, m, r] == list(range(6))     # ids number the ciphertexts, as the reference's do
    with pytest.raises(NotImplementedError, match="not built"):
        dag.AddEvalFunc(i0, np.zeros(q, np.uint64))
    with pytest.raises(FheHipError):
        dag.AddBinGate(bf.AND, i0, i0)
    with pytest.raises(FheHipError):
        dag.AddBinGate(bf.AND3, i0, i1)
    with pytest.raises(FheHipError):
        dag.AddCiphertext(bf.LWECiphertext(np.zeros(cc.params.N, np.uint64), 0, cc.params.Q))   # mod Q
    with pytest.raises(FheHipError):
        dag.GetResult(g)                               # before Execute
    with pytest.raises(IndexError):
        dag.GetResult(6)
    assert dag.AddBinGate(bf.AND, g, m) == 6           # the refused adds consumed no id
    dag.Clear()
    assert dag.AddCiphertext(ct(1)) == 0               # Clear starts a new DAG


def test_circuit_object_model():
    c = bf.Circuit()
    x, y = c.input(), c.input()
    assert c.output(c.gate(bf.NOR, x, c.not_(y))) == 3
    assert (c.num_inputs, c.num_outputs, c.finalized) == (2, 1, False)
    assert c.finalize() is c and c.finalized
    c.set_max_slots(4)
    assert c.node_row(2) == (1, True)
    c.close()
    c.close()
