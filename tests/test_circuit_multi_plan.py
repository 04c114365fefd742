"""Multi-input gates (MAJORITY, AND3 / OR3, AND4 / OR4) as circuit nodes: the host side -- the gate windows and the
fold that moves them onto AND's, the level plan with one more gate class per plaintext modulus, the refusals.
No GPU."""
import numpy as np
import pytest

from fhe_amd import binfhe as bf
from fhe_amd._lib import FheHipError

INVALID, NOT_INIT = -2, -11
MULTI = (bf.MAJORITY, bf.AND3, bf.OR3, bf.AND4, bf.OR4)
# q = 512, 1024, 2048, 4096: every q of the parameter table
ROWS = [(bf.TOY, bf.GINX, 512), (bf.STD128, bf.GINX, 1024), (bf.STD128_LMKCDEY, bf.LMKCDEY, 2048), (17, bf.GINX, 4096)]


def code(fn, *args):
    with pytest.raises(FheHipError) as e:
        fn(*args)
    return e.value.code


def q1_of(gate, q):
    """GetGateConst for the multi-input gates (rgsw-cryptoparameters.cpp:78-92)"""
    return {bf.MAJORITY: 7 * (q >> 3), bf.AND3: 11 * (q // 12), bf.OR3: 7 * (q // 12), bf.AND4: 15 * (q >> 4),
            bf.OR4: 9 * (q >> 4)}[gate]


@pytest.mark.parametrize("ps,m,q", ROWS)
def test_gate_windows_against_bootstrap_gate_core(ps, m, q):
    """binfhe-base-scheme.cpp:535-556 restated: q1 = GetGateConst, Q2p = Q / (2p) + 1; :162 adds Q2p to b"""
    P = bf.params(ps, m)
    assert P.q == q
    for p in (4, 6, 8):
        for g in MULTI:
            q1, value, b_const, bshift = bf.gate_window(ps, m, g, p)
            assert q1 == q1_of(g, q)
            assert value == b_const == P.Q // (2 * p) + 1
            assert bshift == (7 * (q >> 3) - q1) % q
        # a 2-input gate's b is Q/8 + 1 whatever p (:118)
        assert bf.gate_window(ps, m, bf.XOR, p) == (6 * (q >> 3), P.Q // (2 * p) + 1, (P.Q >> 3) + 1, q >> 3)
    # why MAJORITY at p = 4 rides in class 0
    assert bf.gate_window(ps, m, bf.MAJORITY, 4) == bf.gate_window(ps, m, bf.AND, 4)
    assert bf.gate_window(ps, m, bf.AND3, 6) != bf.gate_window(ps, m, bf.AND, 6)
    for bad in ((bf.CMUX, 4), (99, 4), (bf.MAJORITY, 1), (bf.MAJORITY, 0), (bf.AND3, q // 2 + 1)):
        assert code(bf.gate_window, ps, m, *bad) == INVALID
    assert bf.gate_window(ps, m, bf.AND3, q // 2)[1] == P.Q // q + 1      # 2p = q is the last one accepted


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


@pytest.mark.parametrize("ps,m,q", ROWS)
def test_fold_onto_ands_window_builds_the_same_test_vector(ps, m, q):
    """gate G with its own window at b and AND's window at b + bshift_to_and give the same sign pattern for every b
    in [0, q): the windows are half circles, also where q1 is no multiple of q/8 (AND3, OR3)"""
    b = np.arange(q)
    q1_and = bf.gate_window(ps, m, bf.AND, 4)[0]
    assert q1_and == 7 * (q >> 3)
    for G in MULTI:
        q1, _, _, bshift = bf.gate_window(ps, m, G, 4)
        assert np.array_equal(tv_signs(q, q1, b), tv_signs(q, q1_and, (b + bshift) % q)), G
    # and the shift matters: AND3's pattern is not AND's
    assert not np.array_equal(tv_signs(q, q1_of(bf.AND3, q), b), tv_signs(q, q1_and, b))


PERIODIC = [1, 2, 3, 0, 1, 2, 3, 0]


def mixed_level(multi):
    """level 1: AND, XOR, a periodic FUNC's first stage and a LINEAR of the AND -- and, with multi, MAJORITY p=4,
    AND3 p=6, OR3 p=6, AND4 p=8 added in an order that is not the row order; level 2: the FUNC's second stage"""
    c = bf.Circuit()
    i = [c.input() for _ in range(4)]
    n = {}
    if multi:
        n["and4"] = c.gate_multi(bf.AND4, i, 8)
        n["or3"] = c.gate_multi(bf.OR3, i[1:], 6)
    n["and"] = c.gate(bf.AND, i[0], i[1])
    if multi:
        n["maj"] = c.gate_multi(bf.MAJORITY, i[:3], 4)
    n["func"] = c.func(i[2], PERIODIC)
    n["xor"] = c.gate(bf.XOR, i[2], c.not_(i[3]))
    if multi:
        n["and3"] = c.gate_multi(bf.AND3, [i[0], c.not_(i[1]), i[3]], 6)
    n["lin"] = c.linear([n["and"], i[0]], [1, -1], 5)
    for v in n.values():
        c.output(v)
    return c.finalize(), n


def test_plan_orders_a_level_by_class_then_modulus():
    c, n = mixed_level(True)
    assert c.func_class(n["func"]) == 1
    assert (c.num_levels, c.num_bootstraps) == (2, 8)
    assert c.level_classes(1) == (3, 1, 0, 1)
    assert c.level_gate_classes(1) == [(6, 2), (8, 1)]
    assert c.level_classes(2) == (0, 1, 0, 0) and c.level_gate_classes(2) == []
    assert c.level_gate_classes(0) == [] and code(c.level_gate_classes, 3) == INVALID
    assert [c.level(i) for i in range(3)] == [(4, 0), (8, 4), (1, 12)]
    for lvl in range(3):
        assert c.level(lvl)[0] == sum(c.level_classes(lvl)) + sum(w for _, w in c.level_gate_classes(lvl)) + (4 if lvl == 0 else 0)
    row = {k: c.node_row(v)[0] for k, v in n.items()}
    # class 0 in node order (AND, MAJORITY, XOR), the FUNC's first stage at row 7, p = 6 in node order, p = 8, LINEAR
    assert (row["and"], row["maj"], row["xor"]) == (4, 5, 6)
    assert (row["or3"], row["and3"], row["and4"], row["lin"]) == (8, 9, 10, 11)
    assert row["func"] == 12


def test_plan_without_multi_nodes_is_the_parents():
    """the same circuit without its multi-input nodes: the numbers the parent commit's build gives"""
    c, n = mixed_level(False)
    assert (c.num_levels, c.num_bootstraps) == (2, 4)
    assert [c.level(i) for i in range(3)] == [(4, 0), (4, 4), (1, 8)]
    assert [c.level_classes(i) for i in range(3)] == [(0, 0, 0, 0), (2, 1, 0, 1), (0, 1, 0, 0)]
    assert {k: c.node_row(v) for k, v in n.items()} == {"and": (4, False), "func": (8, False), "xor": (5, False),
                                                        "lin": (7, False)}
    assert all(c.level_gate_classes(i) == [] for i in range(3))


def test_operands_of_any_kind_and_levels():
    c = bf.Circuit()
    x, y, z = c.input(), c.input(), c.input()
    g = c.gate(bf.AND, x, y)                          # level 1
    mx = c.cmux(x, y, z)                              # level 2
    bt = c.bootstrap(z)                               # level 1
    fn = c.func(x, [1, 2, 3, 4, 7, 6, 5, 4])          # negacyclic: level 1
    ln = c.linear([g, x])                             # level 1, no bootstrap
    m1 = c.gate_multi(bf.MAJORITY, [g, c.not_(bt), ln], 4)     # level 2
    m2 = c.gate_multi(bf.OR4, [m1, mx, fn, x], 8)               # level 3
    m3 = c.gate_multi(bf.MAJORITY, [x, c.not_(x), y], 4)        # three different ciphertexts: level 1
    m4 = c.gate_multi(bf.AND3, [x, y], 6)                       # k = 2
    c.output(m2)
    c.finalize()
    assert c.func_class(fn) == 0
    assert c.num_levels == 3
    lv = lambda v: next(i for i in range(4) if c.level(i)[1] <= c.node_row(v)[0] < sum(c.level(i)))   # noqa: E731
    assert [lv(v) for v in (g, mx, bt, fn, ln, m1, m2, m3, m4)] == [1, 2, 1, 1, 1, 2, 3, 1, 1]
    assert c.level_gate_classes(1) == [(6, 1)] and c.level_gate_classes(3) == [(8, 1)]
    assert c.level_classes(2)[0] == 2                 # CMUX's last NAND and m1


def test_refusals():
    c = bf.Circuit()
    x, y, z, w = (c.input() for _ in range(4))
    nx = c.not_(x)
    bad = [
        (bf.AND, [x, y, z], 4), (bf.XOR, [x, y], 4), (bf.CMUX, [x, y, z], 4), (99, [x, y, z], 4), (-1, [x, y, z], 4),
        (bf.MAJORITY, [x], 4), (bf.MAJORITY, [], 4), (bf.AND4, [x, y, z, w, nx], 8),       # k out of range
        (bf.MAJORITY, [x, y, 77], 4),                                                       # unknown id
        (bf.MAJORITY, [x, y, z], 1), (bf.MAJORITY, [x, y, z], 0),                           # ptmod < 2
        (bf.MAJORITY, [x, y, x], 4), (bf.AND4, [x, y, z, y], 8),                            # the same ciphertext twice
        (bf.OR3, [nx, y, c.not_(c.not_(nx))], 6),                                           # .. through aliases
    ]
    before = c.not_(y)
    for g, xs, p in bad:
        assert code(c.gate_multi, g, xs, p) == INVALID, (g, xs, p)
    assert c.not_(y) == before + 1                                    # a refused add consumes no id
    m = c.gate_multi(bf.MAJORITY, [x, nx, y], 4)                      # x, NOT x, y: three different ciphertexts
    assert m == before + 2
    for g in MULTI:
        assert code(c.gate, g, x, y) == INVALID                       # add_gate keeps refusing the five codes
    c.output(m)
    assert code(c.level_gate_classes, 1) == NOT_INIT
    c.finalize()
    assert (c.num_levels, c.num_bootstraps) == (1, 1)                 # the refused nodes left nothing behind
    assert code(c.gate_multi, bf.MAJORITY, [x, y, z], 4) == INVALID   # add after finalize


def test_plaintext_modulus_against_the_parameter_set():
    """2p > q is known only against a parameter set: add accepts it, Circuit::check_params -- the first thing an
    evaluation does, and what the table query runs -- refuses it.  Neither needs a context."""
    c = bf.Circuit()
    x, y, z = c.input(), c.input(), c.input()
    c.output(c.gate_multi(bf.AND3, [x, y, z], 512))
    c.finalize()
    assert c.tables(bf.STD128, bf.GINX, 1).shape == (0, 1024)         # q = 1024: 2p = q is accepted
    assert code(c.tables, bf.TOY, bf.GINX, 1) == INVALID              # q = 512
    L = bf.L()
    out = np.zeros((1, 1, 8), np.uint64)
    # the circuit is checked before the context, as for every circuit
    assert L.fhe_hip_eval_circuit_batch(None, c._h, 1, 2, None, None, 1, None, None) == INVALID   # 3 inputs, not 2
    assert L.fhe_hip_eval_circuit_batch(None, c._h, 1, 3, None, None, 1, out.ctypes.data, None) == -1   # no context
