"""Circuits with FUNC (EvalFunc) and LINEAR nodes: the host side -- classes, the expansion into physical bootstraps,
shared first stages, table dedup, launch classes and row numbering, the tables against a numpy restatement of the
reference's lambdas, refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest

from fhe_amd import binfhe as bf
from fhe_amd._lib import FheHipError

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INVALID, NOT_INIT = -2, -11
BETA = 128


def code(fn, *args, **kw):
    with pytest.raises(FheHipError) as e:
        fn(*args, **kw)
    return e.value.code


def luts_for(q, N):
    sys.path.insert(0, GOLD)
    from make_golden import fb_luts
    return fb_luts(q, q // 256, N)


def some_luts(q=1024):
    """a negacyclic, two periodic and two arbitrary LUTs over Z_q"""
    x = np.arange(q, dtype=np.uint64)
    neg = np.where(x < q // 2, q // 4, q - q // 4).astype(np.uint64)
    per1 = ((x % (q // 2)) // 128 * 128).astype(np.uint64)
    per2 = ((x % (q // 2)) // 64 * 64).astype(np.uint64)
    arb1 = (x * x * x % q).astype(np.uint64)         # x^2 would be periodic: (x + q/2)^2 = x^2 mod q
    arb2 = (x // 256 * 256).astype(np.uint64)
    return neg, per1, per2, arb1, arb2


def test_classes_are_decided_when_the_node_is_added():
    neg, per1, per2, arb1, arb2 = some_luts()
    c = bf.Circuit()
    x = c.input()
    ids = [c.func(x, l) for l in (neg, per1, per2, arb1, arb2)]
    assert [c.func_class(i) for i in ids] == [0, 1, 1, 2, 2]      # before finalize
    assert c.func_class(x) == -1 and c.func_class(c.not_(ids[0])) == -1
    assert code(c.func_class, 99) == INVALID


def test_stage1_sharing_levels_and_rows():
    """two periodic LUTs and one arbitrary LUT on one input: 2 first stages (one per class) and 3 second stages"""
    neg, per1, per2, arb1, arb2 = some_luts()
    c = bf.Circuit()
    x, y = c.input(), c.input()
    f1, f2, f3 = c.func(x, per1), c.func(x, per2), c.func(x, arb1)
    c.finalize()
    assert (c.num_levels, c.num_bootstraps) == (2, 5)
    assert c.level_classes(0) == (0, 0, 0, 0)
    assert c.level_classes(1) == (0, 1, 1, 0)        # the shared first stages: one at q, one at 2q
    assert c.level_classes(2) == (0, 2, 1, 0)
    assert [c.level(i) for i in range(3)] == [(2, 0), (2, 2), (3, 4)]
    # FUNC periodic / arbitrary = its second stage, at the operand's level + 2; class 1 rows before class 2
    assert [c.node_row(f) for f in (f1, f2, f3)] == [(4, False), (5, False), (6, False)]
    # tables: class 1 holds TV_HALF + two LUT tables, class 2 TV_HALF + one
    assert c.tables(bf.STD128, bf.GINX, 1).shape == (3, 1024)
    assert c.tables(bf.STD128, bf.GINX, 2).shape == (2, 2048)

    # a different operand does not share; a negacyclic FUNC is one bootstrap at the operand's level + 1
    c = bf.Circuit()
    x, y = c.input(), c.input()
    g = c.gate(bf.AND, x, y)
    fa, fb, fn = c.func(x, per1), c.func(y, per1), c.func(g, neg)
    c.finalize()
    assert c.num_bootstraps == 1 + 4 + 1
    assert c.level_classes(1) == (1, 2, 0, 0) and c.level_classes(2) == (0, 3, 0, 0)
    assert c.node_row(fn)[0] >= c.level(2)[1]        # level(g) + 1
    assert c.tables(bf.STD128, bf.GINX, 1).shape[0] == 3   # TV_HALF, per1 (once), neg


def test_table_dedup():
    neg, per1, per2, arb1, arb2 = some_luts()
    c = bf.Circuit()
    xs = [c.input() for _ in range(3)]
    for x in xs:
        c.func(x, per1), c.func(x, arb1), c.func(x, neg)
    c.func(xs[0], per1.copy())                       # the same LUT again on the same operand: another slot, no new table
    c.finalize()
    t1, t2 = c.tables(bf.STD128, bf.GINX, 1), c.tables(bf.STD128, bf.GINX, 2)
    assert t1.shape[0] == 3 and t2.shape[0] == 2
    assert len({r.tobytes() for r in t1}) == 3 and len({r.tobytes() for r in t2}) == 2
    assert c.level_classes(1) == (0, 6, 3, 0) and c.level_classes(2) == (0, 4, 3, 0)


def test_linear_levels_and_rows_contiguous_per_class():
    neg, per1, per2, arb1, arb2 = some_luts()
    c = bf.Circuit()
    a, b, x = c.input(), c.input(), c.input()
    l0 = c.linear([a, b], [1, -1], 5)                # level 0
    g = c.gate(bf.XOR, a, b)                         # level 1, class 0
    fn = c.func(l0, neg)                             # level 1, class 1
    fa = c.func(x, arb1)                             # levels 1, 2, class 2
    bt = c.bootstrap(x)                              # level 1, class 0
    l1 = c.linear([g, c.not_(fn), a], None, 0)       # level 1: the highest operand level
    fp = c.func(l1, per1)                            # levels 2, 3
    g2 = c.gate(bf.AND, l1, fa)                      # level 3
    for o in (l0, l1, fp, g2, c.not_(l1)):
        c.output(o)
    c.finalize()
    assert (c.num_levels, c.num_bootstraps) == (3, 2 + 1 + 2 + 2 + 1)
    assert c.level_classes(0) == (0, 0, 0, 1)
    assert c.level_classes(1) == (2, 1, 1, 1)
    assert c.level_classes(2) == (0, 1, 1, 0)
    assert c.level_classes(3) == (1, 1, 0, 0)
    assert [c.level(i) for i in range(4)] == [(4, 0), (5, 4), (2, 9), (2, 11)]
    assert c.node_row(l0) == (3, False)              # after the inputs
    assert c.node_row(g) == (4, False) and c.node_row(bt) == (5, False)    # class 0 first
    assert c.node_row(fn) == (6, False)                                    # class 1
    assert c.node_row(l1) == (8, False)                                    # row 7: fa's first stage; LINEAR last
    assert c.node_row(fa) == (10, False) and c.node_row(fp) == (12, False) and c.node_row(g2) == (11, False)
    total = 0
    for i in range(4):
        w, first = c.level(i)
        assert first == total and w == sum(c.level_classes(i)) + (3 if i == 0 else 0)
        total += w
    assert code(c.level_classes, 4) == INVALID


def restated_tables(q, Q, luts):
    """numpy restatement of EvalFunc's lambdas (binfhe-base-scheme.cpp:254-256, 285-290, 302-307, 324-329), times
    Q / fmod: name -> (class, [tables the FUNC node needs, in the order the plan creates them])"""
    out = {}
    for name, lut in luts.items():
        lut = lut.astype(np.int64)
        mid = q // 2
        if np.array_equal(lut[:mid], q - lut[mid:]):                                 # checkInputFunction: negacyclic
            out[name] = (1, [(Q // q) * lut])                                        # fLUT
            continue
        periodic = np.array_equal(lut[:mid], lut[mid:])
        cm = q if periodic else 2 * q                                                # the lambdas' (q, Q) = (cm, cm)
        x = np.arange(cm, dtype=np.int64)
        half = np.where(x < cm // 2, cm - cm // 4, cm // 4)                          # f0
        lut2 = lut if periodic else np.concatenate([lut, lut])                       # LUT2 = LUT || LUT
        anti = np.where(x < cm // 2, lut2[x % len(lut2)], cm - lut2[(x - cm // 2) % len(lut2)])   # fLUT1 / fLUT2
        out[name] = (1 if periodic else 2, [(Q // cm) * half, (Q // cm) * anti])
    return out


@pytest.mark.parametrize("ps,m", [(bf.STD128, bf.GINX), (bf.STD128_LMKCDEY, bf.LMKCDEY)])
def test_tables_equal_the_restated_lambdas(ps, m):
    P = bf.params(ps, m)
    luts = luts_for(P.q, P.N)
    assert ("cube" in luts) == (P.q <= P.N)
    want = restated_tables(P.q, P.Q, luts)
    for name, lut in luts.items():
        c = bf.Circuit()
        f = c.func(c.input(), lut)
        c.finalize()
        cls, tabs = want[name]
        assert c.func_class(f) == {"neg": 0, "per": 1, "cube": 2}[name]
        got = c.tables(ps, m, cls)
        assert got.shape == (len(tabs), P.q * (2 if cls == 2 else 1))
        for g, w in zip(got, tabs):
            assert np.array_equal(g.astype(np.int64), w), name
        assert c.tables(ps, m, 3 - cls).shape[0] == 0


def test_refusals_consume_no_id():
    neg, per1, per2, arb1, arb2 = some_luts()
    c = bf.Circuit()
    x, y = c.input(), c.input()
    nx = c.not_(x)
    lin = c.linear([x, y])
    assert lin == 3
    bad_len = np.zeros(12, np.uint64)
    assert code(c.func, x, bad_len) == INVALID                         # not a power of two
    assert code(c.func, x, np.zeros(2, np.uint64)) == INVALID          # below 4
    big = per1.copy()
    big[7] = 1024
    assert code(c.func, x, big) == INVALID                             # a value >= len
    assert code(c.func, nx, per1) == INVALID                           # a negated operand
    assert code(c.func, c.not_(c.not_(nx)), arb1) == INVALID           # ... through a NOT chain (ids 4, 5 are used)
    assert code(c.func, 99, per1) == INVALID                           # an unknown id
    assert code(c.linear, [lin, x]) == INVALID                         # LINEAR of LINEAR
    assert code(c.linear, [c.not_(lin)]) == INVALID                    # ... through a NOT (id 6)
    assert code(c.linear, []) == INVALID                               # k = 0
    assert code(c.linear, [x, y, x, y, x]) == INVALID                  # k = 5
    assert code(c.linear, [x, 99]) == INVALID
    assert c.func(c.not_(nx), per1) == 8                               # NOT NOT x is x; refused adds took no id
    assert c.linear([x, nx, y, x], [1, -1, -1, 1], 3) == 9
    c.finalize()
    assert c.num_bootstraps == 2
    assert code(c.func, x, per1) == INVALID and code(c.linear, [x]) == INVALID   # any add after finalize
    # len != q is a refusal against a parameter set
    c2 = bf.Circuit()
    c2.func(c2.input(), np.arange(512, dtype=np.uint64) // 2)
    c2.finalize()
    assert code(c2.tables, bf.STD128, bf.GINX, 1) == INVALID
    # the arbitrary class: q > N (STD128_LMKCDEY: q = 2N) and AP
    P = bf.params(bf.STD128_LMKCDEY, bf.LMKCDEY)
    c3 = bf.Circuit()
    c3.func(c3.input(), (np.arange(P.q, dtype=np.uint64) ** 3) % P.q)
    c3.finalize()
    with pytest.raises(FheHipError, match="ciphertext modulus q needs to be <= ring dimension"):
        c3.tables(bf.STD128_LMKCDEY, bf.LMKCDEY, 2)
    Pa = bf.params(bf.STD128_AP, bf.AP)
    c4 = bf.Circuit()
    c4.func(c4.input(), (np.arange(Pa.q, dtype=np.uint64) ** 3) % Pa.q)
    c4.finalize()
    assert code(c4.tables, bf.STD128_AP, bf.AP, 2) == INVALID
    assert code(c4.tables, bf.STD128_AP, bf.AP, 0) == INVALID          # no such class


def test_old_circuits_plan_is_unchanged():
    """only the old node kinds: counts, levels and rows as before, every slot in the gate class"""
    c = bf.Circuit()
    a, b, x = c.input(), c.input(), c.input()
    g1 = c.gate(bf.AND, a, b)
    n1 = c.not_(g1)
    g2 = c.gate(bf.XOR, c.not_(n1), x)
    g3 = c.gate(bf.OR, g2, n1)
    bt = c.bootstrap(x)
    mx = c.cmux(a, b, x)
    g4 = c.gate(bf.NAND, g3, g1)
    g5 = c.gate(bf.XNOR, mx, bt)
    c.finalize()
    assert (c.num_inputs, c.num_levels, c.num_bootstraps) == (3, 4, 9)
    assert [c.level(i) for i in range(5)] == [(3, 0), (4, 3), (2, 7), (2, 9), (1, 11)]
    assert [c.node_row(v) for v in (g1, n1, bt, g2, mx, g3, g5, g4)] == \
        [(3, False), (3, True), (4, False), (7, False), (8, False), (9, False), (10, False), (11, False)]
    assert [c.level_classes(i) for i in range(5)] == [(0, 0, 0, 0), (4, 0, 0, 0), (2, 0, 0, 0), (2, 0, 0, 0), (1, 0, 0, 0)]
    assert c.tables(bf.STD128, bf.GINX, 1).shape[0] == 0 and c.tables(bf.STD128, bf.GINX, 2).shape[0] == 0
