"""K1 GINX (Q < 2^27) and the LMKCDEY / AP op-list kernel take middle stage pairs of their loop transforms as 4-point
groups with product twiddles
(boot_arith.h ct_group4_s / gs_group4_s, nt.h stage_group_table through the C ABI, red_plan.h red_plan_group_ok).

CPU: a numpy model of each grouped pair in the kernel's own arithmetic (32-bit words, signed Montgomery products,
64-bit two-term chains) against two exact radix-2 stages mod Q, for both K1 moduli and every pair position, with the
output bounds the later stages rely on; the product tables of the builder against products of the power table, and
the tables it refuses; the bound chain of the forward pass in exact fractions; the group-aware replay of the
half-wave reduction plan (tests/red_plan_groups_check.cpp, host compiler).  GPU: the one-wave kernels pinned by
FHE_HIP_GINX_KERNEL / FHE_HIP_LMK_KERNEL = wave against the oracle restatement on the gates whose b windows and
doubled inputs test_k1_fwd_group.py does not run, and one gate through the op-list kernel's AP/DM instantiation."""
import ctypes
import itertools
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (paramset, method): STD128 GINX (Q = 134215681 < 2^27: FM 1), STD128_LMKCDEY (Q = 268369921 < 2^28: FM 2) and
# STD128_AP (AP / DM)
SETS = {"std128": (3, 2), "lmkcdey": (21, 3), "ap": (2, 1)}
MODULI = {"std128": 134215681, "lmkcdey": 268369921}
N = 1024


# ---- the kernel's arithmetic on int64 arrays holding 32-bit two's-complement words (as test_k1_fwd_group.py) ------
def wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def smont_red(t, Q):
    """boot_arith.h smont_red: t (int64) 2^-32 mod Q"""
    qinvp = pow(Q, -1, 1 << 32)
    lo = (t.astype(np.uint64) & np.uint64(0xFFFFFFFF)) * np.uint64(qinvp) & np.uint64(0xFFFFFFFF)
    mm = wrap32(lo.astype(np.int64))
    r = t - mm * np.int64(Q)
    assert not np.any(r & 0xFFFFFFFF)
    return r >> 32


def smont_mul(a, bR, Q):
    return smont_red(np.asarray(a, np.int64) * np.int64(bR), Q)


def smont_mul2(x, wR, y, zR, Q):
    """one unreduced 64-bit chain x w + y z (|.| < 2^31 2^28 2 < 2^63), one reduction"""
    return smont_red(np.asarray(x, np.int64) * np.int64(wR) + np.asarray(y, np.int64) * np.int64(zR), Q)


def mont(x, Q):
    return (x << 32) % Q


def ct_group4_model(a, b, c, d, w1, w2, w3, w12, w13n, Q):
    t = smont_mul(c, mont(w1, Q), Q)
    U = smont_mul2(b, mont(w2, Q), d, mont(w12, Q), Q)
    V = smont_mul2(b, mont(w3, Q), d, mont(w13n, Q), Q)
    a1, c1 = wrap32(a + t), wrap32(a - t)
    return wrap32(a1 + U), wrap32(a1 - U), wrap32(c1 + V), wrap32(c1 - V)


def gs_group4_model(a, b, c, d, wa, wb, wg, wag, wbgn, Q):
    s1, s2, X, Y = wrap32(a + b), wrap32(c + d), wrap32(a - b), wrap32(c - d)
    return (wrap32(s1 + s2), smont_mul2(X, mont(wa, Q), Y, mont(wb, Q), Q), smont_mul(wrap32(s1 - s2), mont(wg, Q), Q),
            smont_mul2(X, mont(wag, Q), Y, mont(wbgn, Q), Q))


def ct_exact(a, b, c, d, w1, w2, w3, Q):
    """two Cooley-Tukey stages: bit hi pairs (a, c), (b, d) with w1; bit lo pairs (a, b) with w2, (c, d) with w3"""
    a, b, c, d = ([int(x) for x in v] for v in (a, b, c, d))
    out = []
    for x, y, z, w in zip(a, b, c, d):
        x1, z1, y1, w1_ = (x + w1 * z) % Q, (x - w1 * z) % Q, (y + w1 * w) % Q, (y - w1 * w) % Q
        out.append(((x1 + w2 * y1) % Q, (x1 - w2 * y1) % Q, (z1 + w3 * w1_) % Q, (z1 - w3 * w1_) % Q))
    return np.array(out, dtype=np.int64).T


def gs_exact(a, b, c, d, wa, wb, wg, Q):
    """two Gentleman-Sande stages: bit lo pairs (a, b) with wa, (c, d) with wb; bit hi pairs (a, c), (b, d) with wg"""
    out = []
    for x, y, z, w in zip(*([int(e) for e in v] for v in (a, b, c, d))):
        x1, y1, z1, w1 = (x + y) % Q, (x - y) * wa % Q, (z + w) % Q, (z - w) * wb % Q
        out.append(((x1 + z1) % Q, (y1 + w1) % Q, (x1 - z1) * wg % Q, (y1 - w1) * wg % Q))
    return np.array(out, dtype=np.int64).T


def brv10(k):
    return int(format(k, "010b")[::-1], 2)


def power_tables(P):
    """Table[k] = psi^brv(k), TableI[k] = psi^-brv(k) (nt.h HostNtt)"""
    ipsi = pow(P.psi, -1, P.Q)
    return ([pow(P.psi, brv10(k), P.Q) for k in range(N)], [pow(ipsi, brv10(k), P.Q) for k in range(N)])


def triples():
    """(pair name, outer index k): the inner pair is (2k, 2k + 1); every position of the three pairs of a direction"""
    for j in range(4):
        yield "A bits 2,1", 4 + j
    for l in range(32):
        yield "B bits 4,3", 32 + l
        for j in range(4):
            yield "B bits 2,1", 128 + 4 * l + j


def inputs(bound, rng, n=24):
    """four registers: random up to the bound, and every register at +-bound in all sign patterns"""
    cols = [rng.integers(-bound, bound + 1, 4) for _ in range(n)]
    cols += [np.array(s) * bound for s in itertools.product((1, -1), repeat=4)]
    return np.stack(cols, axis=1).astype(np.int64)


# the proven input bound of each forward pair, units of Q with e = Q 2^-32 (<= 1/32 for FM 1): 3Q/2 + 2^g from the
# first group, a group B -> (1 + 3e) B + Q, a radix-2 stage B -> (1 + e) B + Q/2
def forward_chain(Q, g, groups=(True, True, True)):
    e = F(Q, 1 << 32)
    B = F(3 * Q, 2) + (1 << g)
    bounds = {}
    for name, grp, stages in (("A bits 2,1", groups[0], 2), (None, False, 1), ("B bits 4,3", groups[1], 2),
                              ("B bits 2,1", groups[2], 2), (None, False, 1)):
        if name:
            bounds[name] = B
        if grp:
            B = (1 + 3 * e) * B + Q
        else:
            for _ in range(stages):
                B = (1 + e) * B + F(Q, 2)
    return bounds, B


@pytest.mark.parametrize("name", sorted(MODULI))
def test_forward_groups_equal_two_radix2_stages(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    assert Q == MODULI[name] and P.N == N
    tab, _ = power_tables(P)
    bounds, _ = forward_chain(Q, 10)
    e = F(Q, 1 << 32)
    rng = np.random.default_rng(31)
    for pair, k in triples():
        w1, w2, w3 = tab[k], tab[2 * k], tab[2 * k + 1]
        w12, w13n = w1 * w2 % Q, -w1 * w3 % Q
        B = int(bounds[pair])
        a, b, c, d = inputs(B, rng)
        out = np.stack(ct_group4_model(a, b, c, d, w1, w2, w3, w12, w13n, Q))
        assert np.array_equal(out % Q, ct_exact(a, b, c, d, w1, w2, w3, Q)), (pair, k)
        assert int(np.abs(out).max()) < (1 + 3 * e) * B + Q < 1 << 31, (pair, k)


@pytest.mark.parametrize("name", sorted(MODULI))
def test_inverse_groups_equal_two_radix2_stages(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    _, tabI = power_tables(P)
    # the plan admits a group when |a| + |b| + |c| + |d| <= LIM Q / 10 <= 2^31: every register up to a quarter
    B = (160 if Q < 1 << 27 else 80) * Q // 40
    assert (1 << 31) - (1 << 20) < 4 * B <= 1 << 31
    rng = np.random.default_rng(37)
    for pair, k in triples():
        wg, wa, wb = tabI[k], tabI[2 * k], tabI[2 * k + 1]
        wag, wbgn = wa * wg % Q, -wb * wg % Q
        a, b, c, d = inputs(B, rng)
        out = np.stack(gs_group4_model(a, b, c, d, wa, wb, wg, wag, wbgn, Q))
        assert np.array_equal(out % Q, gs_exact(a, b, c, d, wa, wb, wg, Q)), (pair, k)
        assert np.array_equal(out[0], a + b + c + d)            # the sum, exact in 32 bits
        assert int(np.abs(out[1:]).max()) < Q, (pair, k)        # what the plan counts as 10 (units of Q / 10)


def group_table(Q, table):
    from fhe_amd import binfhe as bf
    L = bf.L()
    L.fhe_hip_stage_group_table.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t]
    t = np.array(table, dtype=np.uint64)
    out = np.zeros(328, np.uint64)
    rc = L.fhe_hip_stage_group_table(Q, t.ctypes.data, len(t), out.ctypes.data, len(out))
    return rc, out


@pytest.mark.parametrize("name", sorted(MODULI))
def test_product_tables_are_products_of_the_power_table(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    for tab in power_tables(P):
        rc, out = group_table(Q, tab)
        assert rc == 0
        for j in range(4):
            assert out[2 * j] == tab[4 + j] * tab[8 + 2 * j] % Q
            assert out[2 * j + 1] == -tab[4 + j] * tab[9 + 2 * j] % Q
        for l in range(32):
            k = 32 + l
            assert out[8 + l] == tab[k] * tab[2 * k] % Q and out[8 + 32 + l] == -tab[k] * tab[2 * k + 1] % Q
            for j in range(4):
                k = 128 + 4 * l + j
                assert out[8 + 32 * (2 + 2 * j) + l] == tab[k] * tab[2 * k] % Q
                assert out[8 + 32 * (3 + 2 * j) + l] == -tab[k] * tab[2 * k + 1] % Q


@pytest.mark.parametrize("name", sorted(MODULI))
def test_table_builder_refuses_corrupted_tables(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    tab, _ = power_tables(P)
    assert group_table(Q, tab)[0] == 0
    # Table[1]; an outer, an even and an odd inner twiddle of the uniform pair and of each lane-major pair
    for k, v in ((1, tab[2]), (5, (tab[5] + 1) % Q), (10, Q - tab[10]), (11, tab[10]), (40, tab[41]),
                 (2 * 40 + 1, tab[2 * 40 + 1] + Q), (2 * (128 + 4 * 31 + 3), 1)):
        bad = list(tab)
        assert bad[k] != v
        bad[k] = v
        assert group_table(Q, bad)[0] == -2, k
        assert b"Table[2k]" in bf.L().fhe_hip_last_error()
    assert group_table(Q - 1, tab)[0] == -2      # even modulus
    assert group_table(Q, tab[:512])[0] == -2    # not a table of 1024


def test_forward_bound_chain():
    """FM 1: with all three pairs grouped the digits end below 6.64 Q + 2^(g+1), inside the 9.5 Q + 2^g everything
    downstream of the pass is proven for (|S| < 40 Q^2 < 2^60, kAccBoundLZ), and below 2^31 throughout.  FM 2: ten
    radix-2 stages after the first group end at 7.43 Q; all three pairs pass 8 Q = 2^31, and any two of them take the
    accumulator past kLmkAcc = 2.4 Q; A' bits 2, 1 alone (what FM 2 takes) ends below 7.52 Q < 8 Q <= 2^31 and keeps
    four such digits times keys < Q at |acc| < 2.38 Q < 2.4 Q.  The subsets the kernels take for FM 1 (A' 2, 1 alone in
    the op-list kernel and with the full monomial table) stay inside 9.5 Q as well."""
    Q = MODULI["std128"]
    for g in range(2, 11):
        bounds, B = forward_chain(Q, g)
        assert B < F(664, 100) * Q + (2 << g) < F(19, 2) * Q + (1 << g) < 1 << 31
        assert all(b < B for b in bounds.values())
        assert 4 * B * Q < 40 * Q * Q < 1 << 60
    Q = 1 << 28                                  # any Q < 2^28, as the kernels' comments argue
    _, B0 = forward_chain(Q, 10, (False, False, False))
    assert B0 < F(744, 100) * Q and B0 < 1 << 31
    assert forward_chain(MODULI["lmkcdey"], 10, (False, False, False))[1] < B0
    _, B3 = forward_chain(Q, 10)
    assert B3 > 1 << 31
    _, B1 = forward_chain(Q, 10, (True, False, False))
    assert B1 < F(752, 100) * Q < 8 * Q <= 1 << 31
    assert 4 * B1 * F(Q, 1 << 32) + F(Q, 2) < F(238, 100) * Q < F(24, 10) * Q
    Q1 = 1 << 27
    for groups in ((True, False, False), (True, True, True)):
        assert forward_chain(Q1, 10, groups)[1] < F(19, 2) * Q1
    for groups in ((True, True, False), (True, False, True), (False, True, True)):
        _, B2 = forward_chain(Q, 10, groups)
        assert 4 * B2 * F(Q, 1 << 32) + F(Q, 2) > F(24, 10) * Q


def test_group_aware_plan_replay(tmp_path):
    exe = str(tmp_path / "red_plan_groups_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "fhe_amd", "csrc"),
                            os.path.join(ROOT, "tests", "red_plan_groups_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and not r.stderr and r.stdout.endswith("OK\n"), r.stdout + r.stderr
    assert "VIOLATION" not in r.stdout
    # K1 GINX: what bootstrap.hip says of its three inverse pairs
    assert "BIN 28 LIM 160 B' bits 1,2: 4 of 8 groups" in r.stdout
    assert "BIN 28 LIM 160 B' bits 3,4: 7 of 8 groups" in r.stdout
    assert "BIN 28 LIM 160 A' bits 1,2: 8 of 8 groups" in r.stdout


# ------------------------------------------------------------------------------------------------ GPU ----
_state = {}


def wave_engine(name):
    """keys, restatement and a context whose gate batches of any size run the one-wave kernel"""
    from fhe_amd import binfhe as bf
    from oracle_lib import Restatement
    if name not in _state:
        ps, m = SETS[name]
        keys = bf.keygen(ps, m, 0x57A6 + ps + m)
        knob = "FHE_HIP_GINX_KERNEL" if name == "std128" else "FHE_HIP_LMK_KERNEL"
        old = os.environ.get(knob)
        os.environ[knob] = "wave"
        try:
            e = bf.GateEngine(ps, m, device=0)
        finally:
            if old is None:
                os.environ.pop(knob)
            else:
                os.environ[knob] = old
        e.load_keys(keys.bsk, keys.kskA, keys.kskB)
        _state[name] = (keys, Restatement(ps, m), e)
    return _state[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["std128", "lmkcdey"])
def test_gpu_one_wave_kernel_other_gates_vs_oracle(name, restatement):
    """5 gates (one full and one partly filled workgroup) of NAND, OR, NOR and XNOR"""
    from fhe_amd import binfhe as bf
    ps, m = SETS[name]
    keys, O, e = wave_engine(name)
    assert e.gate_kernel(5) == ("k_blind_rotate_ginx" if name == "std128" else "k_blind_rotate_lmk")
    rng = np.random.default_rng(11)
    x1, x2 = rng.integers(0, 2, 5), rng.integers(0, 2, 5)
    a1, b1 = bf.encrypt(ps, m, keys.sk, x1, 611)
    a2, b2 = bf.encrypt(ps, m, keys.sk, x2, 612)
    for gate, truth in ((bf.NAND, 1 - (x1 & x2)), (bf.OR, x1 | x2), (bf.NOR, 1 - (x1 | x2)), (bf.XNOR, 1 - (x1 ^ x2))):
        ao, bo = e.eval_gate(gate, a1, b1, a2, b2)
        oa, ob = O.eval_gate(keys.bsk, keys.kskA, keys.kskB, gate, a1, b1, a2, b2)
        assert np.array_equal(ao, oa) and np.array_equal(bo, ob), gate
        assert np.array_equal(bf.decrypt(ps, m, keys.sk, ao, bo), truth.astype(np.int64))


@pytest.mark.gpu
def test_gpu_op_list_kernel_dm_one_gate_vs_oracle(restatement):
    """1 gate on the AP/DM set: the op-list kernel's DM instantiation"""
    from fhe_amd import binfhe as bf
    ps, m = SETS["ap"]
    keys, O, e = wave_engine("ap")
    assert e.gate_kernel(1) == "k_blind_rotate_lmk"
    a1, b1 = bf.encrypt(ps, m, keys.sk, np.array([1]), 621)
    a2, b2 = bf.encrypt(ps, m, keys.sk, np.array([0]), 622)
    ao, bo = e.eval_gate(bf.NAND, a1, b1, a2, b2)
    oa, ob = O.eval_gate(keys.bsk, keys.kskA, keys.kskB, bf.NAND, a1, b1, a2, b2)
    assert np.array_equal(ao, oa) and np.array_equal(bo, ob)
    assert np.array_equal(bf.decrypt(ps, m, keys.sk, ao, bo), np.array([1]))
