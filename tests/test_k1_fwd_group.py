"""K1's signed forward passes run their first two stages (register bits 4 and 3) as one 4-point group with two
products (bootstrap.hip fwd_group4, constants from nt.h fwd_group_consts through the C ABI).

CPU: a numpy model of the group in the kernel's own arithmetic (32-bit words, signed Montgomery products) against
two plain radix-2 Cooley-Tukey stages mod Q, for both K1 moduli; the output bound the later stages rely on; the
table check the builder makes.  GPU: the one-wave kernels K1 (GINX) and the LMKCDEY op-list kernel, pinned by
FHE_HIP_GINX_KERNEL / FHE_HIP_LMK_KERNEL = wave, against the oracle restatement (tests/oracle_lib.py) on the
instantiations the gate goldens do not reach at small batches: partly filled workgroups, XOR's doubled inputs,
the full-resolution monomial table (ciphertext modulus 2N) and the accumulator-I/O seam."""
import ctypes
import os

import numpy as np
import pytest

# (paramset, method) of the two K1 moduli: STD128 GINX (Q = 134215681 < 2^27: FM 1) and STD128_LMKCDEY
# (Q = 268369921 < 2^28: FM 2)
SETS = {"std128": (3, 2), "lmkcdey": (21, 3)}
MODULI = {"std128": 134215681, "lmkcdey": 268369921}


def table123(P):
    """Table[1..3] of the bit-reversed power table: Table[brv(i)] = psi^i over log2(N) bits"""
    return tuple(pow(P.psi, e, P.Q) for e in (P.N // 2, P.N // 4, 3 * P.N // 4))


def group_consts(Q, t1, t2, t3):
    from fhe_amd import binfhe as bf
    L = bf.L()
    L.fhe_hip_fwd_group_consts.argtypes = [ctypes.c_uint64] * 4 + [ctypes.POINTER(ctypes.c_uint64)] * 2
    cp, cm = ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.fhe_hip_fwd_group_consts(Q, t1, t2, t3, ctypes.byref(cp), ctypes.byref(cm))
    return rc, cp.value, cm.value


# ---- the kernel's arithmetic on int64 arrays holding 32-bit two's-complement words -------------------------
def wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def smont_mul(a, bR, Q):
    """boot_arith.h smont_mul: a (int32) * bR (< Q) * 2^-32 mod Q, in (-Q, Q)"""
    qinvp = pow(Q, -1, 1 << 32)
    t = np.asarray(a, np.int64) * np.int64(bR)          # |a| < 2^31, bR < 2^28
    lo = (t.astype(np.uint64) & np.uint64(0xFFFFFFFF)) * np.uint64(qinvp) & np.uint64(0xFFFFFFFF)
    mm = wrap32(lo.astype(np.int64))
    r = t - mm * np.int64(Q)
    assert not np.any(r & 0xFFFFFFFF)
    return r >> 32


def mont(x, Q):
    return (x << 32) % Q


def group4_model(v, Q, t1, cp, cm):
    """fwd_group4 on registers {r, r|8, r|16, r|24}: v is [32, lanes] of int32 words"""
    v = v.copy()
    for r in range(8):
        a, b, c, d = v[r], v[r | 8], v[r | 16], v[r | 24]
        t = smont_mul(c, mont(t1, Q), Q)
        P = smont_mul(wrap32(b + d), mont(cp, Q), Q)
        M = smont_mul(wrap32(b - d), mont(cm, Q), Q)
        X, Y = wrap32(P + M), wrap32(P - M)
        a1, c1 = wrap32(a + t), wrap32(a - t)
        v[r], v[r | 8], v[r | 16], v[r | 24] = wrap32(a1 + X), wrap32(a1 - X), wrap32(c1 + Y), wrap32(c1 - Y)
    return v


def radix2_two_stages(v, Q, t1, t2, t3):
    """the two plain Cooley-Tukey stages on register bits 4 and 3, exact mod Q (fwd_pass2's twA indexing:
    stage bit 4 uses Table[1], stage bit 3 Table[2 + (r >> 4)])"""
    v = [[int(x) % Q for x in row] for row in v]
    for rb, tw in ((4, lambda r: t1), (3, lambda r: (t2, t3)[r >> 4])):
        for r in range(32):
            if r & (1 << rb):
                continue
            s = r | (1 << rb)
            for i in range(len(v[r])):
                t = v[s][i] * tw(r) % Q
                v[r][i], v[s][i] = (v[r][i] + t) % Q, (v[r][i] - t) % Q
    return np.array(v, dtype=np.int64)


def digit_inputs(g, rng, lanes=64):
    """balanced base-2^g digits: random, the extremes +-2^(g-1), 0, all-equal, and each extreme pattern of a group"""
    h = 1 << (g - 1)
    cols = [rng.integers(-h, h + 1, 32) for _ in range(lanes)]
    for c in (h, -h, 0, 1, -1, h - 1):
        cols.append(np.full(32, c))
    for sb, sd in ((1, 1), (1, -1), (-1, 1), (-1, -1)):   # b, d of every group at the extremes: b +- d = +-2^g
        x = rng.integers(-h, h + 1, 32)
        x[8:16], x[24:32] = sb * h, sd * h
        cols.append(x)
        y = np.zeros(32, np.int64)
        y[8:16], y[24:32] = sb * h, sd * h
        cols.append(y)
    alt = np.where(np.arange(32) % 2 == 0, h, -h)
    cols += [alt, -alt]
    return np.stack(cols, axis=1).astype(np.int64)


@pytest.mark.parametrize("name", sorted(SETS))
def test_grouped_first_stages_equal_two_radix2_stages(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    assert Q == MODULI[name] and P.N == 1024
    g = P.baseG.bit_length() - 1
    t1, t2, t3 = table123(P)
    rc, cp, cm = group_consts(Q, t1, t2, t3)
    assert rc == 0
    assert (cp + cm) % Q == t2 and (cp - cm) % Q == t1 * t2 % Q
    v = digit_inputs(g, np.random.default_rng(2024))
    out = group4_model(v, Q, t1, cp, cm)
    ref = radix2_two_stages(v, Q, t1, t2, t3)
    assert np.array_equal(out % Q, ref)
    # the bound the eight later stages start from (bootstrap.hip fwd_group4): 3Q/2 + 2^g
    assert int(np.abs(out).max()) < 3 * Q // 2 + (1 << g)


def test_forward_bounds_follow_from_the_group_bound():
    """the arithmetic of the comments in bootstrap.hip: FM 1 (Q < 2^27) grows by < Q per stage and stays inside the
    bound ten radix-2 stages had; FM 2 (Q < 2^28, no reduction) by B -> (1 + 1/16) B + Q/2 and stays inside 32-bit
    signed words; the LMKCDEY accumulator bound kLmkAcc = 2.4 Q covers four such digits times keys < Q"""
    from fractions import Fraction as F
    Q = MODULI["std128"]
    for g in range(2, 11):
        assert F(3 * Q, 2) + (1 << g) + 8 * Q < 10 * Q + (1 << (g - 1)) < 1 << 31
    Q = MODULI["lmkcdey"]
    B = F(3 * Q, 2) + (1 << 10)
    for _ in range(8):
        B = B * (1 + F(Q, 1 << 32)) + F(Q, 2)
        assert B < 1 << 31
    Bg = F(3, 2) * (1 << 28) + (1 << 10)            # any Q < 2^28
    for _ in range(8):
        Bg = Bg * (1 + F(1, 16)) + F(1 << 27)
    assert Bg < F(744, 100) * (1 << 28) and Bg < 1 << 31
    assert 4 * F(744, 100) / 16 + F(1, 2) < F(24, 10)


@pytest.mark.parametrize("name", sorted(SETS))
def test_table_builder_check_rejects_other_tables(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    t1, t2, t3 = table123(P)
    assert t1 * t1 % Q == Q - 1 and t3 == t1 * t2 % Q
    assert group_consts(Q, t1, t2, t3)[0] == 0
    bad = [(t1, t2, (t3 + 1) % Q), (t1, t2, t2), (t1, t2, Q - t3), (t1, t3, t2), (t2, t2, t3), (1, t2, t2),
           (t1, t2, t3 + Q)]
    for tab in bad:
        rc, _, _ = group_consts(Q, *tab)
        assert rc == -2, tab
        assert b"Table[3]" in bf.L().fhe_hip_last_error()
    assert group_consts(Q - 1, t1, t2, t3)[0] == -2    # even modulus


# ------------------------------------------------------------------------------------------------ GPU ----
_state = {}


def wave_engine(name):
    """keys, restatement and a context whose gate batches of any size run the one-wave kernel"""
    from fhe_amd import binfhe as bf
    from oracle_lib import Restatement
    if name not in _state:
        ps, m = SETS[name]
        keys = bf.keygen(ps, m, 0xD1E7 + ps)
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
        assert e.gate_kernel(1) == e.gate_kernel(5) == ("k_blind_rotate_ginx" if name == "std128" else "k_blind_rotate_lmk")
        _state[name] = (keys, Restatement(ps, m), e)
    return _state[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_gpu_one_wave_kernel_small_batches_vs_oracle(name, restatement):
    """1 gate and 5 gates (a partly filled 4-wave workgroup, then a second one), AND and XOR (doubled inputs)"""
    from fhe_amd import binfhe as bf
    ps, m = SETS[name]
    keys, O, e = wave_engine(name)
    rng = np.random.default_rng(7)
    for count in (1, 5):
        x1, x2 = rng.integers(0, 2, count), rng.integers(0, 2, count)
        a1, b1 = bf.encrypt(ps, m, keys.sk, x1, 300 + count)
        a2, b2 = bf.encrypt(ps, m, keys.sk, x2, 400 + count)
        for gate, truth in ((bf.AND, x1 & x2), (bf.XOR, x1 ^ x2)):
            ao, bo = e.eval_gate(gate, a1, b1, a2, b2)
            oa, ob = O.eval_gate(keys.bsk, keys.kskA, keys.kskB, gate, a1, b1, a2, b2)
            assert np.array_equal(ao, oa) and np.array_equal(bo, ob), (count, gate)
            assert np.array_equal(bf.decrypt(ps, m, keys.sk, ao, bo), truth.astype(np.int64))
            ea, eb = e.eval_gate_extended(gate, a1, b1, a2, b2)
            xa, xb = O.eval_gate(keys.bsk, keys.kskA, keys.kskB, gate, a1, b1, a2, b2, stage=1)
            assert np.array_equal(ea, xa) and np.array_equal(eb, xb), (count, gate)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_gpu_one_wave_kernel_bootstrap_func_at_2N_vs_oracle(name, restatement):
    """BootstrapFunc with ciphertext modulus 2N: any monomial exponent, the full-resolution table (MFULL)"""
    keys, O, e = wave_engine(name)
    P = e.params
    ctmod, fmod, cnt = 2 * P.N, 1 << 16, 5
    rng = np.random.default_rng(19)
    a = rng.integers(0, ctmod, (cnt, P.n), dtype=np.uint64)
    a[:, 0] |= 1                                       # odd exponents present in every gate
    b = rng.integers(0, ctmod, cnt, dtype=np.uint64)
    f = rng.integers(0, fmod, ctmod).astype(np.uint64)
    ga, gb = e.bootstrap_func(a, b, ctmod, f, fmod)
    oa, ob = O.bootstrap_func(keys.bsk, keys.kskA, keys.kskB, a, b, ctmod, (P.Q // fmod) * f, fmod)
    assert np.array_equal(np.asarray(ga, np.uint64), oa) and np.array_equal(np.asarray(gb, np.uint64), ob)


def and_test_vector(P, b):
    """BootstrapGateCore's AND accumulator for test-vector offset b (binfhe-base-scheme.cpp:535-575): COEF"""
    q, Q, N = P.q, P.Q, P.N
    lb, ub, inside, outside = 3 * q // 8, 7 * q // 8, Q // 8 + 1, Q - (Q // 8 + 1)
    factor = 2 * N // q
    m = np.zeros(N, np.uint64)
    for x in range(0, N, factor):
        bx = (b - x // factor) % q
        m[x] = inside if lb <= bx < ub else outside
    return m


def extract(O, P, acc):
    """ctExt of an EVALUATION accumulator (binfhe-base-scheme.cpp:110-121): (Transpose(acc0) in COEF, acc1[0] + Q/8 + 1)"""
    Q = P.Q
    c = O.ntt(Q, P.psi, acc.reshape(-1, P.N), inverse=True).reshape(-1, 2, P.N).astype(np.int64)
    a = np.empty((len(c), P.N), np.int64)
    a[:, 0] = c[:, 0, 0]
    a[:, 1:] = (Q - c[:, 0, :0:-1]) % Q
    return a.astype(np.uint64), ((c[:, 1, 0] + Q // 8 + 1) % Q).astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_gpu_one_wave_kernel_seam_vs_oracle(name, restatement):
    """the accumulator-I/O instantiation (ACCIO): BlindRotate on the AND gate's initial accumulator, read from
    memory, and on the kernel's own test vector (null accumulators), both written back instead of extracted --
    the host-side extraction of either equals the restatement's ctExt of the same AND gates"""
    from fhe_amd import binfhe as bf
    from fhe_amd._lib import check, ptr
    ps, m = SETS[name]
    keys, O, e = wave_engine(name)
    P = e.params
    cnt = 5
    rng = np.random.default_rng(29)
    x1, x2 = rng.integers(0, 2, cnt), rng.integers(0, 2, cnt)
    a1, b1 = bf.encrypt(ps, m, keys.sk, x1, 501)
    a2, b2 = bf.encrypt(ps, m, keys.sk, x2, 502)
    a, b = (a1 + a2) % P.q, (b1 + b2) % P.q
    xa, xb = O.eval_gate(keys.bsk, keys.kskA, keys.kskB, bf.AND, a1, b1, a2, b2, stage=1)
    # BlindRotate on accumulators from memory: acc = (0, NTT(test vector of b))
    acc0 = np.zeros((cnt, 2, P.N), np.uint64)
    acc0[:, 1] = O.ntt(P.Q, P.psi, np.stack([and_test_vector(P, int(x)) for x in b]))
    ctmod = P.q
    if name == "lmkcdey":
        assert P.q == 2 * P.N
    rot = e.blind_rotate_acc(a, ctmod, acc0)
    ga, gb = extract(O, P, rot)
    assert np.array_equal(ga, xa) and np.array_equal(gb, xb)
    # null accumulators: Bootstrap's ct + q/4 (binfhe-base-scheme.cpp:201) through the AND window
    L = bf.L()
    L.fhe_hip_blind_rotate_init_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3
    out = np.zeros((cnt, 2, P.N), np.uint64)
    bq = ((b + P.q - P.q // 4) % P.q).astype(np.uint64)
    check(L.fhe_hip_blind_rotate_init_batch(e._h, cnt, ptr(np.ascontiguousarray(a, np.uint64)), ptr(bq), ptr(out)))
    assert np.array_equal(out, rot)
