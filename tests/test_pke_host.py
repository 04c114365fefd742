"""Public-key encryption on the host (keygen.cpp pubkey_gen / encrypt_pk; no GPU): the arithmetic of PubKeyGen
(lwe-pke.cpp:74-98) and EncryptN (lwe-pke.cpp:133-167) restated in numpy from the generator's own draws, the draw
order documented in keygen.h restated in Python, the noise bound the formulas give, and batch consistency."""
import bisect
import math

import numpy as np
import pytest

from fhe_amd import binfhe as bf

GINX, LMKCDEY = bf.GINX, bf.LMKCDEY
STD256Q = bf.PARAMSETS.index("STD256Q")
SETS = {
    "toy": (bf.TOY, GINX),                                   # N = 512
    "std128": (bf.STD128, GINX),                             # N = 1024, 27-bit Q
    "std256q": (STD256Q, GINX),                              # N = 2048, u32 words
    "toy_logq17": (bf.large_paramset(bf.TOY, False, 17), GINX),  # N = 2048, 54-bit Q
    "std128_lmkcdey": (bf.STD128_LMKCDEY, LMKCDEY),          # Gaussian skN
}
ARITH_SETS = ("toy", "std128", "std256q", "toy_logq17")
SEED = 0x51C0FFEE
FIN = 39   # the sampler table's end: ceil(3.19 * 12.00610553538285)
H = 27     # numpy products in two 27-bit halves: N * 2^27 * 39 < 2^63

_key = {}


def key(name):
    """(P, skN mod qKS, signed s, A, v) of SEED, computed once per set"""
    if name not in _key:
        ps, m = SETS[name]
        P = bf.params(ps, m)
        skN = bf.keygen_ring_secret(ps, m, SEED)
        s = skN.astype(np.int64)
        s = np.where(s > P.qKS // 2, s - P.qKS, s)
        A, v = bf.pubkeygen(ps, m, skN, SEED)
        _key[name] = (P, skN, s, A, v)
    return _key[name]


def small_times_mod(S, X, Q):
    """(S @ X) mod Q as a Python-int object array, S small signed (|.| <= 39), X < 2^54: int64 matmuls of the two
    27-bit halves of X, recombined in Python integers"""
    S = np.asarray(S, np.int64)
    X = np.asarray(X, np.uint64)
    hi = S @ (X >> np.uint64(H)).astype(np.int64)
    lo = S @ (X & np.uint64((1 << H) - 1)).astype(np.int64)
    return (hi.astype(object) * (1 << H) + lo.astype(object)) % Q


def centred(x, Q):
    x = np.asarray(x, object) % Q
    return np.array([int(t) - Q if int(t) > Q // 2 else int(t) for t in x.ravel()], object).reshape(x.shape)


def test_sets_are_the_intended_shapes():
    assert [key(n)[0].N for n in ARITH_SETS] == [512, 1024, 2048, 2048]
    assert key("std256q")[0].Q < 1 << 31 and key("toy_logq17")[0].Q > 1 << 53
    assert key("std128_lmkcdey")[0].keyDist != key("std128")[0].keyDist
    assert int(np.abs(key("std128_lmkcdey")[2]).max()) > 1 and int(np.abs(key("std128")[2]).max()) == 1


@pytest.mark.parametrize("name", ARITH_SETS)
def test_encrypt_pk_arithmetic_is_the_references(name):
    """a == (e' + S' A) mod Q (lwe-pke.cpp:151-154) and b == (m floor(Q / p) + e'' + S' v) mod Q (:158-162)"""
    ps, m = SETS[name]
    P, skN, s, A, v = key(name)
    Q, count = P.Q, 5
    sp, ep, epp = bf.encrypt_pk_draws(ps, m, count, SEED + 1)
    assert set(np.unique(sp)) == {-1, 0, 1} and np.abs(ep).max() <= FIN and np.abs(epp).max() <= FIN
    assert ep.any()
    want_a = (ep.astype(object) + small_times_mod(sp, A, Q)) % Q
    sv = small_times_mod(sp, v, Q)
    for p in (4, 6, 8):
        bits = np.array([0, 1, 2, 3, p - 1])
        a, b = bf.encrypt_pk(ps, m, A, v, bits, SEED + 1, p)
        assert np.array_equal(a.astype(object), want_a), (name, p)
        want_b = ((bits % p).astype(object) * (Q // p) + epp.astype(object) + sv) % Q
        assert np.array_equal(b.astype(object), want_b), (name, p)


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return z ^ (z >> 31)


def _draw(seed, tag, stream, k):
    """draw k of stream (seed, tag, stream) (keygen.h)"""
    s0 = _mix64((_mix64(seed ^ (tag << 56)) + stream * 0xD1B54A32D192ED03) & (2**64 - 1))
    return _mix64((s0 + (k + 2) * 0x9E3779B97F4A7C15) & (2**64 - 1))


def _dgg(r):
    """keygen.h dgg_sample on the table of discretegaussiangenerator-impl.h:78-97"""
    sigma = 3.19
    fin = math.ceil(sigma * 12.00610553538285)
    vals, c = [], 0.0
    for x in range(1, fin + 1):
        c += math.exp(-((x * x) / (2 * sigma * sigma)))
        vals.append(c)
    a = 1.0 / (2 * c + 1.0)
    vals = [t * a for t in vals]
    seed = (r >> 11) * 2.0**-53 - 0.5
    tmp = abs(seed) - a / 2
    if tmp <= 0:
        return 0
    x = min(bisect.bisect_left(vals, tmp) + 1, fin)
    return x if seed > 0 else -x


T_PKA, T_PKV, T_PKENC = 7, 8, 9


@pytest.mark.parametrize("name", list(SETS))
def test_public_key_is_A_s_plus_the_documented_noise(name):
    """v - A s, centred, is draw j of the error stream through dgg_sample (lwe-pke.cpp:90-95), not identically
    zero; rows of A are the documented uniform draws"""
    ps, m = SETS[name]
    P, skN, s, A, v = key(name)
    e = centred(v.astype(object) - small_times_mod(s[None, :], A.T, P.Q)[0], P.Q)
    assert np.array_equal(e, bf.pubkeygen_draws(ps, m, SEED).astype(object))
    assert np.array_equal(e, np.array([_dgg(_draw(SEED, T_PKV, 0, j)) for j in range(P.N)], object))
    assert any(int(t) != 0 for t in e) and max(abs(int(t)) for t in e) <= FIN
    for j, i in ((0, 0), (1, 5), (P.N - 1, P.N - 1)):
        assert int(A[j, i]) == (_draw(SEED, T_PKA, j, i) * P.Q) >> 64
    assert int(A.max()) < P.Q and int(v.max()) < P.Q


def test_encrypt_pk_draw_order_is_the_documented_one():
    """ciphertext g: stream (seed, T_PKENC, first + g); s' draws 0..N-1, e' draws N..2N-1, e'' draw 2N"""
    ps, m = SETS["toy"]
    N = key("toy")[0].N
    sp, ep, epp = bf.encrypt_pk_draws(ps, m, 2, SEED, first=41)
    for g in range(2):
        for k in (0, 1, N - 1):
            assert sp[g, k] == ((_draw(SEED, T_PKENC, 41 + g, k) * 3) >> 64) - 1
            assert ep[g, k] == _dgg(_draw(SEED, T_PKENC, 41 + g, N + k))
        assert epp[g] == _dgg(_draw(SEED, T_PKENC, 41 + g, 2 * N))


@pytest.mark.parametrize("name", list(SETS))
def test_large_dim_noise_is_within_the_formulas_bound_and_decrypts(name):
    """b - <a, s> - m floor(Q / p) = sum_j s'_j e_j + e'' - <e', s>: at most fin (1 + N (1 + smax)) in absolute
    value, with smax = 1 (ternary skN) or fin (Gaussian); nonzero; far below Q / (2 p), so it decrypts"""
    ps, m = SETS[name]
    P, skN, s, A, v = key(name)
    Q, p, count = P.Q, 4, 64
    smax = FIN if name == "std128_lmkcdey" else 1
    assert int(np.abs(s).max()) <= smax
    bound = FIN * (1 + P.N * (1 + smax))
    assert bound < Q // (2 * p) // 4
    bits = np.arange(count) % p
    a, b = bf.encrypt_pk(ps, m, A, v, bits, SEED + 2, p)
    inner = small_times_mod(s[None, :], a.T, Q)[0]
    err = centred(b.astype(object) - inner - bits.astype(object) * (Q // p), Q)
    assert all(abs(int(t)) <= bound for t in err), (name, max(abs(int(t)) for t in err), bound)
    assert any(int(t) != 0 for t in err)
    assert list(bf.decrypt(ps, m, skN, a, b, mod=Q, p=p)) == list(bits)


def test_batches_are_consistent_and_seeds_independent():
    ps, m = SETS["toy"]
    P, skN, s, A, v = key("toy")
    bits = np.array([0, 1, 2, 3, 0, 1, 2])
    a, b = bf.encrypt_pk(ps, m, A, v, bits, SEED + 3, 4)
    a0, b0 = bf.encrypt_pk(ps, m, A, v, bits[:3], SEED + 3, 4, first=0)
    a1, b1 = bf.encrypt_pk(ps, m, A, v, bits[3:], SEED + 3, 4, first=3)
    assert np.array_equal(a, np.concatenate([a0, a1])) and np.array_equal(b, np.concatenate([b0, b1]))
    a2, b2 = bf.encrypt_pk(ps, m, A, v, bits, SEED + 4, 4)
    assert all(not np.array_equal(a[g], a2[g]) and b[g] != b2[g] for g in range(len(bits)))


def test_pke_capi_exported_and_validates():
    L = bf.L()
    for sym in ("fhe_hip_pubkeygen", "fhe_hip_pubkeygen_draws", "fhe_hip_encrypt_pk", "fhe_hip_encrypt_pk_draws",
                "fhe_hip_load_pubkey", "fhe_hip_pubkeygen_device", "fhe_hip_encrypt_pk_batch",
                "fhe_hip_encrypt_pk_batch_device", "fhe_hip_encrypt_pk_tile", "fhe_hip_copy_keys"):
        assert hasattr(L, sym), sym
    assert bf.encrypt_pk_tile() >= 1
    assert (bf.SYM_ENCRYPT, bf.PUB_ENCRYPT) == (0, 1)
    # a null context is rejected without touching a device
    one = np.zeros(1, np.int32)
    out = np.zeros(4096, np.uint64)
    assert L.fhe_hip_load_pubkey(None, bf.ptr(out), bf.ptr(out)) == -1
    assert L.fhe_hip_pubkeygen_device(None, bf.ptr(out), 1024, 1, None, None) == -1
    assert L.fhe_hip_encrypt_pk_batch(None, bf.ptr(one), 1, 0, 1, 4, 3, bf.ptr(out), bf.ptr(out)) == -1
    assert L.fhe_hip_encrypt_pk_batch_device(None, bf.ptr(one), 1, 0, 1, 4, 3, bf.ptr(out), bf.ptr(out), None) == -1
    # host refusals: the plaintext modulus, a key not reduced mod Q, a secret outside the key distributions
    ps, m = SETS["std128"]
    P, skN, s, A, v = key("std128")
    for bad_p in (0, 1, P.Q + 1):
        with pytest.raises(bf.FheHipError) as e:
            bf.encrypt_pk(ps, m, A, v, [1], SEED, bad_p)
        assert e.value.code == -2
    assert len(bf.encrypt_pk(ps, m, A, v, [], SEED, 4)[1]) == 0    # count = 0: a no-op
    A2 = A.copy()
    A2[3, 4] = P.Q
    with pytest.raises(bf.FheHipError) as e:
        bf.encrypt_pk(ps, m, A2, v, [1], SEED, 4)
    assert e.value.code == -2
    bad = skN.copy()
    bad[0] = 100
    with pytest.raises(bf.FheHipError) as e:
        bf.pubkeygen(ps, m, bad, SEED)
    assert e.value.code == -2
