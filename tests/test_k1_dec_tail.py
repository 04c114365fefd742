"""K1's loop inverse ends on the digit decomposition's d + C instead of a canonical coefficient (bootstrap.hip
dec_leg): a numpy model of that leg in the kernel's own arithmetic against decompose2's (canonical value, compare,
select, add), for every residue class near 0, Q/2 and Q - 1 and at the signed extremes of the last stage's words,
for both K1 moduli and both legs' multipliers (2^32 mod Q on the sum leg, TableI[1] on the difference leg).
The GPU side is covered by tests/test_k1_fwd_group.py (same kernels, same restatement) and the gate goldens."""
import numpy as np
import pytest

SETS = {"std128": (3, 2), "lmkcdey": (21, 3)}
MODULI = {"std128": 134215681, "lmkcdey": 268369921}


def dec_leg(a, wR, Q, C):
    """bootstrap.hip dec_leg on int32 words a (as Python-int arrays of dtype object: 64-bit products exactly)"""
    s = Q - (Q >> 1)
    qinv = (-pow(Q, -1, 1 << 32)) % (1 << 32)
    t = a * wR + (s << 32)
    assert all(1 << 32 <= x <= Q << 32 for x in t)
    mm = (t % (1 << 32)) * qinv % (1 << 32)
    z = t + mm * Q
    assert all(x % (1 << 32) == 0 for x in z)
    r = z >> 32
    assert all(1 <= x < 2 * Q for x in r)
    r = np.where(r >= Q, r - Q, r)
    return (r + (C - s)) % (1 << 32)


def decompose2_offset(x, Q, C):
    """decompose2's u = d + C from the canonical x: x >= Q >> 1 ? x + C - Q : x + C, as 32-bit words"""
    return np.where(x >= (Q >> 1), x + C - Q, x + C) % (1 << 32)


def digits(u, g):
    """decompose2<SG>'s two signed digits of u: fields [g, 2g) and [2g, 3g) of u ^ M, sign-extended"""
    h = 1 << (g - 1)
    w = u ^ ((h << g) | (h << (2 * g)))
    f = lambda k: ((w >> (k * g)) % (1 << g) + h) % (1 << g) - h  # noqa: E731
    return f(1), f(2)


def dec_leg2(x, w1R, y, w2R, Q, C):
    """bootstrap.hip dec_leg2: the two-term leg x w1 + y w2"""
    s = Q - (Q >> 1)
    qinv = (-pow(Q, -1, 1 << 32)) % (1 << 32)
    t = x * w1R + y * w2R + (s << 32)
    assert all(1 << 32 <= v <= Q << 32 for v in t)
    mm = (t % (1 << 32)) * qinv % (1 << 32)
    r = (t + mm * Q) >> 32
    assert all(1 <= v < 2 * Q for v in r)
    r = np.where(r >= Q, r - Q, r)
    return (r + (C - s)) % (1 << 32)


@pytest.mark.parametrize("name", sorted(SETS))
def test_grouped_last_inverse_stages_equal_two_radix2_stages(name):
    """inv_pass_s's last two Gentleman-Sande stages of a group {r, r|8, r|16, r|24} as four legs (dec_leg on the
    sums, dec_leg2 on X = a - b, Y = c - d) against the two plain stages mod Q followed by decompose2's offset;
    inputs: random words and the extremes under the plan's bound |a| + |b| + |c| + |d| <= 2^F Q, zeros, all-equal"""
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q, N = P.Q, P.N
    g = P.baseG.bit_length() - 1
    h = 1 << (g - 1)
    C = h * (1 + (1 << g) + (1 << (2 * g)))
    F = 4 if Q < (1 << 27) else 3
    lim = (1 << F) * Q
    M = lambda x: (x << 32) % Q  # noqa: E731
    w1, u, v = (pow(P.psi, -e, Q) for e in (N // 2, N // 4, 3 * N // 4))     # TableI[1..3]
    assert v == w1 * u % Q and w1 * w1 % Q == Q - 1
    rng = np.random.default_rng(77)
    groups = [[int(x) for x in rng.integers(-lim // 4, lim // 4 + 1, 4)] for _ in range(300)]
    groups += [[int(x) for x in rng.integers(-Q, Q + 1, 4)] for _ in range(100)]
    q4 = lim // 4
    for sa in (1, -1):
        for sb in (1, -1):
            for sc in (1, -1):
                for sd in (1, -1):
                    groups.append([sa * q4, sb * q4, sc * q4, sd * q4])
    groups += [[lim - 3, 1, 1, 1], [-(lim - 3), -1, -1, -1], [lim // 2, -(lim // 2), 0, 0], [0, 0, lim // 2, -(lim // 2)],
               [0, 0, 0, 0], [1, 1, 1, 1], [-1, -1, -1, -1], [Q - 1] * 4, [-(Q - 1)] * 4]
    a, b, c, d = (np.array(col, dtype=object) for col in zip(*groups))
    assert all(abs(int(x)) + abs(int(y)) + abs(int(z)) + abs(int(w)) <= lim for x, y, z, w in zip(a, b, c, d))
    s1, s2, X, Y = a + b, c + d, a - b, c - d
    got = {0: dec_leg(s1 + s2, M(1), Q, C), 16: dec_leg(s1 - s2, M(w1), Q, C),
           8: dec_leg2(X, M(u), Y, M(v), Q, C), 24: dec_leg2(X, M(v), Y, M(u), Q, C)}
    # two plain radix-2 Gentleman-Sande stages mod Q (register bit 3 with TableI[2 + (r >> 4)], then bit 4 with TableI[1])
    a1, b1, c1, d1 = (a + b) % Q, (a - b) * u % Q, (c + d) % Q, (c - d) * v % Q
    ref = {0: (a1 + c1) % Q, 16: (a1 - c1) * w1 % Q, 8: (b1 + d1) % Q, 24: (b1 - d1) * w1 % Q}
    for k in ref:
        assert np.array_equal(got[k], decompose2_offset(ref[k], Q, C)), k


@pytest.mark.parametrize("name", sorted(SETS))
def test_dec_leg_equals_decompose2_on_every_boundary(name):
    from fhe_amd import binfhe as bf
    P = bf.params(*SETS[name])
    Q = P.Q
    assert Q == MODULI[name]
    g = P.baseG.bit_length() - 1
    h = 1 << (g - 1)
    C = h * (1 + (1 << g) + (1 << (2 * g)))
    F = 4 if Q < (1 << 27) else 3                      # |x +- y| < 2^F Q < 2^31 in the last stage
    assert (1 << F) * Q < 1 << 31
    oneR = (1 << 32) % Q
    w1R = (pow(P.psi, -(P.N // 2), Q) << 32) % Q       # TableI[1] = psi^-(N/2), Montgomery
    near = sorted({x % Q for c in (0, Q >> 1, (Q + 1) >> 1, Q - 1, C % Q, (Q - C) % Q) for x in range(c - 40, c + 41)})
    rng = np.random.default_rng(5)
    for wR in (oneR, w1R):
        winv = pow(wR, -1, Q)
        words, vals = [], []
        for x in near + [int(v) for v in rng.integers(0, Q, 200)]:
            a0 = (x << 32) * winv % Q                 # a0 wR 2^-32 = x (mod Q)
            for k in sorted({0, -1, 1, -(1 << F), (1 << F) - 1, -(1 << (F - 1)), (1 << (F - 1)) - 1}):
                words.append(a0 + k * Q)
                vals.append(x)
        for a in ((1 << F) * Q - 1, -((1 << F) * Q - 1), (1 << 31) - 1, -(1 << 31), 0, 1, -1):   # the extremes
            words.append(a)
            vals.append(a * wR * pow(1 << 32, -1, Q) % Q)
        a = np.array(words, dtype=object)
        assert all(-(1 << 31) <= x < (1 << 31) for x in a)
        u = dec_leg(a, wR, Q, C)
        ref = decompose2_offset(np.array(vals, dtype=object), Q, C)
        assert np.array_equal(u, ref)
        for got, exp in zip(digits(u, g), digits(ref, g)):
            assert np.array_equal(got, exp)
        # and the digits are the balanced ones: d = d0 + dA 2^g + dB 4^g (mod 8^g: the last digit is the
        # sign-extended g-bit field, as in the reference) with d0, dA in [-2^(g-1), 2^(g-1))
        d = np.array([v - Q if v >= (Q >> 1) else v for v in vals], dtype=object)
        dA, dB = digits(u, g)
        d0 = ((d - dA * (1 << g) - dB * (1 << (2 * g)) + h) % (1 << (3 * g))) - h
        assert all(-h <= x < h for x in d0) and all(-h <= x < h for x in dA)
