"""Shared by tests/test_ntt_sizes.py, tests/test_ntt_sizes_gpu.py and tests/golden/make_golden_ntt_sizes.py:
the rows of tests/golden/ntt_sizes.npz and how their inputs are drawn."""
import hashlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntt_sizes.npz")
SIZES = [1 << k for k in range(2, 17)]   # 4 .. 65536
BITS = [27, 30, 31, 60]
SEED0 = 0x5EED1000


def is_prime(n):
    """deterministic Miller-Rabin below 2^64"""
    if n < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in bases:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def largest_prime(N, bits):
    """the largest prime = 1 mod 2N below 2^bits"""
    q = ((1 << bits) - 2) // (2 * N) * (2 * N) + 1
    while not is_prime(q):
        q -= 2 * N
    assert q > 2 * N
    return q


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.uint64).tobytes()).hexdigest()


def inputs(Q, N, seed):
    """3 rows: all Q - 1, then two seeded uniform rows"""
    x = np.empty((3, N), np.uint64)
    x[0] = Q - 1
    x[1:] = np.random.default_rng(int(seed)).integers(0, Q, size=(2, N), dtype=np.uint64)
    return x


def rows():
    """the golden rows as dicts (N, bits, Q, psi, seed, fwd8, inv8, fwd_sha, inv_sha)"""
    g = np.load(GOLD)
    return [dict(N=int(g["N"][i]), bits=int(g["bits"][i]), Q=int(g["Q"][i]), psi=int(g["psi"][i]),
                 seed=int(g["seed"][i]), fwd8=g["fwd8"][i], inv8=g["inv8"][i], fwd_sha=str(g["fwd_sha"][i]),
                 inv_sha=str(g["inv_sha"][i])) for i in range(len(g["N"]))]


def check_row(r, fwd, inv):
    """fwd / inv: the (3, N) transforms of inputs(Q, N, seed)"""
    assert np.array_equal(fwd.reshape(-1)[:8], r["fwd8"]) and sha(fwd) == r["fwd_sha"], (r["N"], r["Q"], "forward")
    assert np.array_equal(inv.reshape(-1)[:8], r["inv8"]) and sha(inv) == r["inv_sha"], (r["N"], r["Q"], "inverse")


def negacyclic_mul(a, b, Q):
    """schoolbook a*b mod (X^N + 1, Q) (python ints, exact)."""
    N = len(a)
    r = [0] * N
    for i in range(N):
        ai = int(a[i])
        if ai == 0:
            continue
        for j in range(N):
            k = i + j
            if k < N:
                r[k] += ai * int(b[j])
            else:
                r[k - N] -= ai * int(b[j])
    return np.array([v % Q for v in r], dtype=np.uint64)
