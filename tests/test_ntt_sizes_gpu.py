"""The batched negacyclic NTT at every power-of-two ring dimension from 4 to 65536 (ntt_sizes.hip) and the
negacyclic product on the GPU: against the reference's golden rows (tests/golden/ntt_sizes.npz), the
restatement (pinned to those rows by tests/test_ntt_sizes.py; the yardstick above the reference's 60-bit
integers) and the schoolbook product."""
import ctypes

import numpy as np
import pytest

from ntt_sizes_common import SIZES, check_row, inputs, largest_prime, negacyclic_mul, rows

pytestmark = pytest.mark.gpu

ROWS = rows()


class DevBuf:
    """device words through the C-ABI's allocation and copy calls"""

    def __init__(self, words):
        from fhe_amd._lib import check, lib, vp
        self.p, self.words = vp(), words
        check(lib().fhe_hip_alloc(0, max(words, 1) * 8, ctypes.byref(self.p)))

    @property
    def addr(self):
        return self.p.value

    def put(self, a):
        from fhe_amd._lib import check, lib, ptr
        a = np.ascontiguousarray(a, np.uint64)
        check(lib().fhe_hip_copy_to_device(self.p, ptr(a), a.nbytes))
        return self

    def get(self, shape):
        from fhe_amd._lib import check, lib, ptr
        a = np.zeros(shape, np.uint64)
        check(lib().fhe_hip_synchronize(0))
        check(lib().fhe_hip_copy_to_host(ptr(a), self.p, a.nbytes))
        return a

    def free(self):
        from fhe_amd._lib import lib
        lib().fhe_hip_free(self.p)


def resolve_n(kind, wide):
    """an N of the comparison: a fixed size, or the two sides of the one-pass / two-pass cut as the dispatch
    reports it for the arithmetic width"""
    from fhe_amd.ntt import onepass_max
    return {"onepass_max": onepass_max(wide), "twopass_min": 2 * onepass_max(wide)}.get(kind, kind)


def edge_batch(Q, N, count, seed):
    """uniform rows with the lazy bounds' worst cases in front: all Q - 1, alternating Q - 1 / 0, zeros"""
    x = np.random.default_rng(seed).integers(0, Q, size=(count, N), dtype=np.uint64)
    x[0] = Q - 1
    if count > 1:
        x[1, 0::2] = Q - 1
        x[1, 1::2] = 0
    if count > 2:
        x[2] = 0
    return x


# ------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("N", SIZES)
def test_gpu_matches_reference_rows(N):
    from fhe_amd import NttPlan
    for r in (r for r in ROWS if r["N"] == N):
        plan = NttPlan(r["Q"], N=N)   # psi chosen by the library exactly as the reference does
        assert plan.psi == r["psi"], (N, r["Q"])
        x = inputs(r["Q"], N, r["seed"])
        check_row(r, plan.forward(x), plan.inverse(x))
        plan.close()


# ------------------------------------------------------------------ 2. restatement
@pytest.mark.parametrize("bits", [30, 62])
@pytest.mark.parametrize("kind", [4, 8, 64, 512, 2048, 4096, "onepass_max", "twopass_min"])
def test_gpu_matches_restatement(restatement, kind, bits):
    """the largest admissible primes below 2^30 and 2^62 (the lazy bound of each width: 4Q < 2^32, 4Q < 2^64);
    counts 1, 3 and one more than a workgroup transforms (a partial last workgroup wherever it holds several)"""
    from fhe_amd import NttPlan
    N = resolve_n(kind, bits > 30)
    Q = largest_prime(N, bits)
    plan = NttPlan(Q, N=N)
    passes, ppg = plan.dispatch()
    assert passes == (2 if kind == "twopass_min" else 1) and ppg >= 1
    for count in (1, 3, ppg + 1):
        x = edge_batch(Q, N, count, 100 + count)
        f = plan.forward(x)
        assert np.array_equal(f, restatement.ntt(Q, plan.psi, x)), (N, Q, count)
        assert np.array_equal(plan.inverse(x), restatement.ntt(Q, plan.psi, x, inverse=True)), (N, Q, count)
        assert np.array_equal(plan.inverse(f), x), (N, Q, count)


@pytest.mark.parametrize("bits", [30, 62])
@pytest.mark.parametrize("N,cut", [(4096, 2048), (16384, 4096), (65536, 2048), (16384, 16384)])
def test_gpu_moved_cut_same_result(restatement, N, cut, bits):
    """the other side of the cut (two passes with 8 and with 64 rows, blocks smaller than a workgroup's tile,
    one pass at the largest size that fits LDS) computes the same words"""
    from fhe_amd import NttPlan
    Q = largest_prime(N, bits)
    plan = NttPlan(Q, N=N)
    plan.set_onepass_max(cut)
    assert plan.dispatch()[0] == (1 if N <= cut else 2)
    x = edge_batch(Q, N, 3, 7)
    f = plan.forward(x)
    assert np.array_equal(f, restatement.ntt(Q, plan.psi, x))
    assert np.array_equal(plan.inverse(f), x)


# ------------------------------------------------------------------ 3. device entry
@pytest.mark.parametrize("bits", [30, 62])
@pytest.mark.parametrize("kind", ["onepass_max", "twopass_min"])
def test_gpu_device_entry(kind, bits):
    from fhe_amd import NttPlan
    N = resolve_n(kind, bits > 30)
    Q = largest_prime(N, bits)
    plan = NttPlan(Q, N=N)
    count = 5
    x = edge_batch(Q, N, count, 11)
    ref = plan.forward(x)   # the host path
    dx, dy, dz = DevBuf(x.size).put(x), DevBuf(x.size).put(np.zeros_like(x)), DevBuf(x.size).put(np.zeros_like(x))
    try:
        # out of place: the host path's words, the input intact
        plan.run_device(dx.addr, dy.addr, count, False)
        assert np.array_equal(dy.get(x.shape), ref)
        assert np.array_equal(dx.get(x.shape), x)
        # count = 0 touches nothing
        plan.run_device(dx.addr, dy.addr, 0, True)
        plan.run_device(0, 0, 0, False)
        assert np.array_equal(dy.get(x.shape), ref) and np.array_equal(dx.get(x.shape), x)
        # two calls queued on the plan's stream without a synchronise between them: forward into dz, inverse
        # of dz in place
        plan.run_device(dx.addr, dz.addr, count, False)
        plan.run_device(dz.addr, dz.addr, count, True)
        assert np.array_equal(dz.get(x.shape), x)
        # in place (d_in == d_out)
        plan.run_device(dx.addr, dx.addr, count, False)
        assert np.array_equal(dx.get(x.shape), ref)
    finally:
        for d in (dx, dy, dz):
            d.free()


# ------------------------------------------------------------------ 4. product
def test_gpu_multiply_kat():
    """the reference's known-answer test (UnitTestTransform.cpp:57-91): modulus 113, m = 8,
    (1 + 2x + 4x^2 + x^3)^2 -> {94, 109, 11, 18}"""
    from fhe_amd import NttPlan
    plan = NttPlan(113, N=4)
    a = np.array([[1, 2, 4, 1]], dtype=np.uint64)
    assert list(plan.multiply(a, a)[0]) == [94, 109, 11, 18]
    assert lib_plan_n(plan) == 4


def lib_plan_n(plan):
    from fhe_amd._lib import lib
    return int(lib().fhe_hip_ntt_plan_n(plan._h))


@pytest.mark.parametrize("bits", [30, 60])
@pytest.mark.parametrize("N", [1024, 2048, 8192])
def test_gpu_multiply_schoolbook(N, bits):
    """a dense a times a 6-term b == the schoolbook negacyclic product; the second pair of the batch swaps the
    operands.  N = 1024 runs the product on the kernels of ntt.hip."""
    from fhe_amd import NttPlan
    Q = largest_prime(N, bits)
    plan = NttPlan(Q, N=N)
    rng = np.random.default_rng(3)
    a = rng.integers(0, Q, size=(2, N), dtype=np.uint64)
    b = np.zeros((2, N), dtype=np.uint64)
    b[0, rng.choice(N, 6, replace=False)] = rng.integers(1, Q, 6, dtype=np.uint64)
    b[1, rng.choice(N, 6, replace=False)] = Q - 1
    want = np.stack([negacyclic_mul(b[i], a[i], Q) for i in range(2)])   # sparse operand first: 6 N steps
    a0, b0 = a.copy(), b.copy()
    assert np.array_equal(plan.multiply(a, b), want)
    assert np.array_equal(plan.multiply(b, a), want)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    assert plan.multiply(a[:0], b[:0]).shape == (0, N)
    # device entry: out of place with the operands intact, then the result over b
    da, db, do = DevBuf(a.size).put(a), DevBuf(a.size).put(b), DevBuf(a.size).put(np.zeros_like(a))
    try:
        plan.multiply_device(da.addr, db.addr, do.addr, 2)
        assert np.array_equal(do.get(a.shape), want)
        assert np.array_equal(da.get(a.shape), a) and np.array_equal(db.get(a.shape), b)
        plan.multiply_device(da.addr, db.addr, db.addr, 2)
        assert np.array_equal(db.get(a.shape), want)
    finally:
        for d in (da, db, do):
            d.free()


# ------------------------------------------------------------------ 5. the library's rings
def library_rings():
    """every distinct (N, Q, psi) of fhe_hip_params_get over the reference's parameter table and the
    large-precision family, N = 1024 (ntt.hip, tests/test_ntt.py) left out"""
    from fhe_amd import binfhe as bf
    codes = [(ps, m) for ps in range(len(bf.PARAMSETS)) for m in (bf.AP, bf.GINX, bf.LMKCDEY)
             if bf.method_compatible(ps, m)]
    codes += [(bf.large_paramset(ps, arb, logQ), bf.GINX)
              for ps in (bf.TOY, bf.STD128) for arb in (False, True) for logQ in (11, 17, 29)]
    rings = set()
    for ps, m in codes:
        p = bf.params(ps, m)
        if p.N != 1024:
            rings.add((p.N, p.Q, p.psi))
    return sorted(rings)


def test_gpu_library_rings(restatement):
    from fhe_amd import NttPlan
    rings = library_rings()
    assert {N for N, _, _ in rings} >= {512, 2048}
    for N, Q, psi in rings:
        plan = NttPlan(Q, N=N)
        assert plan.psi == psi, (N, Q)
        x = edge_batch(Q, N, 2, N)
        assert np.array_equal(plan.forward(x), restatement.ntt(Q, psi, x)), (N, Q)
        plan.close()


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("Q,N,why", [
    (113, 3, "power of two"), (13, 6, "power of two"), (113, 2, "power of two"),
    (786433, 131072, "power of two in 4 .. 65536"),   # 3 2^18 + 1: prime, 1 mod 2N
    (18433, 2048, "1 mod 2N"),    # 9 2^11 + 1: prime, 1 mod N but not mod 2N
    (4097, 2048, "prime"),        # 1 mod 2N, 17 x 241
])
def test_gpu_refusals(Q, N, why):
    from fhe_amd import FheHipError, NttPlan
    with pytest.raises(FheHipError) as e:
        NttPlan(Q, N=N)
    assert e.value.code == -2 and why in str(e.value), str(e.value)
