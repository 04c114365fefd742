"""The yardstick of the general-N transform (CPU): the restatement reproduces the reference's golden rows
(tests/golden/ntt_sizes.npz, written by tests/golden/make_golden_ntt_sizes.py from the reference itself) at
every power-of-two ring dimension from 4 to 65536.  The GPU tests of tests/test_ntt_sizes_gpu.py compare the
kernels with these rows and with the restatement."""
import numpy as np
import pytest

from ntt_sizes_common import BITS, SIZES, check_row, inputs, largest_prime, rows

ROWS = rows()


def test_golden_rows_cover_every_size_and_bound():
    assert [(r["N"], r["bits"]) for r in ROWS] == [(N, b) for N in SIZES for b in BITS]
    for r in ROWS:
        assert r["Q"] == largest_prime(r["N"], r["bits"])


@pytest.mark.parametrize("N", SIZES)
def test_restatement_matches_reference_rows(restatement, N):
    for r in (r for r in ROWS if r["N"] == N):
        x = inputs(r["Q"], N, r["seed"])
        check_row(r, restatement.ntt(r["Q"], r["psi"], x), restatement.ntt(r["Q"], r["psi"], x, inverse=True))


def test_restatement_roots_match_reference_rows(restatement):
    for r in ROWS:
        assert restatement.L.tfo_root_of_unity(2 * r["N"], r["Q"]) == r["psi"], (r["N"], r["Q"])


def test_restatement_kat_at_n4(restatement):
    """the reference's arithmetic known-answer test (UnitTestTransform.cpp:57-91) has a row's N: 4"""
    Q = 113
    psi = restatement.L.tfo_root_of_unity(8, Q)
    A = restatement.ntt(Q, psi, np.array([[1, 2, 4, 1]], dtype=np.uint64))
    r = restatement.ntt(Q, psi, (A * A) % np.uint64(Q), inverse=True)
    assert list(r[0]) == [94, 109, 11, 18]
