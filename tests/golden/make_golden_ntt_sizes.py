"""Generates tests/golden/ntt_sizes.npz by running the REFERENCE itself (oracle/_ref/libfhe_ref.so,
NativePoly::SwitchFormat through ref_ntt) at every power-of-two ring dimension from 4 to 65536.  Run where
the reference is built, on the CPU:

    make -C oracle -j8 && python tests/golden/make_golden_ntt_sizes.py

One row per (N, bits): Q = the largest prime = 1 mod 2N below 2^bits, the reference's psi, the seed of the
inputs (ntt_sizes_common.inputs: one all-(Q-1) row and two uniform rows), the first 8 words and the sha256
of the forward transform of those rows and of their inverse transform (the rows taken as EVALUATION input).
Data only: hashes and a few words per row, no transforms.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ntt_sizes_common import BITS, GOLD, SEED0, SIZES, inputs, largest_prime, sha  # noqa: E402
from oracle_lib import Ref  # noqa: E402


def main():
    ref = Ref(None, None)
    cols = {k: [] for k in ("N", "bits", "Q", "psi", "seed", "fwd8", "inv8", "fwd_sha", "inv_sha")}
    for N in SIZES:
        for bits in BITS:
            Q = largest_prime(N, bits)
            seed = SEED0 + len(cols["N"])
            x = inputs(Q, N, seed)
            fwd, psi = ref.ntt(Q, x, inverse=False)
            inv, psi_i = ref.ntt(Q, x, inverse=True)
            assert psi == psi_i
            for k, v in (("N", N), ("bits", bits), ("Q", Q), ("psi", psi), ("seed", seed), ("fwd8", fwd.reshape(-1)[:8]),
                         ("inv8", inv.reshape(-1)[:8]), ("fwd_sha", sha(fwd)), ("inv_sha", sha(inv))):
                cols[k].append(v)
            print(N, bits, Q, psi, flush=True)
    np.savez(GOLD, N=np.array(cols["N"], np.uint32), bits=np.array(cols["bits"], np.uint32),
             Q=np.array(cols["Q"], np.uint64), psi=np.array(cols["psi"], np.uint64),
             seed=np.array(cols["seed"], np.uint64), fwd8=np.array(cols["fwd8"], np.uint64),
             inv8=np.array(cols["inv8"], np.uint64), fwd_sha=np.array(cols["fwd_sha"]),
             inv_sha=np.array(cols["inv_sha"]))


if __name__ == "__main__":
    main()
