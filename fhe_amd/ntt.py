"""Batched negacyclic NTT on the GPU, any power-of-two N in 4 .. 65536 -- mirrors NativePoly::SwitchFormat
(src/core/include/lattice/hal/default/poly-impl.h:420-440 in the reference) -- and the negacyclic
product built on it (SwitchFormat / Times / SwitchFormat)."""
import ctypes

import numpy as np

from ._lib import check, lib, ptr, u64, vp


def onepass_max(wide):
    """Largest N (other than 1024, which has kernels of its own) transformed in one pass, for the
    32-bit (wide false: Q < 2^30) or the 64-bit arithmetic; larger N take two passes."""
    return int(lib().fhe_hip_ntt_onepass_max(int(bool(wide))))


class NttPlan:
    """Plan for prime Q = 1 mod 2N, Q < 2^62, and N a power of two in 4 .. 65536; psi = 0 picks
    the reference's minimal primitive 2N-th root."""

    def __init__(self, Q, psi=0, N=1024, device=0):
        self._h = vp()
        psi_out = u64()
        check(lib().fhe_hip_ntt_plan_create(Q, psi, N, device, ctypes.byref(self._h), ctypes.byref(psi_out)))
        self.Q, self.psi, self.N, self.device = int(Q), int(psi_out.value), N, device

    def close(self):
        if self._h:
            lib().fhe_hip_ntt_plan_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().fhe_hip_ntt_plan_stream(self._h)

    def dispatch(self):
        """(passes, polynomials per workgroup) of this plan's launches."""
        passes, ppg = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().fhe_hip_ntt_plan_dispatch(self._h, ctypes.byref(passes), ctypes.byref(ppg)))
        return int(passes.value), int(ppg.value)

    def set_onepass_max(self, n):
        """Move this plan's one-pass / two-pass cut (measurement; results do not change)."""
        check(lib().fhe_hip_ntt_plan_set_onepass_max(self._h, n))

    def forward(self, polys):
        """COEFFICIENT -> EVALUATION (bit-reversed); returns a new uint64 array."""
        return self._run(polys, 0)

    def inverse(self, polys):
        return self._run(polys, 1)

    def _batch(self, polys):
        a = np.array(polys, dtype=np.uint64, copy=True, order="C")
        if a.ndim != 2 or a.shape[1] != self.N:
            raise ValueError(f"expected shape (count, {self.N})")
        return a

    def _run(self, polys, inv):
        a = self._batch(polys)
        check(lib().fhe_hip_ntt_batch(self._h, ptr(a), a.shape[0], inv))
        return a

    def multiply(self, a, b):
        """Negacyclic products a[i] * b[i] mod (X^N + 1, Q); a, b and the result in COEFFICIENT form."""
        a, b = self._batch(a), self._batch(b)
        if a.shape != b.shape:
            raise ValueError("a and b must have the same shape")
        check(lib().fhe_hip_poly_mul_batch(self._h, ptr(a), ptr(b), ptr(a), a.shape[0]))
        return a

    def run_device(self, d_in, d_out, count, inverse=False, stream=None):
        """Asynchronous transform of device buffers (raw device pointers as ints)."""
        check(lib().fhe_hip_ntt_batch_device(self._h, vp(d_in), vp(d_out), count, int(inverse),
                                             vp(stream) if stream else None))

    def multiply_device(self, d_a, d_b, d_out, count, stream=None):
        """Asynchronous negacyclic product of device buffers (raw device pointers as ints)."""
        check(lib().fhe_hip_poly_mul_batch_device(self._h, vp(d_a), vp(d_b), vp(d_out), count,
                                                  vp(stream) if stream else None))
