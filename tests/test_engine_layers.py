"""The host layer between the C-ABI and the launchers (engine.cpp / engine_host.cpp / devbuf.h):

  * the blind-rotation plan: fhe_hip_gate_kernel reports what Engine::plan_rotation decides and rotate_device
    launches, asserted here on the 64-bit path's branches (the 32-bit path's names are asserted in test_capi.py,
    test_gates.py, test_circuit_func.py and test_k1_fwd_group.py);
  * the host-buffer entry points against their _device forms, bit for bit, while one context's staging block and
    workspace grow, grow again and are reused;
  * the Carver that sizes and lays out the staging block, as a stand-alone host program under the sanitizers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

# one set per branch of the 64-bit path's plan (the smallest keys of each): the kernel a keyed context reports for
# AND batches, the knob that keeps the set off that kernel, and the kernel it then falls back to.  The two rows
# without a faster kernel take FHE_HIP_NARROW, which changes the residue width (kernel code 3 -> 0), not the kernel.
WIDE_ROWS = {
    "std128q": ("k_blind_rotate_ginx2", "FHE_HIP_GINX3", "k_blind_rotate_wide"),                # K1s-3 GINX
    "lpf_std128q_lmkcdey": ("k_blind_rotate_lmk3", "FHE_HIP_GINX3", "k_blind_rotate_wide_ops"),  # K1m-3 LMKCDEY
    "std256": ("k_blind_rotate_n2k", "FHE_HIP_N2K", "k_blind_rotate_wide"),                      # K1w GINX
    "std256q_lmkcdey": ("k_blind_rotate_lmk2k", "FHE_HIP_N2K", "k_blind_rotate_wide_ops"),       # K1w LMKCDEY
    "toy_lmkcdey": ("k_blind_rotate_wide_ops", "FHE_HIP_NARROW", "k_blind_rotate_wide_ops"),     # the op-list kernel
    "toy": ("k_blind_rotate_wide", "FHE_HIP_NARROW", "k_blind_rotate_wide"),                     # plain K5
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE_ROWS))
def test_gpu_gate_kernel_wide_rows(name, monkeypatch):
    from fhe_amd import binfhe as bf
    from make_golden import WIDER_SETS
    ps, m = WIDER_SETS[name]
    kernel, knob, fallback = WIDE_ROWS[name]
    for k in ("FHE_HIP_GINX3", "FHE_HIP_N2K", "FHE_HIP_NARROW", "FHE_HIP_KS32"):
        monkeypatch.delenv(k, raising=False)
    sk = bf.keygen_secret(ps, m, 0xE1)
    e = bf.GateEngine(ps, m, device=0)
    keys = e.keygen_device(sk, 0xE1, export=True)
    assert e.gate_kernel(1) == kernel and e.gate_kernel(37) == kernel
    assert e.kernel() == bf.params(ps, m).kernel
    # the name belongs to a context that really launched: three AND gates, decrypted
    x1, x2 = np.array([0, 1, 1]), np.array([1, 1, 0])
    a1, b1 = bf.encrypt(ps, m, sk, x1, 0xE2)
    a2, b2 = bf.encrypt(ps, m, sk, x2, 0xE3)
    ao, bo = e.eval_gate(bf.AND, a1, b1, a2, b2)
    assert list(bf.decrypt(ps, m, sk, ao, bo)) == [0, 1, 0]
    assert e.gate_kernel(1) == kernel
    e.close()
    # the same keys in a context created with the knob off
    monkeypatch.setenv(knob, "0")
    f = bf.GateEngine(ps, m, device=0)
    f.load_keys(keys.bsk, keys.kskA, keys.kskB)
    assert f.gate_kernel(1) == fallback and f.gate_kernel(37) == fallback
    assert f.kernel() == bf.params(ps, m).kernel
    if fallback != kernel:
        assert f.kernel() in (0, 3)
    else:
        assert f.kernel() == 0
    fo = f.eval_gate(bf.AND, a1, b1, a2, b2)
    f.close()
    assert np.array_equal(fo[0], ao) and np.array_equal(fo[1], bo)


class _Dev:
    """device buffers from fhe_hip_alloc, freed together"""

    def __init__(self):
        from fhe_amd import binfhe as bf
        self.L, self.ptrs = bf.L(), []

    def put(self, x):
        from fhe_amd._lib import check
        x = np.ascontiguousarray(x)
        d = ctypes.c_void_p()
        check(self.L.fhe_hip_alloc(0, max(x.nbytes, 8), ctypes.byref(d)))
        self.ptrs.append(d)
        check(self.L.fhe_hip_copy_to_device(d, x.ctypes.data, x.nbytes))
        return d.value

    def out(self, *shape):
        return self.put(np.zeros(shape, np.uint64))

    def get(self, d, *shape):
        from fhe_amd._lib import check
        h = np.zeros(shape, np.uint64)
        check(self.L.fhe_hip_synchronize(0))
        check(self.L.fhe_hip_copy_to_host(h.ctypes.data, ctypes.c_void_p(d), h.nbytes))
        return h

    def free(self):
        for d in self.ptrs:
            self.L.fhe_hip_free(d)
        self.ptrs = []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "medium"])
def test_gpu_host_path_equals_device_path_across_growth(name):
    """TOY (64-bit path) and MEDIUM (32-bit path), one context each, counts 1, 5, 2: the staging block and the
    workspace grow, grow again and are reused.  Every host entry point against its _device form on caller-allocated
    buffers, bit for bit.  KeySwitch on caller-provided ctExt has no _device form in the C-ABI: its rows are
    compared with one 5-row call on a second context that never grew."""
    from fhe_amd import binfhe as bf
    from fhe_amd._lib import check, sz, vp
    from make_golden import WIDER_SETS
    ps, m = WIDER_SETS[name]
    P = bf.params(ps, m)
    n, N, q = P.n, P.N, P.q
    sk = bf.keygen_secret(ps, m, 0xE5)
    e, e2 = bf.GateEngine(ps, m, device=0), bf.GateEngine(ps, m, device=0)
    keys = e.keygen_device(sk, 0xE5, export=True)
    e2.load_keys(keys.bsk, keys.kskA, keys.kskB)
    rng = np.random.default_rng(0xE6)
    M = 5
    cols = [bf.encrypt(ps, m, sk, rng.integers(0, 2, M), 0xE7 + j, 8) for j in range(4)]   # AND4: p = 8
    g1, g2, g3 = (bf.encrypt(ps, m, sk, rng.integers(0, 2, M), 0xF0 + j) for j in range(3))
    big_a = rng.integers(0, P.Q, (M, N), dtype=np.uint64)     # ciphertexts mod Q (SwitchCTtoqn)
    big_b = rng.integers(0, P.Q, M, dtype=np.uint64)
    ks_a = rng.integers(0, P.qKS, (M, N), dtype=np.uint64)    # ctExt mod qKS (KeySwitch)
    ks_b = rng.integers(0, P.qKS, M, dtype=np.uint64)
    half = rng.integers(1, q, q // 2, dtype=np.uint64)
    lut = np.concatenate([half, q - half])                    # negacyclic: one bootstrap
    ks_all = e2.keyswitch(ks_a, ks_b)
    e2.close()
    circ = bf.Circuit()
    x, y = circ.input(), circ.input()
    t = circ.gate(bf.NAND, x, y)
    u = circ.gate(bf.OR, t, x)
    circ.output(circ.gate(bf.AND, u, y))
    circ.output(t)
    circ.finalize()
    L = bf.L()
    D = _Dev()

    def same(host, dao, dbo, rows, width, what):
        ga, gb = D.get(dao, rows, width), D.get(dbo, rows)
        assert np.array_equal(host[0].reshape(rows, width), ga) and np.array_equal(host[1].reshape(rows), gb), what

    try:
        for c in (1, 5, 2):
            s = slice(0, c)
            # the 2-input gate
            dao, dbo = D.out(c, n), D.out(c)
            host = e.eval_gate(bf.AND, g1[0][s], g1[1][s], g2[0][s], g2[1][s])
            e.eval_gate_device(bf.AND, c, D.put(g1[0][s]), D.put(g1[1][s]), D.put(g2[0][s]), D.put(g2[1][s]), dao, dbo)
            same(host, dao, dbo, c, n, ("gate", c))
            # AND4, switched and extended (k = 4, the widest staging)
            A, B = [a[s] for a, _ in cols], [b[s] for _, b in cols]
            dA, dB = [D.put(a) for a in A], [D.put(b) for b in B]
            dao, dbo = D.out(c, n), D.out(c)
            host = e.eval_gate_multi(bf.AND4, A, B, 8)
            e.eval_gate_multi_device(bf.AND4, c, 8, dA, dB, dao, dbo)
            same(host, dao, dbo, c, n, ("AND4", c))
            dao, dbo = D.out(c, N), D.out(c)
            host = e.eval_gate_multi(bf.AND4, A, B, 8, extended=True)
            pa, pb = (vp * 4)(*dA), (vp * 4)(*dB)
            check(L.fhe_hip_eval_mixed_batch_device(e._h, bf.AND4, 4, 8, c, pa, pb, None, vp(dao), vp(dbo), 1, None))
            same(host, dao, dbo, c, N, ("AND4 extended", c))
            # CMUX (a workspace of 2 x count)
            dao, dbo = D.out(c, n), D.out(c)
            host = e.eval_cmux(g1[0][s], g1[1][s], g2[0][s], g2[1][s], g3[0][s], g3[1][s])
            e.eval_cmux_device(c, D.put(g1[0][s]), D.put(g1[1][s]), D.put(g2[0][s]), D.put(g2[1][s]), D.put(g3[0][s]),
                               D.put(g3[1][s]), dao, dbo)
            same(host, dao, dbo, c, n, ("CMUX", c))
            # Bootstrap (refresh)
            dao, dbo = D.out(c, n), D.out(c)
            host = e.bootstrap(g3[0][s], g3[1][s])
            check(L.fhe_hip_bootstrap_batch_device(e._h, sz(c), vp(D.put(g3[0][s])), vp(D.put(g3[1][s])), vp(dao),
                                                   vp(dbo), None))
            same(host, dao, dbo, c, n, ("refresh", c))
            # SwitchCTtoqn
            dao, dbo = D.out(c, n), D.out(c)
            host = e.switch_to_qn(big_a[s], big_b[s])
            check(L.fhe_hip_switch_to_qn_batch_device(e._h, c, D.put(big_a[s]), D.put(big_b[s]), dao, dbo, None))
            same(host, dao, dbo, c, n, ("switch_to_qn", c))
            # KeySwitch
            host = e.keyswitch(ks_a[s], ks_b[s])
            assert np.array_equal(host[0], ks_all[0][s]) and np.array_equal(host[1], ks_all[1][s]), ("keyswitch", c)
            # EvalFunc, negacyclic LUT
            dao, dbo = D.out(c, n), D.out(c)
            host = e.eval_func(g1[0][s], g1[1][s], q, lut)
            check(L.fhe_hip_eval_func_batch_device(e._h, c, D.put(g1[0][s]), D.put(g1[1][s]), q, lut.ctypes.data,
                                                   len(lut), dao, dbo, None))
            same(host, dao, dbo, c, n, ("EvalFunc", c))
            # a 3-node circuit, B = count
            ca, cb = np.stack([g1[0][s], g2[0][s]]), np.stack([g1[1][s], g2[1][s]])
            dao, dbo = D.out(2, c, n), D.out(2, c)
            host = e.eval_circuit(circ, ca, cb)
            e.eval_circuit_device(circ, c, D.put(ca), D.put(cb), dao, dbo)
            same(host, dao, dbo, 2 * c, n, ("circuit", c))
            D.free()
    finally:
        check(L.fhe_hip_synchronize(0))
        D.free()
        e.close()
        circ.close()


def test_carver_layout_and_bounds(tmp_path):
    """devbuf.h's Carver without HIP: the listed layout and the hand-out agree, a request past the end (or of
    another size than listed) throws std::logic_error.  Plain host code, so it runs under ASan and UBSan: every
    sub-array of a block of exactly words() words is written in full."""
    exe = str(tmp_path / "carver_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "fhe_amd", "csrc"),
                            os.path.join(ROOT, "tests", "carver_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "carver ok", run.stdout + run.stderr
