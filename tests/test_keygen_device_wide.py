"""Device BTKeyGen for every parameter set (keygen_dev_wide.hip): the sets outside the N = 1024, digitsG = 3 fast
path of keygen_dev.hip, the large-precision family and its timeOptimization map.  The device generator reproduces
the seeded host generator bit for bit, so exported keys hash to the keys the reference was run on for the goldens
(keys_sha), and gates evaluated on the resident keys -- never exported, never generated on the host -- reproduce
the reference's outputs in every resident-layout class."""
import hashlib
import os
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden import GATES, LARGE_SETS, WIDER_PER_GATE, WIDER_SETS  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.uint64).tobytes()).hexdigest()


# ----------------------------------------------------------------- CPU ----
def _plan_rows():
    from fhe_amd import binfhe as bf
    rows = [(ps, m) for ps in range(len(bf.PARAMSETS)) for m in (bf.AP, bf.GINX, bf.LMKCDEY)
            if bf.method_compatible(ps, m)]
    for st in (bf.TOY, bf.STD128):
        for logQ, arb in ((11, False), (12, True), (17, False), (29, False)):
            for topt in (False, True):
                rows.append((bf.large_paramset(st, arb, logQ, 0, topt), bf.GINX))
    return rows


def test_keygen_plan_every_row():
    """fhe_hip_keygen_plan_get for every (paramset, method) row of the table and the large family (logQ 11, 12
    arbFunc, 17, 29; with and without timeOptimization): generated on the device, the switching-key rows in closed
    form, one row pair per 2N raw words less AP's never-drawn j = 0 slots, two transformed polynomials per pair"""
    from fhe_amd import binfhe as bf
    rows = _plan_rows()
    assert len(rows) == 70 + 16
    for ps, m in rows:
        P, k = bf.params(ps, m), bf.keygen_plan(ps, m)
        topt = bool(ps & bf.LARGE) and bool(ps & bf.TIMEOPT) and (ps & 0xff) != 11
        assert k.on_device == 1, (ps, m)
        assert k.keys == (3 if topt else 1), (ps, m)
        assert k.ksk_rows == P.N * P.baseKS * P.digitsKS * k.keys == P.ksk_rows, (ps, m)
        pairs = P.bsk_words // (2 * P.N)
        if m == bf.AP:   # raw [n][baseR][digitsR][dG2][2][N], digitsR = ceil(log_baseR q): the j = 0 slots are not drawn
            dG2 = 2 * (P.digitsG - 1)
            prod = pairs // (P.n * dG2)
            assert pairs == P.n * prod * dG2
            digitsR = [d for d in range(1, 8) if prod % d == 0 and (prod // d) ** d >= P.q > (prod // d) ** (d - 1)]
            assert len(digitsR) == 1, (ps, prod)
            pairs -= P.n * digitsR[0] * dG2
        assert k.row_pairs == pairs, (ps, m, k.row_pairs, pairs)
        assert k.ntt_polys == 2 * k.row_pairs
        assert 0 < k.scratch_bytes <= (768 << 20) + 48 * k.row_pairs + (1 << 20), (ps, m, k.scratch_bytes)


# ----------------------------------------------------------------- GPU ----
SMALL_GATE_SETS = ["toy", "toy_ap", "toy_lmkcdey"]                                        # N = 512, prime qKS
SMALL_LARGE_SETS = ["toy11", "toy12arb", "toy17", "toy29", "toy17t", "toy29t"]            # *t: the three-key map


def _small(name):
    from fhe_amd import binfhe as bf
    if name in SMALL_GATE_SETS:
        g = np.load(os.path.join(GOLD, f"gates_{name}.npz"))
        return g, int(g["paramset"]), int(g["method"]), int(g["key_seed"])
    st, arb, logQ, *topt = LARGE_SETS[name]
    topt = bool(topt and topt[0])
    g = np.load(os.path.join(GOLD, f"large_{name}.npz"))
    seed = 0xB1600000 + logQ + (st << 8) + (int(arb) << 7) + (int(topt) << 6)   # make_golden.large_inputs
    return g, bf.large_paramset(st, arb, logQ, 0, topt), bf.GINX, seed


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL_GATE_SETS + SMALL_LARGE_SETS)
def test_gpu_exported_keys_hash_to_reference_keys(name):
    """the exported raw keys of the device generator are the keys the reference ran on (n = 64 / 32: small
    exports): N = 512 with the prime qKS, AP's zero slots, LMKCDEY's automorphism keys, 27- and 54-bit Q at
    N = 1024 / 2048 with qKS = 2^35, and the concatenated three-key map"""
    from fhe_amd import binfhe as bf
    g, ps, m, seed = _small(name)
    assert bf.keygen_plan(ps, m).on_device == 1
    e = bf.GateEngine(ps, m)
    ks = e.keygen_device(bf.keygen_secret(ps, m, seed), seed, export=True)
    e.close()
    assert sha(ks.bsk) + sha(ks.kskA) + sha(ks.kskB) == str(g["keys_sha"])


# One set per resident-layout class (narrow, g3, n2k, ks32, ks32w) of the committed goldens, the smallest n of
# each; these never run the host generator.
LAYOUT_CLASSES = {
    "std128q": "g3 GINX (g2_key_word), A32, u16 rows",
    "lpf_std128q_lmkcdey": "g3 LMKCDEY (ek / ak), A32, u16 rows",
    "std256q": "n2k GINX, A32, u16 rows",
    "std256q_3_lmkcdey": "n2k LMKCDEY (ek / ak), A32, u16 rows",
    "std256": "n2k GINX at 29-bit Q, digitsG = 3",
    "std256_lmkcdey": "A32 without a second layout, u16 rows",
    "std192q": "A64, u16 rows",
    "std192q_4": "A64, u32 rows (qKS = 2^17)",
    "std256q_4_lmkcdey": "n2k LMKCDEY, digitsG = 5, u32 rows (qKS = 2^17)",
    "signed_mod_test": "prime qKS at N = 1024 with digitsG = 4, A32, u32 rows",
    "std256q_3": "baseKS 21, n2k GINX digitsG = 5, u16 rows",
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUT_CLASSES))
def test_gpu_resident_device_keys_reproduce_reference_gates(name):
    """keys generated straight into the resident layouts (no export, no host key generation) reproduce the
    reference's six gates and their extended outputs"""
    _gates_on_device_keys(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["std128q", "std256q_3_lmkcdey"])
def test_gpu_second_layout_from_64bit_resident_words(name, monkeypatch):
    """FHE_HIP_NARROW=0 keeps the resident key in u64 words (x 2^64 mod Q): the split kernels' second layout is
    then repacked from those with the constant N^-1 2^-32 instead of N^-1"""
    monkeypatch.setenv("FHE_HIP_NARROW", "0")
    _gates_on_device_keys(name)


def _gates_on_device_keys(name):
    from fhe_amd import binfhe as bf
    from make_golden import gate_inputs_for
    g = np.load(os.path.join(GOLD, f"gates_{name}.npz"))
    ps, m, seed = int(g["paramset"]), int(g["method"]), int(g["key_seed"])
    assert (ps, m) == WIDER_SETS[name]
    pg = WIDER_PER_GATE
    sk = bf.keygen_secret(ps, m, seed)
    bits1, bits2, a1, b1, a2, b2 = gate_inputs_for(ps, m, seed, sk, pg)
    assert sha(a1) + sha(b1) + sha(a2) + sha(b2) == str(g["in_sha"])
    e = bf.GateEngine(ps, m, device=0)
    assert e.keygen_device(sk, seed) is None
    outs, outb, exts = [], [], []
    for i, gate in enumerate(GATES.values()):
        sl = slice(i * pg, (i + 1) * pg)
        ao, bo = e.eval_gate(gate, a1[sl], b1[sl], a2[sl], b2[sl])
        ea, eb = e.eval_gate_extended(gate, a1[sl], b1[sl], a2[sl], b2[sl])
        outs.append(ao); outb.append(bo); exts.append(ea)
    e.close()
    assert np.array_equal(np.concatenate(outs), g["out_a"].astype(np.uint64))
    assert np.array_equal(np.concatenate(outb), g["out_b"].astype(np.uint64))
    assert sha(np.concatenate(exts)) == str(g["ext_sha"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy17", "toy29", "toy29t", "toy17t"])
def test_gpu_large_family_on_device_keys(name):
    """the large-precision family keyed by keygen_device: AND / XOR and EvalSign (which walks all three keys of
    the timeOptimization map) against the reference's outputs"""
    from fhe_amd import binfhe as bf
    from make_golden import large_inputs
    g = np.load(os.path.join(GOLD, f"large_{name}.npz"))
    ps, seed, keys, P, b1, b2, (a1, bb1), (a2, bb2), mod, PL, xs, la, lb = large_inputs(name)
    e = bf.GateEngine(ps, bf.GINX)
    e.keygen_device(keys.sk, seed)
    for gname, gate in (("AND", 1), ("XOR", 4)):
        ao, bo = e.eval_gate(gate, a1, bb1, a2, bb2)
        assert np.array_equal(ao, g[f"{gname}_a"]) and np.array_equal(bo, g[f"{gname}_b"]), gname
    ao, bo = e.eval_sign(la, lb, mod)
    e.close()
    assert np.array_equal(ao, g["sign_a"]) and np.array_equal(bo, g["sign_b"])


@pytest.mark.gpu
def test_gpu_context_btkeygen_wide_sets():
    from fhe_amd import binfhe as bf
    for ps, m in ((bf.TOY, bf.LMKCDEY), (bf.PARAMSETS.index("STD128_3"), bf.GINX)):
        cc = bf.BinFHEContext()
        cc.GenerateBinFHEContext(ps, m)
        sk = cc.KeyGen()
        cc.BTKeyGen(sk)
        for x in range(2):
            for y in range(2):
                r = cc.EvalBinGate(bf.NAND, cc.Encrypt(sk, x), cc.Encrypt(sk, y))
                assert cc.Decrypt(sk, r) == 1 - (x & y)


@pytest.mark.gpu
def test_gpu_failed_keygen_leaves_no_keys():
    """a wrong-length secret is refused (FHE_HIP_ERR_INVALID_PARAM) and the context holds no keys: the next gate
    call reports that instead of evaluating"""
    from fhe_amd import binfhe as bf
    from fhe_amd._lib import FheHipError, ptr
    ps, m = WIDER_SETS["toy"]
    e = bf.GateEngine(ps, m)
    sk = bf.keygen_secret(ps, m, 5)
    short = np.ascontiguousarray(sk[:-1])
    assert bf.L().fhe_hip_btkeygen_device(e._h, ptr(short), short.size, 5, None, None, None) == -2
    a, b = bf.encrypt(ps, m, sk, [0, 1], 6)
    with pytest.raises(FheHipError) as err:
        e.eval_gate(bf.AND, a, b, a[::-1].copy(), b[::-1].copy())
    assert err.value.code == -11 and "not loaded" in str(err.value)
    e.close()
