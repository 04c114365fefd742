"""Public-key encryption on the device (pke.hip, pke_engine.cpp): PubKeyGen and EncryptN bit for bit against the
host generator (tests/test_pke_host.py pins that one to the reference's lines), SMALL_DIM against the existing
SwitchCTtoqn, and the reference's examples/pke flows through the BinFHEContext mirror."""
import ctypes

import numpy as np
import pytest

from test_pke_host import SEED, SETS, key

pytestmark = pytest.mark.gpu

LARGE_SETS = ("toy", "std128", "std256q", "toy_logq17", "std128_lmkcdey")
_eng, _ctx = {}, {}


def engine(name):
    """a context of the set with the public key of SEED generated on the device (no other keys)"""
    from fhe_amd import binfhe as bf
    if name not in _eng:
        e = bf.GateEngine(*SETS[name], 0)
        _eng[name] = (e, e.pubkeygen_device(key(name)[1], SEED, export=True))
    return _eng[name]


def context(which):
    """a BinFHEContext after KeyGen and BTKeyGen(sk, PUB_ENCRYPT)"""
    from fhe_amd import binfhe as bf
    sets = {"std128": (bf.STD128, bf.GINX), "std128_lmkcdey": (bf.STD128_LMKCDEY, bf.LMKCDEY),
            "std128_ap": (bf.STD128_AP, bf.AP), "toy": (bf.TOY, bf.GINX),
            "signed_mod_test": (bf.PARAMSETS.index("SIGNED_MOD_TEST"), bf.GINX)}
    if which not in _ctx:
        cc = bf.BinFHEContext()
        cc.GenerateBinFHEContext(*sets[which])
        sk = cc.KeyGen()
        cc.BTKeyGen(sk, bf.PUB_ENCRYPT)
        _ctx[which] = (cc, sk)
    return _ctx[which]


@pytest.mark.parametrize("name", LARGE_SETS)
def test_gpu_pubkeygen_device_is_the_host_key(name):
    P, skN, s, A, v = key(name)
    e, (dA, dv) = engine(name)
    assert np.array_equal(dv, v) and np.array_equal(dA, A)


@pytest.mark.parametrize("name", LARGE_SETS)
def test_gpu_encrypt_pk_large_dim_is_the_host_encryption(name):
    """counts around the kernel's ciphertext tile, both plaintext moduli and offsets, generated and loaded key"""
    from fhe_amd import binfhe as bf
    ps, m = SETS[name]
    P, skN, s, A, v = key(name)
    e, _ = engine(name)
    G = bf.encrypt_pk_tile()
    top = 2 * G + 5
    want = {}
    for p in (4, 6):
        for first in (0, 1000):
            bits = (np.arange(top) * 7 + first) % p
            want[p, first] = (bits, *bf.encrypt_pk(ps, m, A, v, bits, SEED + 5, p, first))
            for count in (1, 3, G + 1, top):
                a, b = e.encrypt_pk(bits[:count], SEED + 5, p, bf.LARGE_DIM, first)
                assert a.shape == (count, P.N)
                assert np.array_equal(b, want[p, first][2][:count]), (name, p, first, count)
                assert np.array_equal(a, want[p, first][1][:count]), (name, p, first, count)
    e.load_pubkey(A, v)
    for (p, first), (bits, wa, wb) in want.items():
        a, b = e.encrypt_pk(bits[:G + 1], SEED + 5, p, bf.LARGE_DIM, first)
        assert np.array_equal(a, wa[:G + 1]) and np.array_equal(b, wb[:G + 1]), (name, p, first, "loaded")


@pytest.mark.parametrize("which", ("std128", "std128_lmkcdey", "std128_ap"))
def test_gpu_small_dim_is_switch_to_qn_of_large_dim_and_decrypts(which):
    from fhe_amd import binfhe as bf
    cc, sk = context(which)
    bits = np.arange(64) % 4
    al, bl = cc.engine.encrypt_pk(bits, SEED + 6, 4, bf.LARGE_DIM)
    a, b = cc.engine.encrypt_pk(bits, SEED + 6, 4, bf.SMALL_DIM)
    sa, sb = cc.engine.switch_to_qn(al, bl)
    assert a.shape == (64, cc.params.n)
    assert np.array_equal(a, sa) and np.array_equal(b, sb)
    assert list(bf.decrypt(cc.paramset, cc.method, sk.s, a, b)) == list(bits)


TRUTH = {"AND": lambda x, y: x & y, "OR": lambda x, y: x | y, "NAND": lambda x, y: 1 - (x & y),
         "NOR": lambda x, y: 1 - (x | y), "XOR": lambda x, y: x ^ y, "XNOR": lambda x, y: 1 - (x ^ y)}


@pytest.mark.parametrize("which", ("std128", "std128_lmkcdey", "std128_ap"))
def test_gpu_boolean_pke_flow_through_the_mirror(which):
    """boolean-pke.cpp / UnitTestFHEWPKE.cpp: KeyGen, BTKeyGen(sk, PUB_ENCRYPT), Encrypt(GetPublicKey(), b), then
    NOT, Bootstrap and the six gates on all four input pairs, inputs SMALL_DIM and LARGE_DIM.  Bootstrap's
    decryption is asserted on SMALL_DIM inputs only: on a ciphertext mod Q the reference's Bootstrap adds Q / 4 at
    the switched modulus q (binfhe-base-scheme.cpp:199-201) and its test vector is constant, which the mixed entry
    point mirrors (tests/test_mixed.py pins it bit for bit); NOT of a LARGE_DIM input is checked through a gate"""
    from fhe_amd import binfhe as bf
    cc, sk = context(which)
    pk = cc.GetPublicKey()
    for dim in (bf.SMALL_DIM, bf.LARGE_DIM):
        for x in (0, 1):
            ct = cc.Encrypt(pk, x, dim)
            assert ct.modulus == (cc.params.Q if dim == bf.LARGE_DIM else cc.params.q)
            assert len(ct.a) == (cc.params.N if dim == bf.LARGE_DIM else cc.params.n)
            if dim == bf.SMALL_DIM:
                assert cc.Decrypt(sk, ct) == x and cc.Decrypt(sk, cc.EvalNOT(ct)) == 1 - x
                assert cc.Decrypt(sk, cc.Bootstrap(ct)) == x
                assert cc.Decrypt(sk, cc.Bootstrap(cc.EvalNOT(ct))) == 1 - x
            else:
                assert cc.Decrypt(sk, cc.EvalBinGate(bf.AND, cc.EvalNOT(ct), cc.Encrypt(pk, 1, dim))) == 1 - x
        for gname, f in TRUTH.items():
            for x in (0, 1):
                for y in (0, 1):
                    out = cc.EvalBinGate(bf.GATE_NAMES[gname], cc.Encrypt(pk, x, dim), cc.Encrypt(pk, y, dim))
                    assert cc.Decrypt(sk, out) == f(x, y), (which, dim, gname, x, y)


@pytest.mark.parametrize("which", ("toy", "signed_mod_test"))
def test_gpu_boolean_pke_flow_on_the_references_test_sets(which):
    """the same flow on the sets UnitTestFHEWPKE.cpp runs: the gate outputs are eval_mixed's on the same arrays
    bit for bit; the truth table where that composition of existing entry points decrypts correctly too"""
    from fhe_amd import binfhe as bf
    cc, sk = context(which)
    pk = cc.GetPublicKey()
    for dim in (bf.SMALL_DIM, bf.LARGE_DIM):
        large = [np.ones(1, np.uint8)] * 2 if dim == bf.LARGE_DIM else None
        for gname, f in TRUTH.items():
            for x in (0, 1):
                for y in (0, 1):
                    c1, c2 = cc.Encrypt(pk, x, dim), cc.Encrypt(pk, y, dim)
                    out = cc.EvalBinGate(bf.GATE_NAMES[gname], c1, c2)
                    ma, mb = cc.engine.eval_mixed(bf.GATE_NAMES[gname], [c1.a[None, :], c2.a[None, :]],
                                                  [np.array([c1.b], np.uint64), np.array([c2.b], np.uint64)], large)
                    assert np.array_equal(out.a, ma[0]) and out.b == int(mb[0]), (which, dim, gname, x, y)
                    if int(bf.decrypt(cc.paramset, cc.method, sk.s, ma, mb)[0]) == f(x, y):
                        assert cc.Decrypt(sk, out) == f(x, y)


def test_gpu_eval_function_pke():
    """eval-function-pke.cpp: EvalFunc of Encrypt(pk, m, SMALL_DIM, p) with GenerateLUTviaFunction"""
    from fhe_amd import binfhe as bf
    cc, sk = context("std128")
    p = cc.GetMaxPlaintextSpace()
    lut = cc.GenerateLUTviaFunction(lambda m, p1: (m * m * m) % p1, p)
    for m in range(p):
        ct = cc.Encrypt(cc.GetPublicKey(), m, bf.SMALL_DIM, p)
        assert cc.Decrypt(sk, ct, p) == m
        assert cc.Decrypt(sk, cc.EvalFunc(ct, lut), p) == (m * m * m) % p


def test_gpu_public_key_arrays_are_fetched_on_demand_and_key_pairs_work():
    from fhe_amd import binfhe as bf
    cc, sk = context("std128")
    pk = cc.GetPublicKey()
    assert pk._A is None          # the handle of the resident key: nothing fetched yet
    skN = bf.keygen_ring_secret(cc.paramset, cc.method, cc._key_seed)
    A, v = bf.pubkeygen(cc.paramset, cc.method, skN, cc._key_seed)
    assert np.array_equal(pk.A, A) and np.array_equal(pk.v, v)
    # KeyGenPair (boolean-pke has BTKeyGen make the pair; UnitTestFHEWPKE's KeyGenPair path): LARGE_DIM under skN
    cc2 = bf.BinFHEContext()
    cc2.GenerateBinFHEContext(bf.TOY, bf.GINX)
    kp = cc2.KeyGenPair()
    for x in (0, 1, 2, 3):
        assert cc2.Decrypt(kp.secretKey, cc2.Encrypt(kp.publicKey, x, bf.LARGE_DIM)) == x


def test_gpu_device_calls_are_ordered_and_keys_copy():
    """two asynchronous encryptions queued without a synchronise, a gate on their outputs; copy_keys_from carries
    the public key"""
    from fhe_amd import binfhe as bf
    from fhe_amd._lib import check, vp
    cc, sk = context("std128")
    e, L, P = cc.engine, bf.L(), cc.params
    cnt = 8
    x, y = np.arange(cnt, dtype=np.int32) % 2, (np.arange(cnt, dtype=np.int32) // 2) % 2
    bufs = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        d = vp()
        check(L.fhe_hip_alloc(0, max(arr.nbytes, 8), ctypes.byref(d)))
        check(L.fhe_hip_copy_to_device(d, arr.ctypes.data, arr.nbytes))
        bufs.append(d.value)
        return d.value

    dx, dy = dev(x), dev(y)
    a1, b1, a2, b2, ao = (dev(np.zeros((cnt, P.n), np.uint64)) for _ in range(5))
    bo = dev(np.zeros(cnt, np.uint64))
    e.encrypt_pk_device(dx, cnt, SEED + 7, a1, b1, 4, bf.SMALL_DIM)
    e.encrypt_pk_device(dy, cnt, SEED + 8, a2, b2, 4, bf.SMALL_DIM)
    e.eval_gate_device(bf.AND, cnt, a1, b1, a2, b2, ao, bo)
    check(L.fhe_hip_synchronize(0))
    ha, hb = np.zeros((cnt, P.n), np.uint64), np.zeros(cnt, np.uint64)
    check(L.fhe_hip_copy_to_host(ha.ctypes.data, ao, ha.nbytes))
    check(L.fhe_hip_copy_to_host(hb.ctypes.data, bo, cnt * 8))
    for d in bufs:
        L.fhe_hip_free(d)
    wa, wb = e.eval_gate(bf.AND, *e.encrypt_pk(x, SEED + 7, 4, bf.SMALL_DIM), *e.encrypt_pk(y, SEED + 8, 4, bf.SMALL_DIM))
    assert np.array_equal(ha, wa) and np.array_equal(hb, wb)
    assert list(bf.decrypt(cc.paramset, cc.method, sk.s, ha, hb)) == list(x & y)

    e2 = bf.GateEngine(cc.paramset, cc.method, 0)
    e2.copy_keys_from(e)
    for dim in (bf.LARGE_DIM, bf.SMALL_DIM):
        r1, r2 = e.encrypt_pk(x, SEED + 9, 4, dim), e2.encrypt_pk(x, SEED + 9, 4, dim)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    e2.close()


def test_gpu_refusals_on_a_live_context():
    from fhe_amd import binfhe as bf
    P, skN, s, A, v = key("std128")
    e = bf.GateEngine(*SETS["std128"], 0)

    def code(fn):
        with pytest.raises(bf.FheHipError) as err:
            fn()
        return err.value.code

    assert code(lambda: e.encrypt_pk([1], SEED, 4, bf.LARGE_DIM)) == -11      # no public key resident
    assert code(lambda: e.pubkeygen_device(skN[:-1], SEED)) == -2             # wrong N
    e.pubkeygen_device(skN, SEED)
    assert code(lambda: e.encrypt_pk([1], SEED, 4, bf.SMALL_DIM)) == -11      # no switching key
    assert code(lambda: e.encrypt_pk([1], SEED, 1, bf.LARGE_DIM)) == -2
    assert code(lambda: e.encrypt_pk([1], SEED, P.Q + 1, bf.LARGE_DIM)) == -2
    assert code(lambda: e.encrypt_pk([1], SEED, 4, 5)) == -2
    a, b = e.encrypt_pk([], SEED, 4, bf.LARGE_DIM)                            # count = 0: a no-op
    assert a.shape == (0, P.N) and b.shape == (0,)
    a, b = e.encrypt_pk([1], SEED, 4, bf.LARGE_DIM)
    assert list(bf.decrypt(*SETS["std128"], skN, a, b, mod=P.Q)) == [1]
    e.close()
