"""The host-pointer forms with PADDED host strides on the MI355X: the one staging path the Python wrappers never reach, because they pack their rows.
Through raw ctypes, count = 3, the smallest set of each scheme (ML-DSA-44, SLH-DSA-SHAKE-128f) and SHAKE256: every call is made once with packed rows and
once with every strided argument at len + 3 (len + 5 for messages) inside a guard-filled array, for message lengths 0 (a NULL pointer), 1 and 33, and
for sign and verify also under one shared key (stride 0).  The outputs of the two calls must be byte-identical and no guard byte may change.  The keys
and signatures the verifications read are made once per module by the packed host forms, which the other GPU tests compare with the models."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNT, PAD, GUARD = 3, 16, 0xA5
MSG_LENS = (0, 1, 33)
MLDSA, SLH = "ML-DSA-44", "SLH-DSA-SHAKE-128f"
MAX_ROUNDS = 64                                                          # ML-DSA-44: a signing attempt succeeds with probability about 1 / 4.25


class Laid:
    """`count` rows of `length` bytes at stride length + extra inside an array of guard bytes, PAD more of them on either side; length 0: NULL."""

    def __init__(self, count, length, extra=0, rows=None):
        self.count, self.length, self.stride = count, length, length + extra
        self.buf = np.full(2 * PAD + count * self.stride, GUARD, np.uint8)
        self.mask = np.zeros(self.buf.size, bool)
        for c in range(count):
            self.mask[PAD + c * self.stride:PAD + c * self.stride + length] = True
        if rows is not None:
            self.buf[self.mask] = np.asarray(rows, np.uint8).reshape(-1)
        self.before = self.buf.copy()

    @property
    def ptr(self):
        return self.buf.ctypes.data + PAD if self.length else None

    def rows(self):
        return self.buf[self.mask].reshape(self.count, self.length).copy()

    def guards_intact(self):
        return bool((self.buf[~self.mask] == GUARD).all())

    def unchanged(self):
        return bool((self.buf == self.before).all())


def _rand(rng, count, length):
    return rng.integers(0, 256, (count, length), dtype=np.uint8)


def _ok(status, where):
    assert status == 0, (where, status)


def _intact(*laid):
    for x in laid:
        assert x.guards_intact(), "a guard byte changed"


@pytest.fixture(scope="module")
def libs():
    import tools_amd
    from tools_amd import fips203, fips204, mldsa, slhdsa
    return {"mldsa": (mldsa._lib(), mldsa._param(MLDSA), mldsa.sizes(MLDSA)), "slh": (slhdsa._lib(), slhdsa._param(SLH), slhdsa.sizes(SLH)),
            "fips204": fips204._lib(), "keccak": (tools_amd._ffi.lib(), fips203.SHAKE256)}


# ---- the calls: every buffer a Laid, `shared` one key for all (stride 0) ---------------------------------------------------------------------------------
def mldsa_sign(libs, sk, msg, rnd, shared, with_rounds=True):
    L, param, sz = libs["mldsa"]
    sig, rounds = Laid(COUNT, sz["sig"]), Laid(COUNT, 4)
    _ok(L.psf_mldsa_sign(0, param, COUNT, sk.ptr, 0 if shared else sk.stride, msg.ptr, msg.length, msg.stride, 0, rnd.ptr, sig.ptr, MAX_ROUNDS,
                         rounds.ptr if with_rounds else None), "psf_mldsa_sign")
    _intact(sig, rounds)
    assert sk.unchanged() and msg.unchanged() and rnd.unchanged()
    return sig.rows(), rounds.rows() if with_rounds else None


def mldsa_verify(libs, pk, msg, sig, shared, with_why=True):
    L, param, _ = libs["mldsa"]
    ok, why = Laid(COUNT, 1), Laid(COUNT, 1)
    _ok(L.psf_mldsa_verify(0, param, COUNT, pk.ptr, 0 if shared else pk.stride, msg.ptr, msg.length, msg.stride, 0, sig.ptr, ok.ptr, why.ptr if with_why else None),
        "psf_mldsa_verify")
    _intact(ok, why)
    assert pk.unchanged() and msg.unchanged() and sig.unchanged()
    return ok.rows(), why.rows() if with_why else None


def slh_sign(libs, sk, msg, addrnd, shared):
    L, param, sz = libs["slh"]
    sig = Laid(COUNT, sz["sig"])
    _ok(L.psf_slhdsa_sign(0, param, COUNT, sk.ptr, 0 if shared else sk.stride, msg.ptr, msg.length, msg.stride, addrnd.ptr, sig.ptr), "psf_slhdsa_sign")
    _intact(sig)
    assert sk.unchanged() and msg.unchanged() and addrnd.unchanged()
    return sig.rows()


def slh_verify(libs, pk, msg, sig, shared):
    L, param, _ = libs["slh"]
    ok = Laid(COUNT, 1)
    _ok(L.psf_slhdsa_verify(0, param, COUNT, pk.ptr, 0 if shared else pk.stride, msg.ptr, msg.length, msg.stride, sig.ptr, ok.ptr), "psf_slhdsa_verify")
    _intact(ok)
    assert pk.unchanged() and msg.unchanged() and sig.unchanged()
    return ok.rows()


# ---- keys, made once -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mldsa_keys(libs):
    L, param, sz = libs["mldsa"]
    xi, pk, sk = _rand(np.random.default_rng(204), COUNT, 32), np.empty((COUNT, sz["pk"]), np.uint8), np.empty((COUNT, sz["sk"]), np.uint8)
    _ok(L.psf_mldsa_keygen(0, param, COUNT, xi.ctypes.data, pk.ctypes.data, sk.ctypes.data), "psf_mldsa_keygen")
    return pk, sk


@pytest.fixture(scope="module")
def slh_keys(libs):
    L, param, sz = libs["slh"]
    n = sz["pk"] // 2
    seeds = [_rand(np.random.default_rng(205 + i), COUNT, n) for i in range(3)]
    pk, sk = np.empty((COUNT, sz["pk"]), np.uint8), np.empty((COUNT, sz["sk"]), np.uint8)
    _ok(L.psf_slhdsa_keygen(0, param, COUNT, *[s.ctypes.data for s in seeds], pk.ctypes.data, sk.ctypes.data), "psf_slhdsa_keygen")
    return pk, sk


def _keys(keys, shared):
    """(rows, count) of the public and the secret keys a call reads"""
    return (keys[0][:1], keys[1][:1], 1) if shared else (keys[0], keys[1], COUNT)


# ---- sign and verify -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["key_per_instance", "shared_key"])
@pytest.mark.parametrize("msg_len", MSG_LENS)
def test_mldsa_sign_and_verify_with_padded_rows(libs, mldsa_keys, msg_len, shared):
    rng = np.random.default_rng(1000 + msg_len)
    pk, sk, keys = _keys(mldsa_keys, shared)
    msg, rnd = _rand(rng, COUNT, msg_len), _rand(rng, COUNT, 32)
    sig_p, rounds_p = mldsa_sign(libs, Laid(keys, sk.shape[1], 0, sk), Laid(COUNT, msg_len, 0, msg), Laid(COUNT, 32, 0, rnd), shared)
    sig_s, rounds_s = mldsa_sign(libs, Laid(keys, sk.shape[1], 3, sk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, 32, 0, rnd), shared)
    assert (sig_p == sig_s).all() and (rounds_p == rounds_s).all()
    assert (rounds_p.view(np.uint32) >= 1).all()
    sig_n, none = mldsa_sign(libs, Laid(keys, sk.shape[1], 3, sk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, 32, 0, rnd), shared, with_rounds=False)
    assert none is None and (sig_n == sig_p).all()
    bad = sig_p.copy()
    bad[1, 40] ^= 1                                                        # instance 1 must fail, in both layouts alike
    for sig, want in ((sig_p, [1, 1, 1]), (bad, [1, 0, 1])):
        ok_p, why_p = mldsa_verify(libs, Laid(keys, pk.shape[1], 0, pk), Laid(COUNT, msg_len, 0, msg), Laid(COUNT, sig.shape[1], 0, sig), shared)
        ok_s, why_s = mldsa_verify(libs, Laid(keys, pk.shape[1], 3, pk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, sig.shape[1], 0, sig), shared)
        assert ok_p.reshape(-1).tolist() == want and (ok_p == ok_s).all() and (why_p == why_s).all()
        ok_n, none = mldsa_verify(libs, Laid(keys, pk.shape[1], 3, pk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, sig.shape[1], 0, sig), shared, with_why=False)
        assert none is None and (ok_n == ok_p).all()


@pytest.mark.parametrize("shared", [False, True], ids=["key_per_instance", "shared_key"])
@pytest.mark.parametrize("msg_len", MSG_LENS)
def test_slhdsa_sign_and_verify_with_padded_rows(libs, slh_keys, msg_len, shared):
    rng = np.random.default_rng(2000 + msg_len)
    pk, sk, keys = _keys(slh_keys, shared)
    n = pk.shape[1] // 2
    msg, addrnd = _rand(rng, COUNT, msg_len), _rand(rng, COUNT, n)
    sig_p = slh_sign(libs, Laid(keys, sk.shape[1], 0, sk), Laid(COUNT, msg_len, 0, msg), Laid(COUNT, n, 0, addrnd), shared)
    sig_s = slh_sign(libs, Laid(keys, sk.shape[1], 3, sk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, n, 0, addrnd), shared)
    assert (sig_p == sig_s).all()
    det_p = slh_sign(libs, Laid(keys, sk.shape[1], 0, sk), Laid(COUNT, msg_len, 0, msg), Laid(COUNT, 0), shared)      # addrnd NULL: the deterministic variant
    det_s = slh_sign(libs, Laid(keys, sk.shape[1], 3, sk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, 0), shared)
    assert (det_p == det_s).all() and not (det_p == sig_p).all()
    bad = sig_p.copy()
    bad[1, n + 3] ^= 1
    for sig, want in ((sig_p, [1, 1, 1]), (bad, [1, 0, 1])):
        ok_p = slh_verify(libs, Laid(keys, pk.shape[1], 0, pk), Laid(COUNT, msg_len, 0, msg), Laid(COUNT, sig.shape[1], 0, sig), shared)
        ok_s = slh_verify(libs, Laid(keys, pk.shape[1], 3, pk), Laid(COUNT, msg_len, 5, msg), Laid(COUNT, sig.shape[1], 0, sig), shared)
        assert ok_p.reshape(-1).tolist() == want and (ok_p == ok_s).all()


# ---- SHAKE256 and the FIPS 204 stages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_len", MSG_LENS + (136, 137))
def test_keccak_with_padded_rows_in_and_out(libs, in_len):
    """in_stride = in_len + 5 and out_stride = out_len + 3: the one call whose OUTPUT rows are strided, so the guard bytes between them count."""
    L, func = libs["keccak"]
    msg = _rand(np.random.default_rng(3000 + in_len), COUNT, in_len)
    digests = []
    for in_extra, out_extra in ((0, 0), (5, 3), (5, 0), (0, 3)):
        src, dst = Laid(COUNT, in_len, in_extra, msg), Laid(COUNT, 50, out_extra)
        _ok(L.psf_keccak(0, func, COUNT, src.ptr, in_len, src.stride, dst.ptr, 50, dst.stride), "psf_keccak")
        _intact(dst)
        assert src.unchanged()
        digests.append(dst.rows())
    assert all((d == digests[0]).all() for d in digests[1:])
    import hashlib
    assert [bytes(r) for r in digests[0]] == [hashlib.shake_256(bytes(m)).digest(50) for m in msg]


def _stage(call, seed_rows, out_words):
    outs = []
    for extra in (0, 3):
        seed, out = Laid(COUNT, seed_rows.shape[1], extra, seed_rows), Laid(1, out_words * 8)
        call(seed, out)
        _intact(out)
        assert seed.unchanged()
        outs.append(out.rows())
    assert (outs[0] == outs[1]).all() and outs[0].any()


def test_sample_ntt_fips204_with_padded_seeds(libs):
    L, rng = libs["fips204"], np.random.default_rng(4000)
    _stage(lambda s, o: _ok(L.psf_sample_ntt_fips204(0, COUNT, 0, 0, s.ptr, s.stride, o.ptr), "psf_sample_ntt_fips204"), _rand(rng, COUNT, 34), COUNT * 256)
    _stage(lambda s, o: _ok(L.psf_sample_ntt_fips204(0, COUNT, 2, 3, s.ptr, s.stride, o.ptr), "psf_sample_ntt_fips204"), _rand(rng, COUNT, 32), COUNT * 6 * 256)


def test_sample_bounded_fips204_with_padded_seeds(libs):
    L, rng = libs["fips204"], np.random.default_rng(4001)
    for eta in (2, 4):
        _stage(lambda s, o: _ok(L.psf_sample_bounded_fips204(0, COUNT, eta, s.ptr, s.stride, 1, 2, o.ptr), "psf_sample_bounded_fips204"), _rand(rng, COUNT, 64),
               COUNT * 2 * 256)


def test_sample_in_ball_fips204_with_padded_rows(libs):
    L, rng = libs["fips204"], np.random.default_rng(4002)
    for length in (1, 32, 64):
        _stage(lambda s, o: _ok(L.psf_sample_in_ball_fips204(0, COUNT, 39, s.ptr, s.length, s.stride, o.ptr), "psf_sample_in_ball_fips204"), _rand(rng, COUNT, length),
               COUNT * 256)


def test_the_laid_rows_helper():
    """The helper itself: rows land at the stride, the guards around and between them are seen, a changed guard is noticed."""
    rows = np.arange(6, dtype=np.uint8).reshape(3, 2)
    x = Laid(3, 2, 3, rows)
    assert x.stride == 5 and x.buf.size == 2 * PAD + 15 and (x.rows() == rows).all() and x.guards_intact() and x.unchanged()
    assert x.buf[PAD:PAD + 7].tolist() == [0, 1, GUARD, GUARD, GUARD, 2, 3]
    x.buf[PAD + 2] ^= 1
    assert not x.guards_intact() and not x.unchanged()
    assert Laid(3, 0, 5).ptr is None and Laid(3, 0, 5).stride == 5
