"""No-GPU checks of the sample fills: the centred-binomial slot rule (exhaustively per field, and positions worked by hand), the vectorised
model against the definition over oracle.philox, every argument error of the six entry points of include/psf_mi355x.h in its stated order
(checked before any HIP call), and the regenerated FFI.  The device results are compared with the oracle and the model in
tests/test_gpu_sample_fill.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import sample_fill_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8


@pytest.mark.parametrize("eta", [1, 2, 3, 4])
def test_slot_rule_gives_the_binomial_counts(eta):
    """over all 2^(2 eta) fields, popcount(lo) - popcount(hi) = v occurs C(2 eta, eta + v) times: the convolution of two Binomial(eta, 1/2) laws"""
    hist = {}
    for f in range(1 << (2 * eta)):
        v = M.cbd_value(f, eta)
        hist[v] = hist.get(v, 0) + 1
    assert hist == {v: math.comb(2 * eta, eta + v) for v in range(-eta, eta + 1)}
    conv = {}
    for x in range(eta + 1):
        for y in range(eta + 1):
            conv[x - y] = conv.get(x - y, 0) + math.comb(eta, x) * math.comb(eta, y)
    assert hist == conv


def test_positions_worked_by_hand_for_eta_3():
    """eta = 3: 5 slots per word, 20 coefficients per block"""
    assert M.cbd_position(4, 3) == (0, 0, 4)       # word x, slot 4
    assert M.cbd_position(5, 3) == (0, 1, 0)       # word y, slot 0
    assert M.cbd_position(19, 3) == (0, 3, 4)      # word w, slot 4
    assert M.cbd_position(20, 3) == (1, 0, 0)      # block 1, word x, slot 0
    from oracle import oracle as O
    seed, tag, idx = 0x1234567890ABCDEF, 77, (5 << 32) | 9
    w = O.philox(seed, 0, 9, 0, 77 | (5 << 8))
    f = (w[1] >> 0) & 63
    assert M.cbd_coeff(seed, tag, idx, 5, 3) == bin(f & 7).count("1") - bin(f >> 3).count("1")
    f = (w[3] >> 24) & 63
    assert M.cbd_coeff(seed, tag, idx, 19, 3) == bin(f & 7).count("1") - bin(f >> 3).count("1")
    assert [M.cbd_position(i, 16) for i in (0, 3, 4)] == [(0, 0, 0), (0, 3, 0), (1, 0, 0)]
    assert [M.cbd_position(i, 2) for i in (7, 8, 31, 32)] == [(0, 0, 7), (0, 1, 0), (0, 3, 7), (1, 0, 0)]


def test_numpy_philox_and_vectorised_model_equal_the_definition():
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    for _ in range(50):
        seed = int(rng.integers(0, 1 << 63)) * 2 + 1
        c = [int(v) for v in rng.integers(0, 1 << 32, size=4)]
        assert [int(x) for x in M.philox_np(seed, *c)] == O.philox(seed, *c)
    for eta, n in [(1, 70), (2, 33), (3, 41), (5, 13), (8, 9), (16, 5)]:
        first = (1 << 32) - 2
        got = M.cbd_fill(99, 200, first, 4, n, eta)
        want = [[M.cbd_coeff(99, 200, first + c, i, eta) for i in range(n)] for c in range(4)]
        assert got.tolist() == want, eta
        assert np.abs(got).max() <= eta


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _forms(L, cen_ptr=None):
    """name -> f(tag, io, first, count, n, out, q=, eta=, s=, center=, centers=): the six entry points with valid defaults"""
    vp = C.c_void_p

    def head(tag, first, count, n):
        return (0, C.c_uint64(5), C.c_uint32(tag & 0xFFFFFFFF), C.c_uint64(first), C.c_size_t(count), C.c_size_t(n))

    def uni_d(tag, io, first, count, n, out, q=3329, **_):
        return L.psf_sample_uniform_dev(*head(tag, first, count, n), C.c_uint64(q), vp(out), C.c_int(io), None)

    def cbd_d(tag, io, first, count, n, out, eta=2, **_):
        return L.psf_sample_cbd_dev(*head(tag, first, count, n), C.c_uint32(eta), vp(out), C.c_int(io), None)

    def gau_d(tag, io, first, count, n, out, s=8.0, center=0.0, centers=None, **_):
        return L.psf_sample_discrete_gauss_dev(*head(tag, first, count, n), C.c_double(center), vp(centers), C.c_double(s), vp(out), None, C.c_int(io), None)

    def uni_h(tag, io, first, count, n, out, q=3329, **_):
        return L.psf_sample_uniform(*head(tag, first, count, n), C.c_uint64(q), vp(out))

    def cbd_h(tag, io, first, count, n, out, eta=2, **_):
        return L.psf_sample_cbd(*head(tag, first, count, n), C.c_uint32(eta), vp(out))

    def gau_h(tag, io, first, count, n, out, s=8.0, center=0.0, centers=None, **_):
        return L.psf_sample_discrete_gauss(*head(tag, first, count, n), C.c_double(center), vp(centers), C.c_double(s), vp(out))

    return {"uniform_dev": uni_d, "cbd_dev": cbd_d, "gauss_dev": gau_d, "uniform": uni_h, "cbd": cbd_h, "gauss": gau_h}


def test_argument_errors_through_the_abi():
    """every check returns before the first HIP call, so these codes hold on any host; the order is the header's"""
    L = _lib()
    buf = np.zeros(64, dtype=np.uint64)
    cen = np.zeros(64, dtype=np.float64)
    P, CP = buf.ctypes.data, cen.ctypes.data
    smax = (1 << (8 * C.sizeof(C.c_size_t))) - 1
    bad = dict(q=1, eta=0, s=-1.0)                                          # a later PARAM error, to show what outranks it
    uns = dict(q=1 << 62, eta=17, s=2.0 ** 29)                              # an UNSUPPORTED one
    for name, f in _forms(L).items():
        dev = name.endswith("_dev")
        for tag in (0, 1, 12, 63, 256, 1 << 31, 0xFFFFFFFF):
            assert f(tag, 64, 0, 2, 8, P) == ERR_PARAM, (name, tag)
            assert f(tag, 7, 0, 2, 0, None, **bad) == ERR_PARAM, (name, tag)
            assert f(tag, 64, 0, 0, 8, P) == ERR_PARAM, (name, tag)         # ... checked before count = 0
        for tag in (64, 255):
            assert f(tag, 64, 0, 0, 8, P) == OK, (name, tag)                # count = 0: no work, no device needed
            assert f(tag, 64, 0, 0, 8, None) == OK, (name, tag)
        assert f(64, 64, 1 << 56, 0, 8, None) == OK, name
        if dev:
            for io in (0, 8, 32, 63, 128, -16):
                assert f(64, io, 0, 2, 8, P) == ERR_PARAM, (name, io)
                assert f(64, io, 0, 2, 8, P, **uns) == ERR_PARAM, (name, io)
            assert f(64, 16, 0, 0, 8, P) == OK, name
        assert f(64, 64, 0, 2, 0, P) == ERR_PARAM, name                     # n = 0
        assert f(64, 64, 0, 2, 1 << 32, P) == ERR_PARAM, name               # n >= 2^32
        assert f(64, 64, 0, 0, 1 << 32, P) == ERR_PARAM, name
        assert f(64, 64, (1 << 56) - 1, 2, 8, P) == ERR_PARAM, name         # first_index + count > 2^56
        assert f(64, 64, (1 << 56) + 1, 0, 8, P) == ERR_PARAM, name
        assert f(64, 64, (1 << 64) - 1, 2, 8, P) == ERR_PARAM, name
        assert f(64, 64, 0, smax // 8, 8, P) == ERR_PARAM, name             # the byte count overflows size_t
        assert f(64, 64, 0, 1 << 40, (1 << 32) - 1, P) == ERR_PARAM, name
        assert f(64, 64, 0, 2, 8, None) == ERR_PARAM, name                  # NULL with count > 0
        assert f(64, 64, 0, 2, 8, None, **uns) == ERR_PARAM, name
        assert f(64, 64, 0, 2, 0, None) == ERR_PARAM, name
    F = _forms(L)
    for sfx in ("_dev", ""):
        u, c, g = F["uniform" + sfx], F["cbd" + sfx], F["gauss" + sfx]
        for q in (0, 1):
            assert u(64, 64, 0, 2, 8, P, q=q) == ERR_PARAM
        for q in (1 << 62, (1 << 64) - 1):
            assert u(64, 64, 0, 2, 8, P, q=q) == ERR_UNSUPPORTED
            assert u(64, 64, 0, 2, 8, None, q=q) == ERR_PARAM               # NULL outranks q >= 2^62
        assert u(64, 64, 0, 0, 8, P, q=(1 << 62) - 57) == OK
        assert c(64, 64, 0, 2, 8, P, eta=0) == ERR_PARAM
        for eta in (17, 32, 0xFFFFFFFF):
            assert c(64, 64, 0, 2, 8, P, eta=eta) == ERR_UNSUPPORTED
        assert c(64, 64, 0, 0, 8, P, eta=16) == OK
        for s in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert g(64, 64, 0, 2, 8, P, s=s) == ERR_PARAM, s
            assert g(64, 64, 0, 2, 8, P, s=s, center=float("nan")) == ERR_PARAM, s
        for cc in (float("nan"), float("inf"), -float("inf")):
            assert g(64, 64, 0, 2, 8, P, center=cc) == ERR_PARAM, cc
            assert g(64, 64, 0, 2, 8, P, center=cc, s=2.0 ** 29) == ERR_PARAM, cc     # PARAM outranks s > 2^28
            assert g(64, 64, 0, 0, 8, P, center=cc, centers=CP) == OK, cc            # ignored with per-element centres
        assert g(64, 64, 0, 2, 8, P, s=2.0 ** 28 * 1.0000001) == ERR_UNSUPPORTED
        assert g(64, 64, 0, 0, 8, P, s=2.0 ** 28) == OK
    ud, cd, gd = F["uniform_dev"], F["cbd_dev"], F["gauss_dev"]
    assert ud(64, 16, 0, 2, 8, P, q=65537) == ERR_UNSUPPORTED              # 16-bit words: q <= 2^16
    assert ud(64, 16, 0, 0, 8, P, q=65536) == OK
    assert ud(64, 16, 0, 2, 8, P, q=1) == ERR_PARAM
    assert cd(64, 16, 0, 0, 8, P, eta=16) == OK
    assert gd(64, 16, 0, 2, 8, P, centers=CP) == ERR_UNSUPPORTED           # 16-bit words: a shared centre only
    assert gd(64, 16, 0, 0, 8, P, s=5461.0) == OK                          # 6 s + 1 = 32767: |c| + 6 s + 1 < 2^15 holds up to |c| < 1
    assert gd(64, 16, 0, 2, 8, P, s=5461.0, center=1.0) == ERR_UNSUPPORTED
    assert gd(64, 16, 0, 2, 8, P, s=5461.0, center=-1.0) == ERR_UNSUPPORTED
    assert gd(64, 16, 0, 2, 8, P, s=5462.0) == ERR_UNSUPPORTED
    assert gd(64, 16, 0, 0, 8, P, s=5461.0, center=0.5) == OK
    assert gd(64, 16, 0, 2, 8, P, s=8.0, center=-32720.0) == ERR_UNSUPPORTED
    assert gd(64, 16, 0, 2, 8, P, s=-8.0, center=-32720.0) == ERR_PARAM
    assert (buf == 0).all()


def test_valid_call_without_a_device_is_a_hip_error():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    buf = np.full(16, 7, dtype=np.uint64)
    P = C.c_void_p(buf.ctypes.data)
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        head = (dev, C.c_uint64(1), C.c_uint32(64), C.c_uint64(0), C.c_size_t(2), C.c_size_t(8))
        assert L.psf_sample_uniform(*head, C.c_uint64(3329), P) == ERR_HIP, dev
        assert L.psf_sample_cbd(*head, C.c_uint32(2), P) == ERR_HIP, dev
        assert L.psf_sample_discrete_gauss(*head, C.c_double(0.0), None, C.c_double(8.0), P) == ERR_HIP, dev
    assert (buf == 7).all()
    if not _have_device():
        import tools_amd as T
        for call in (lambda: T.sample.sample_uniform(2, 8, 3329, seed=1), lambda: T.sample.sample_cbd(2, 8, 2, seed=1),
                     lambda: T.sample.sample_discrete_gauss(2, 8, 8.0, seed=1)):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP


def test_header_and_ffi_agree():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"])
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for fn in ("psf_sample_uniform", "psf_sample_cbd", "psf_sample_discrete_gauss"):
        assert f"pub fn {fn}(" in ffi and f"pub fn {fn}_dev(" in ffi, fn
        assert hasattr(_lib(), fn) and hasattr(_lib(), fn + "_dev")
