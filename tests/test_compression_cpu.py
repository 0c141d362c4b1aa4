"""No-GPU checks of the compression and message-encoding layer: the big-integer model against the reference's known answers and FIPS 203,
the division-free decompression identity the kernels use, the digit split / composition of tools_amd.encodings, and every argument error of the
eight entry points of include/psf_mi355x.h (checked before any HIP call).  The device results are compared with the model in
tests/test_gpu_compression.py."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from tests.helpers import fips203_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8


@pytest.fixture(scope="module")
def enc_kats():
    with open(os.path.join(ROOT, "tests", "golden", "ref_encoding_kats.json")) as fh:
        return json.load(fh)


def test_model_reproduces_the_reference_encodings(enc_kats):
    for rec in enc_kats["encode"]:
        for c in rec["cases"]:
            got = M.encode_value(c["value"], rec["base"], rec["q"], rec["n"])
            assert got == c["expect"], (rec["source"], c)
            assert max(i for i, v in enumerate(got) if v) == c["degree"]
    for rec in enc_kats["encode_errors"]:
        assert M.encode_value(rec["value"], rec["base"], rec["q"], rec["n"]) is None, rec["source"]
    rng = random.Random(7)
    for rec in enc_kats["round_trips"]:
        lo, hi = rec.get("value_range", [rec.get("value"), rec.get("value")])
        for v in {lo, hi, *(rng.randint(lo, hi) for _ in range(200))}:
            enc = M.encode_value(v, rec["base"], rec["q"], rec["n"])
            assert M.decode_value(enc, rec["base"], rec["q"]) == v, (rec["source"], v)


def test_compress_1_at_3329_is_the_fips203_message_bit():
    """Compress_1 over Z_3329 is 1 exactly on [833, 2496] (FIPS 203, section 4.2.1: the values closer to q/2 than to 0)"""
    ones = [x for x in range(3329) if M.compress(x, 1, 3329) == 1]
    assert ones == list(range(833, 2497))
    assert M.decompress(1, 1, 3329) == 1665


@pytest.mark.parametrize("q,d", [(257, 4), (3329, 11)])
def test_round_trip_error_bound(q, d):
    """the reference's round-trip bound (lossy_compression_fips203.rs tests): |x - Decompress(Compress(x))| mod+- q <= 2^(ceil(log2 q) - d - 1)"""
    bound = 1 << ((q - 1).bit_length() - d - 1)
    for x in range(q):
        dist = (M.decompress(M.compress(x, d, q), d, q) - x) % q
        assert min(dist, q - dist) <= bound, x


def test_decompress_needs_no_division():
    """the kernels' form: y' = y mod 2^d (a mask), t = floor((y' q + 2^(d-1)) / 2^d) <= q, one conditional subtraction.  Adding 2^d to y adds
    exactly q to the quotient, so y' gives the same residue; and y' <= 2^d - 1 bounds t by q + 1/2 - q/2^d < q + 1."""
    rng = random.Random(11)
    cases = [(q, d, y) for q in (2, 3, 257, 3329) for d in range(1, 13) for y in range(-(1 << (d + 1)), 1 << (d + 1))]
    for _ in range(20000):
        q = rng.randrange(2, 1 << 62)
        d = rng.randrange(1, 64)
        cases.append((q, d, rng.randrange(-(1 << 63), 1 << 63)))
    for q, d, y in cases:
        ym = y & ((1 << d) - 1)
        t = (ym * q + (1 << (d - 1))) >> d
        assert t <= q
        assert (t - q if t == q else t) == M.decompress(y, d, q), (q, d, y)


def test_digit_split_and_composition():
    from tools_amd import encodings as E
    rng = random.Random(5)
    for base in (2, 3, 5, 256, 1 << 40, 10**18, (1 << 63) - 1):
        for n in (1, 16, 17, 64):
            vals = [0, base ** n - 1] + [rng.randrange(base ** n) for _ in range(40)]
            D = E._split(vals, base, n, "test")
            assert D.shape == (len(vals), n) and D.dtype == np.uint64
            for v, row in zip(vals, D):
                ds = M.digits_of(v, base)
                assert [int(x) for x in row] == ds + [0] * (n - len(ds))
            assert E._compose(D, base) == vals


def test_encoding_errors_are_the_references(enc_kats):
    import tools_amd as T
    for rec in enc_kats["encode_errors"]:
        with pytest.raises(T.PsfError) as ei:
            T.encodings.encode_value_in_polynomialringzq(rec["value"], rec["base"], rec["q"], rec["n"])
        assert ei.value.status == ERR_PARAM, rec["source"]
    for rec in enc_kats["decode_errors"]:
        with pytest.raises(T.PsfError) as ei:
            T.encodings.decode_value_from_polynomialringzq(np.zeros(rec["n"], dtype=np.uint64), rec["base"], rec["q"])
        assert ei.value.status == ERR_PARAM, rec["source"]
    with pytest.raises(T.PsfError) as ei:
        T.encodings.encode_values([5], 1 << 63, 257, 4)
    assert ei.value.status == ERR_UNSUPPORTED


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _host_calls(L, x, y):
    """(name, callable(q, p, len, io_bits)) of the eight entry points; p is d or base, io_bits is ignored by the host forms"""
    u64, i64, vp = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_void_p
    X, Y = x.ctypes.data_as(u64), y.ctypes.data_as(i64)
    Yu = y.ctypes.data_as(u64)
    return [
        ("psf_lossy_compress", lambda q, p, n, io, a=X, b=Y: L.psf_lossy_compress(0, C.c_uint64(q), C.c_uint32(p), C.c_size_t(n), a, b)),
        ("psf_lossy_decompress", lambda q, p, n, io, a=Y, b=X: L.psf_lossy_decompress(0, C.c_uint64(q), C.c_uint32(p), C.c_size_t(n), a, b)),
        ("psf_encode_digits", lambda q, p, n, io, a=X, b=Yu: L.psf_encode_digits(0, C.c_uint64(q), C.c_uint64(p), C.c_size_t(n), a, b)),
        ("psf_decode_digits", lambda q, p, n, io, a=X, b=Yu: L.psf_decode_digits(0, C.c_uint64(q), C.c_uint64(p), C.c_size_t(n), a, b)),
        ("psf_lossy_compress_dev", lambda q, p, n, io, a=vp(x.ctypes.data), b=vp(y.ctypes.data):
            L.psf_lossy_compress_dev(0, C.c_uint64(q), C.c_uint32(p), C.c_size_t(n), a, b, C.c_int(io), None)),
        ("psf_lossy_decompress_dev", lambda q, p, n, io, a=vp(y.ctypes.data), b=vp(x.ctypes.data):
            L.psf_lossy_decompress_dev(0, C.c_uint64(q), C.c_uint32(p), C.c_size_t(n), a, b, C.c_int(io), None)),
        ("psf_encode_digits_dev", lambda q, p, n, io, a=vp(x.ctypes.data), b=vp(y.ctypes.data):
            L.psf_encode_digits_dev(0, C.c_uint64(q), C.c_uint64(p), C.c_size_t(n), a, b, C.c_int(io), None)),
        ("psf_decode_digits_dev", lambda q, p, n, io, a=vp(x.ctypes.data), b=vp(y.ctypes.data):
            L.psf_decode_digits_dev(0, C.c_uint64(q), C.c_uint64(p), C.c_size_t(n), a, b, C.c_int(io), None)),
    ]


def test_argument_errors_through_the_abi():
    """every check returns before the first HIP call, so these codes hold on any host"""
    L = _lib()
    x, y = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.int64)
    for name, f in _host_calls(L, x, y):
        lossy = "lossy" in name
        good = 4 if lossy else 2
        assert f(1, good, 8, 64) == ERR_PARAM, name                             # q < 2
        assert f(0, good, 8, 64) == ERR_PARAM, name
        assert f(1 << 62, good, 8, 64) == ERR_UNSUPPORTED, name                 # q >= 2^62
        assert f(3329, good, 0, 64) == OK, name                                 # len = 0: no work, no device needed
        if lossy:
            assert f(3329, 0, 8, 64) == ERR_PARAM, name                         # d < 1 (the reference panics)
            assert f(3329, 64, 8, 64) == ERR_UNSUPPORTED, name                  # d > 63
            assert f(3329, 0, 0, 64) == ERR_PARAM, name                         # checked before len = 0
        else:
            assert f(3329, 1, 8, 64) == ERR_PARAM, name                         # base < 2
            assert f(3329, 0, 8, 64) == ERR_PARAM, name
            assert f(3329, 1 << 63, 8, 64) == ERR_UNSUPPORTED, name             # base >= 2^63
            assert f(3329, (1 << 64) - 1, 8, 64) == ERR_UNSUPPORTED, name
        if name.endswith("_dev"):
            for io in (0, 8, 32, 63, 128, -16):
                assert f(3329, good, 8, io) == ERR_PARAM, (name, io)
            assert f(65537, good, 8, 16) == ERR_UNSUPPORTED, name               # 16-bit words: q <= 2^16
            if lossy:
                assert f(3329, 17, 8, 16) == ERR_UNSUPPORTED, name              # d <= 16
            else:
                assert f(3329, 65537, 8, 16) == ERR_UNSUPPORTED, name           # base <= 2^16
    # NULL pointers with len > 0
    assert L.psf_lossy_compress(0, C.c_uint64(3329), C.c_uint32(4), C.c_size_t(8), None, None) == ERR_PARAM
    assert L.psf_decode_digits_dev(0, C.c_uint64(3329), C.c_uint64(2), C.c_size_t(8), None, C.c_void_p(y.ctypes.data), 64, None) == ERR_PARAM
    assert L.psf_encode_digits_dev(0, C.c_uint64(3329), C.c_uint64(2), C.c_size_t(0), None, None, 16, None) == OK


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def test_valid_call_without_a_device_is_a_hip_error():
    """no CPU fallback: a valid host-form call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    x, y = np.arange(8, dtype=np.uint64), np.zeros(8, dtype=np.int64)
    devices = [-1, 4096] + ([] if _have_device() else [0])
    for dev in devices:
        assert L.psf_lossy_compress(dev, C.c_uint64(3329), C.c_uint32(11), C.c_size_t(8), x.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    y.ctypes.data_as(C.POINTER(C.c_int64))) == ERR_HIP, dev
        assert L.psf_decode_digits(dev, C.c_uint64(3329), C.c_uint64(2), C.c_size_t(8), x.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   y.ctypes.data_as(C.POINTER(C.c_uint64))) == ERR_HIP, dev
    if not _have_device():
        import tools_amd as T
        with pytest.raises(T.PsfError) as ei:
            T.compression.lossy_compress(np.arange(16), 4, 257)
        assert ei.value.status == ERR_HIP
        with pytest.raises(T.PsfError) as ei:
            T.encodings.encode_value_in_polynomialringzq(3, 2, 257, 16)
        assert ei.value.status == ERR_HIP
