"""No-GPU checks of the FIPS 203 byte encodings: the two forms of the model (tests/helpers/byte_encoding_model.py) against each other and against
answers worked by hand, the ML-KEM lengths, the round trips, the modulus flag of ByteDecode_12, and every argument error of the eight entry
points of include/psf_mi355x.h with its precedence (checked before any HIP call).  The device results are compared with the model in
tests/test_gpu_byte_encoding.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import byte_encoding_model as B

OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8


@pytest.mark.parametrize("d", range(1, 64))
def test_the_two_forms_of_the_model_agree(d):
    rng = np.random.default_rng(d)
    for n in (0, 1, 7, 8, 9, 255, 256, 257):
        ys = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64, endpoint=True)
        e_int = B.encode_int(ys.tolist(), d)
        e_np = B.encode_np(ys, d)
        assert len(e_int) == B.nbytes(n, d) == e_np.size
        assert e_np.tobytes() == e_int, (d, n)
        v_int, _ = B.decode_int(e_int, d, n)
        v_np, _ = B.decode_np(e_np, d, n)
        assert v_int == [int(y) & ((1 << d) - 1) for y in ys] == [int(v) for v in v_np], (d, n)
        if (n * d) % 8:
            assert e_int[-1] >> ((n * d) % 8) == 0                          # the unused high bits of the last byte


KATS = [(12, [0x123, 0xABC], "23C1AB"),
        (10, [0x3FF, 0, 0, 0], "FF03000000"),
        (4, [1, 2], "21"),
        (1, [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], "0102"),
        (3, [7, 0, 7], "C701")]


@pytest.mark.parametrize("d,values,expect", KATS)
def test_known_answers(d, values, expect):
    want = bytes.fromhex(expect)
    assert B.encode_int(values, d) == want
    assert B.encode_np(np.array(values, dtype=np.int64), d).tobytes() == want
    assert B.decode_int(want, d, len(values))[0] == values
    assert [int(v) for v in B.decode_np(np.frombuffer(want, dtype=np.uint8), d, len(values))[0]] == values


def test_ml_kem_lengths():
    for d in range(1, 13):
        assert B.nbytes(256, d) == 32 * d
    k, du, dv = 3, 10, 4
    assert k * B.nbytes(256, du) + B.nbytes(256, dv) == 1088             # an ML-KEM-768 ciphertext
    assert B.nbytes(k * 256, du) == k * 320                              # a flat call over k polynomials ...
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << du, size=(k, 256), dtype=np.int64)
    flat = B.encode_np(u, du).tobytes()
    assert flat == b"".join(B.encode_int(row.tolist(), du) for row in u)  # ... is the concatenation of the per-polynomial encodings
    from tools_amd.compression import encoded_size
    assert [encoded_size(256, d) for d in (1, 4, 10, 12)] == [32, 128, 320, 384] and encoded_size(3, 3) == 2 and encoded_size(0, 5) == 0


def test_round_trips():
    rng = np.random.default_rng(1)
    for d in (1, 3, 4, 5, 10, 11, 12, 16, 31, 32, 33, 63):
        for n in (8, 64, 256, 1000):
            ys = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64, endpoint=True)
            back, _ = B.decode_np(B.encode_np(ys, d), d, n)
            assert np.array_equal(back, ys.view(np.uint64) & np.uint64((1 << d) - 1)), (d, n)
            raw = rng.integers(0, 256, size=n * d // 8, dtype=np.uint8)   # n is a multiple of 8: len d is a multiple of 8
            vals, _ = B.decode_np(raw, d, n)
            assert np.array_equal(B.encode_np(vals, d), raw), (d, n)
            assert B.encode_int(B.decode_int(raw.tobytes(), d, n)[0], d) == raw.tobytes()


def test_modulus_flag_of_byte_decode_12():
    q, d = 3329, 12
    canonical = np.array([0, 1, 3328, 1664] * 64, dtype=np.int64)
    for model in (lambda b, n: B.decode_int(b.tobytes(), d, n, q), lambda b, n: B.decode_np(b, d, n, q)):
        vals, flag = model(B.encode_np(canonical, d), canonical.size)
        assert not flag and [int(v) for v in vals] == canonical.tolist()
        for bad in (3329, 3330, 4095):
            ys = canonical.copy()
            ys[77] = bad
            vals, flag = model(B.encode_np(ys, d), ys.size)
            assert flag
            assert [int(v) for v in vals] == [int(y) % q for y in ys]


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _calls(L, vals, data):
    """(name, fused, has_q, dev, f(q, d, len, io_bits, vals_ptr, bytes_ptr)) of the eight entry points"""
    vp = C.c_void_p

    def u(q):
        return C.c_uint64(q)

    return [
        ("psf_byte_encode", False, False, False, lambda q, d, n, io, v, b: L.psf_byte_encode(0, C.c_uint32(d), C.c_size_t(n), vp(v), vp(b))),
        ("psf_byte_decode", False, True, False, lambda q, d, n, io, v, b: L.psf_byte_decode(0, u(q), C.c_uint32(d), C.c_size_t(n), vp(b), vp(v), None)),
        ("psf_compress_encode", True, True, False, lambda q, d, n, io, v, b: L.psf_compress_encode(0, u(q), C.c_uint32(d), C.c_size_t(n), vp(v), vp(b))),
        ("psf_decode_decompress", True, True, False, lambda q, d, n, io, v, b: L.psf_decode_decompress(0, u(q), C.c_uint32(d), C.c_size_t(n), vp(b), vp(v))),
        ("psf_byte_encode_dev", False, False, True,
         lambda q, d, n, io, v, b: L.psf_byte_encode_dev(0, C.c_uint32(d), C.c_size_t(n), vp(v), vp(b), C.c_int(io), None)),
        ("psf_byte_decode_dev", False, True, True,
         lambda q, d, n, io, v, b: L.psf_byte_decode_dev(0, u(q), C.c_uint32(d), C.c_size_t(n), vp(b), vp(v), None, C.c_int(io), None)),
        ("psf_compress_encode_dev", True, True, True,
         lambda q, d, n, io, v, b: L.psf_compress_encode_dev(0, u(q), C.c_uint32(d), C.c_size_t(n), vp(v), vp(b), C.c_int(io), None)),
        ("psf_decode_decompress_dev", True, True, True,
         lambda q, d, n, io, v, b: L.psf_decode_decompress_dev(0, u(q), C.c_uint32(d), C.c_size_t(n), vp(b), vp(v), C.c_int(io), None)),
    ]


def test_argument_errors_through_the_abi():
    """every check returns before the first HIP call, so these codes hold on any host; every PSF_ERR_PARAM outranks every PSF_ERR_UNSUPPORTED"""
    L = _lib()
    vals, data = np.zeros(64, dtype=np.uint64), np.zeros(512, dtype=np.uint8)
    V, D = vals.ctypes.data, data.ctypes.data
    smax = (1 << (8 * C.sizeof(C.c_size_t))) - 1
    for name, fused, has_q, dev, f in _calls(L, vals, data):
        assert f(3329, 0, 8, 64, V, D) == ERR_PARAM, name                      # d < 1
        assert f(3329, 0, 0, 64, V, D) == ERR_PARAM, name                      # ... checked before len = 0
        assert f(3329, 12, 0, 64, V, D) == OK, name                            # len = 0: no work, no device needed
        assert f(3329, 12, 0, 64, None, None) == OK, name
        assert f(3329, 12, 8, 64, None, D) == ERR_PARAM, name                  # NULL with len > 0
        assert f(3329, 12, 8, 64, V, None) == ERR_PARAM, name
        assert f(3329, 12, smax // 8, 64, V, D) == ERR_PARAM, name             # len d overflows size_t
        assert f(3329, 1, smax // 4, 64, V, D) == ERR_PARAM, name              # the value bytes overflow size_t
        assert f(3329, 8, 8, 64, V, V) == ERR_PARAM, name                      # in place
        assert f(3329, 8, 8, 64, V, V + 63) == ERR_PARAM, name                 # the last value byte is the first packed byte
        assert f(3329, 8, 8, 64, V + 7, V) == ERR_PARAM, name                  # the last packed byte is the first value byte
        assert f(3329, 64, 8, 64, V, D) == ERR_UNSUPPORTED, name               # d > 63
        assert f(3329, 255, 8, 64, V, D) == ERR_UNSUPPORTED, name
        assert f(3329, 64, 8, 64, None, D) == ERR_PARAM, name                  # NULL outranks d > 63
        assert f(3329, 64, 8, 64, V, V) == ERR_PARAM, name                     # overlap outranks d > 63
        if has_q:
            assert f(1 << 62, 12, 8, 64, V, D) == ERR_UNSUPPORTED, name        # q >= 2^62
            assert f((1 << 64) - 1, 12, 8, 64, V, D) == ERR_UNSUPPORTED, name
            assert f(1, 12, 8, 64, V, D) == ERR_PARAM, name                    # q = 1
            assert f(1, 64, 8, 64, V, D) == ERR_PARAM, name                    # q = 1 outranks d > 63
            assert f(1 << 62, 0, 8, 64, V, D) == ERR_PARAM, name               # d < 1 outranks q >= 2^62
            assert f(1 << 62, 12, 8, 64, None, D) == ERR_PARAM, name
        if fused:
            assert f(0, 12, 8, 64, V, D) == ERR_PARAM, name                    # q < 2 in the fused forms
            assert f(0, 64, 8, 64, V, D) == ERR_PARAM, name
        if dev:
            for io in (0, 8, 32, 63, 128, -16):
                assert f(3329, 12, 8, io, V, D) == ERR_PARAM, (name, io)
                assert f(3329, 64, 8, io, V, D) == ERR_PARAM, (name, io)       # io_bits outranks d > 63
            assert f(3329, 0, 8, 0, None, None) == ERR_PARAM, name
            assert f(3329, 17, 8, 16, V, D) == ERR_UNSUPPORTED, name           # 16-bit words: d <= 16
            assert f(3329, 16, 0, 16, V, D) == OK, name
            assert f(3329, 17, 8, 16, None, D) == ERR_PARAM, name
            assert f(3329, 8, 8, 16, V, V + 15) == ERR_PARAM, name             # 16 value bytes at 16-bit words
            if has_q:
                assert f(65537, 12, 8, 16, V, D) == ERR_UNSUPPORTED, name      # 16-bit words: q <= 2^16
                assert f(65536, 12, 0, 16, V, D) == OK, name
                assert f(1, 17, 8, 16, V, D) == ERR_PARAM, name
    # q = 0 is the plain ByteDecode_d; it is valid, so without a device it gets as far as the device
    if not _have_device():
        assert L.psf_byte_decode(0, C.c_uint64(0), C.c_uint32(12), C.c_size_t(8), C.c_void_p(D), C.c_void_p(V), None) == ERR_HIP


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def test_valid_call_without_a_device_is_a_hip_error():
    """no CPU fallback: a valid host-form call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    vals, data = np.arange(8, dtype=np.uint64), np.zeros(16, dtype=np.uint8)
    V, D = C.c_void_p(vals.ctypes.data), C.c_void_p(data.ctypes.data)
    flag = C.c_int(5)
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        assert L.psf_byte_encode(dev, C.c_uint32(12), C.c_size_t(8), V, D) == ERR_HIP, dev
        assert L.psf_byte_decode(dev, C.c_uint64(3329), C.c_uint32(12), C.c_size_t(8), D, V, C.byref(flag)) == ERR_HIP, dev
        assert L.psf_compress_encode(dev, C.c_uint64(3329), C.c_uint32(10), C.c_size_t(8), V, D) == ERR_HIP, dev
        assert L.psf_decode_decompress(dev, C.c_uint64(3329), C.c_uint32(10), C.c_size_t(8), D, V) == ERR_HIP, dev
    assert flag.value == 5
    if not _have_device():
        import tools_amd as T
        for call in (lambda: T.compression.byte_encode(np.arange(16), 4), lambda: T.compression.byte_decode(np.zeros(8, dtype=np.uint8), 4, 16),
                     lambda: T.compression.compress_encode(np.arange(16), 4, 257),
                     lambda: T.compression.decode_decompress(np.zeros(8, dtype=np.uint8), 4, 257, 16)):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP
