"""LossyCompressionFIPS203 (compression/lossy_compression_fips203.rs) for PolynomialRingZq and MatPolynomialRingZq through the C ABI.

A polynomial is the last axis of an array (..., n) -- one polynomial (n,), a matrix of polynomials (rows, cols, n), any batch of them -- and every
coefficient is mapped on its own, so one call covers all of them.  Compress_d / Decompress_d run on the device (include/psf_mi355x.h), and so do
the byte encodings of FIPS 203 (ByteEncode_d / ByteDecode_d, Algorithms 5 / 6) over the flattened array, alone or fused with them."""
import ctypes as C

import numpy as np

from ._ffi import _p, check, lib


def _residues(x, q):
    """x as uint64 words that are congruent to x mod q: signed arrays are reduced here, unsigned ones on the device"""
    x = np.asarray(x)
    if x.dtype.kind == "i":
        return np.ascontiguousarray(np.mod(x.astype(np.int64), np.int64(q)).astype(np.uint64))
    return np.ascontiguousarray(x, dtype=np.uint64)


def lossy_compress(x, d, q, device=0):
    """Compress_d (lossy_compression_fips203.rs:89-112): y = floor((x 2^d + floor(q/2)) / q) mod 2^d per coefficient, x read mod q.
    Returns int64 of x's shape."""
    x = _residues(x, q)
    y = np.empty(x.shape, dtype=np.int64)
    check(lib().psf_lossy_compress(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(x.size), _p(x, C.c_uint64), _p(y, C.c_int64)),
          "lossy_compress")
    return y


def lossy_decompress(y, d, q, device=0):
    """Decompress_d (lossy_compression_fips203.rs:143-172): x = floor((y q + 2^(d-1)) / 2^d) mod q per coefficient, y any int64.
    Returns the least non-negative residues (uint64) of y's shape."""
    y = np.ascontiguousarray(y, dtype=np.int64)
    x = np.empty(y.shape, dtype=np.uint64)
    check(lib().psf_lossy_decompress(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(y.size), _p(y, C.c_int64), _p(x, C.c_uint64)),
          "lossy_decompress")
    return x


def lossy_compress_dev(d_x, d_y, q, d, length, io_bits=64, device=0, stream=None):
    """psf_lossy_compress_dev on device buffers (raw pointers, e.g. torch `data_ptr()`), in `stream`, nothing allocated.
    io_bits 64: x uint64 -> y int64; io_bits 16: uint16 -> uint16 (q <= 2^16, d <= 16)."""
    check(lib().psf_lossy_compress_dev(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), C.c_void_p(d_x), C.c_void_p(d_y),
                                       C.c_int(io_bits), C.c_void_p(stream or 0)), "lossy_compress_dev")


def lossy_decompress_dev(d_y, d_x, q, d, length, io_bits=64, device=0, stream=None):
    """psf_lossy_decompress_dev: y int64 -> x uint64 in [0, q) (io_bits 64), or uint16 -> uint16 (io_bits 16, y read mod 2^d)."""
    check(lib().psf_lossy_decompress_dev(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), C.c_void_p(d_y), C.c_void_p(d_x),
                                         C.c_int(io_bits), C.c_void_p(stream or 0)), "lossy_decompress_dev")


def encoded_size(length, d):
    """ceil(length d / 8): the bytes of ByteEncode_d over `length` values (32 d per polynomial at n = 256)"""
    return (int(length) * int(d) + 7) // 8


def byte_encode(y, d, device=0):
    """ByteEncode_d (FIPS 203 Algorithm 5, any length): the flat array y, each value read mod 2^d, as ceil(len d / 8) bytes -- bit j of value i
    is stream bit i d + j, least significant bit of a byte first.  Returns uint8 (nbytes,)."""
    y = np.ascontiguousarray(y, dtype=np.int64)
    out = np.empty(encoded_size(y.size, d), dtype=np.uint8)
    check(lib().psf_byte_encode(C.c_int(device), C.c_uint32(d), C.c_size_t(y.size), _p(y, C.c_int64), _p(out, C.c_uint8)), "byte_encode")
    return out


def byte_decode(data, d, length, q=0, device=0):
    """ByteDecode_d (Algorithm 6): `length` values from ceil(length d / 8) bytes.  q = 0: the values as they are, in [0, 2^d); q >= 2: their least
    non-negative residues mod q.  Returns (y int64 (length,), noncanonical): noncanonical is True when q is set and some value was >= q."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if data.size != encoded_size(length, d):
        raise ValueError(f"byte_decode: {data.size} bytes for {length} values of {d} bits")
    y = np.empty(length, dtype=np.int64)
    flag = C.c_int(0)
    check(lib().psf_byte_decode(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), _p(data, C.c_uint8), _p(y, C.c_int64),
                                C.byref(flag)), "byte_decode")
    return y, bool(flag.value)


def compress_encode(x, d, q, device=0):
    """ByteEncode_d(Compress_d(x)) in one pass over the flat array x (read mod q).  Returns uint8 (ceil(len d / 8),)."""
    x = _residues(x, q)
    out = np.empty(encoded_size(x.size, d), dtype=np.uint8)
    check(lib().psf_compress_encode(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(x.size), _p(x, C.c_uint64), _p(out, C.c_uint8)),
          "compress_encode")
    return out


def decode_decompress(data, d, q, length, device=0):
    """Decompress_d(ByteDecode_d(data)) in one pass: `length` least non-negative residues (uint64)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if data.size != encoded_size(length, d):
        raise ValueError(f"decode_decompress: {data.size} bytes for {length} values of {d} bits")
    x = np.empty(length, dtype=np.uint64)
    check(lib().psf_decode_decompress(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), _p(data, C.c_uint8), _p(x, C.c_uint64)),
          "decode_decompress")
    return x


def byte_encode_dev(d_y, d_bytes, d, length, io_bits=64, device=0, stream=None):
    """psf_byte_encode_dev on device buffers (raw pointers), in `stream`, nothing allocated: int64 (io_bits 64) or uint16 (io_bits 16, d <= 16)
    values -> ceil(length d / 8) bytes.  No in-place form."""
    check(lib().psf_byte_encode_dev(C.c_int(device), C.c_uint32(d), C.c_size_t(length), C.c_void_p(d_y), C.c_void_p(d_bytes), C.c_int(io_bits),
                                    C.c_void_p(stream or 0)), "byte_encode_dev")


def byte_decode_dev(d_bytes, d_y, q, d, length, d_noncanonical=None, io_bits=64, device=0, stream=None):
    """psf_byte_decode_dev: bytes -> values in [0, 2^d) (q = 0) or [0, q) (q >= 2).  d_noncanonical: a device int (or None) that is OR-ed with 1
    when q is set and some value was >= q; never cleared here."""
    check(lib().psf_byte_decode_dev(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), C.c_void_p(d_bytes), C.c_void_p(d_y),
                                    C.c_void_p(d_noncanonical or 0), C.c_int(io_bits), C.c_void_p(stream or 0)), "byte_decode_dev")


def compress_encode_dev(d_x, d_bytes, q, d, length, io_bits=64, device=0, stream=None):
    """psf_compress_encode_dev: x uint64 / uint16 -> the bytes of ByteEncode_d(Compress_d(x)), one pass."""
    check(lib().psf_compress_encode_dev(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), C.c_void_p(d_x), C.c_void_p(d_bytes),
                                        C.c_int(io_bits), C.c_void_p(stream or 0)), "compress_encode_dev")


def decode_decompress_dev(d_bytes, d_x, q, d, length, io_bits=64, device=0, stream=None):
    """psf_decode_decompress_dev: bytes -> Decompress_d of each value, in [0, q), uint64 / uint16, one pass."""
    check(lib().psf_decode_decompress_dev(C.c_int(device), C.c_uint64(q), C.c_uint32(d), C.c_size_t(length), C.c_void_p(d_bytes), C.c_void_p(d_x),
                                          C.c_int(io_bits), C.c_void_p(stream or 0)), "decode_decompress_dev")
