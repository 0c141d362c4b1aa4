"""LossyCompressionFIPS203 (compression/lossy_compression_fips203.rs) for PolynomialRingZq and MatPolynomialRingZq through the C ABI.

A polynomial is the last axis of an array (..., n) -- one polynomial (n,), a matrix of polynomials (rows, cols, n), any batch of them -- and every
coefficient is mapped on its own, so one call covers all of them.  Compress_d / Decompress_d run on the device (include/psf_mi355x.h)."""
import ctypes as C

import numpy as np

from ._ffi import check, lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


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
