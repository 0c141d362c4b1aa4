"""sample_uniform / sample_binomial (p = 1/2, centred) / sample_discrete_gauss of MatZq, PolynomialRingZq, MatPolynomialRingZq and MatZ through
the C ABI (psf_sample_*, include/psf_mi355x.h): fills bound to no PSF handle.

A fill is `count` polynomials of `n` coefficients, row-major, polynomial first_index + c in row c.  Every value is a pure function of
(seed, tag, global polynomial index, coefficient): a fill of [0, 8) is the fill of [0, 3) followed by the fill of [3, 8).  `tag` (64 ... 255)
selects the stream; two tags under one seed are independent.  Everything runs on the device."""
import ctypes as C

import numpy as np

from ._ffi import _p, check, lib

TAG_MIN, TAG_MAX = 64, 255


def _head(device, seed, tag, first_index, count, n):
    return (C.c_int(device), C.c_uint64(seed), C.c_uint32(tag), C.c_uint64(first_index), C.c_size_t(count), C.c_size_t(n))


def cbd_slots(eta):
    """(slots per 32-bit word, coefficients per Philox block) of the centred-binomial contract"""
    sw = 16 // eta
    return sw, 4 * sw


def sample_uniform(count, n, q, seed, tag=TAG_MIN, first_index=0, device=0):
    """uniform on [0, q) (MatZq / PolynomialRingZq::sample_uniform): uint64 (count, n)"""
    out = np.empty((count, n), dtype=np.uint64)
    check(lib().psf_sample_uniform(*_head(device, seed, tag, first_index, count, n), C.c_uint64(q), _p(out, C.c_uint64)), "sample_uniform")
    return out


def sample_cbd(count, n, eta, seed, tag=TAG_MIN, first_index=0, device=0):
    """centred binomial: 2 eta trials at p = 1/2 shifted by -eta (sample_binomial; the law of FIPS 203's SamplePolyCBD_eta): int64 (count, n)"""
    out = np.empty((count, n), dtype=np.int64)
    check(lib().psf_sample_cbd(*_head(device, seed, tag, first_index, count, n), C.c_uint32(eta), _p(out, C.c_int64)), "sample_cbd")
    return out


def sample_discrete_gauss(count, n, s, seed, center=0.0, centers=None, tag=TAG_MIN, first_index=0, device=0):
    """D_{Z,s,c} (sample_discrete_gauss): int64 (count, n).  `centers`: a (count, n) array of doubles, one centre per coefficient (then `center`
    is ignored).  Raises PsfError(ERR_SAMPLER) when a draw ended at the attempt cap or a centre was at or beyond 2^62."""
    out = np.empty((count, n), dtype=np.int64)
    cen = None
    if centers is not None:
        cen = np.ascontiguousarray(centers, dtype=np.float64)
        if cen.size != count * n:
            raise ValueError(f"sample_discrete_gauss: {cen.size} centres for {count} x {n} samples")
    check(lib().psf_sample_discrete_gauss(*_head(device, seed, tag, first_index, count, n), C.c_double(center),
                                          _p(cen, C.c_double) if cen is not None else None, C.c_double(s), _p(out, C.c_int64)), "sample_discrete_gauss")
    return out


def sample_uniform_dev(d_out, count, n, q, seed, tag=TAG_MIN, first_index=0, io_bits=64, device=0, stream=None):
    """psf_sample_uniform_dev on a device buffer (raw pointer, e.g. torch `data_ptr()`), in `stream`, nothing allocated: uint64, or uint16
    (io_bits 16, q <= 2^16)."""
    check(lib().psf_sample_uniform_dev(*_head(device, seed, tag, first_index, count, n), C.c_uint64(q), C.c_void_p(d_out), C.c_int(io_bits),
                                       C.c_void_p(stream or 0)), "sample_uniform_dev")


def sample_cbd_dev(d_out, count, n, eta, seed, tag=TAG_MIN, first_index=0, io_bits=64, device=0, stream=None):
    """psf_sample_cbd_dev: int64 or int16 -- what matpoly_mul_*_dev reads as operand b."""
    check(lib().psf_sample_cbd_dev(*_head(device, seed, tag, first_index, count, n), C.c_uint32(eta), C.c_void_p(d_out), C.c_int(io_bits),
                                   C.c_void_p(stream or 0)), "sample_cbd_dev")


def sample_discrete_gauss_dev(d_out, count, n, s, seed, center=0.0, d_centers=None, d_fail=None, tag=TAG_MIN, first_index=0, io_bits=64, device=0,
                              stream=None):
    """psf_sample_discrete_gauss_dev: int64 (int16 with a shared centre and |center| + 6 s + 1 < 2^15).  d_centers: count x n device doubles or
    None; d_fail: a device int (or None) that is OR-ed with 1 when a draw ended at the attempt cap or a centre was at or beyond 2^62."""
    check(lib().psf_sample_discrete_gauss_dev(*_head(device, seed, tag, first_index, count, n), C.c_double(center), C.c_void_p(d_centers or 0),
                                              C.c_double(s), C.c_void_p(d_out), C.c_void_p(d_fail or 0), C.c_int(io_bits), C.c_void_p(stream or 0)),
          "sample_discrete_gauss_dev")
