"""MatPolynomialRingZq * MatPolynomialRingZq over R_q = Z_q[X]/(X^n + 1) through the C ABI (psf_matpoly_mul_*, include/psf_mi355x.h), and the
products of the cyclic ring Z_q[X]/(X^n - 1) (new_cyclic, common_moduli.rs:72-79): the *_cyclic functions at the end, with the same conventions.
The matpoly_mul_add* functions are the fused forms E + sign * A B (psf_matpoly_mul_add_*): one launch for t = A s + e or w = v - s^T u.

The reference multiplies matrices of polynomials at gpv_ring.rs:245 (a * sigma), gadget_ring.rs:78 (a_bar * r), gadget_ring.rs:190-202 (is_trapdoor)
and short_basis_ring.rs:183-198 (is_basis).  A matrix of polynomials is an array (rows, cols, n): row-major, constant term first."""
import ctypes as C

import numpy as np

from ._ffi import _p, check, lib


def matpoly_mul(A, B, q, device=0):
    """A (rows, inner, n) times B (inner, cols, n) mod (X^n + 1, q) on the device; returns (rows, cols, n) uint64 in [0, q).
    Signed entries are read as integers (reduced mod q), unsigned ones as residues."""
    A, B = np.asarray(A), np.asarray(B)
    if A.ndim != 3 or B.ndim != 3 or A.shape[1] != B.shape[0] or A.shape[2] != B.shape[2]:
        raise ValueError(f"matpoly_mul: shapes {A.shape} x {B.shape}")
    rows, inner, n = A.shape
    cols = B.shape[1]
    a = np.ascontiguousarray(np.mod(A.astype(np.int64), np.int64(q)).astype(np.uint64) if A.dtype.kind == "i" else A, dtype=np.uint64)
    b = np.ascontiguousarray(np.mod(B, q).astype(np.int64) if B.dtype.kind == "u" else B, dtype=np.int64)
    c = np.empty((rows, cols, n), dtype=np.uint64)
    check(lib().psf_matpoly_mul_negacyclic(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols),
                                           _p(a, C.c_uint64), _p(b, C.c_int64), _p(c, C.c_uint64)), "matpoly_mul")
    return c


def matpoly_mul_dev(d_a, d_b, d_c, q, n, count, rows, inner, cols, a_stride=0, trans_a=0, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_negacyclic_dev on device buffers (raw pointers, e.g. torch `data_ptr()`), in `stream`, nothing allocated:
    C[c] = op(A[c]) B[c] for c < count; a_stride in polynomials (0: one A for every batch), trans_a = 1: A stored inner x rows."""
    check(lib().psf_matpoly_mul_negacyclic_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner),
                                               C.c_size_t(cols), C.c_void_p(d_a), C.c_size_t(a_stride), C.c_int(trans_a), C.c_void_p(d_b), C.c_void_p(d_c),
                                               C.c_int(io_bits), C.c_void_p(stream or 0)), "matpoly_mul_dev")


def matpoly_mul_hat_dev(d_hat, d_b, d_c, q, n, count, rows, inner, cols, hat_stride=0, trans_a=0, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_hat_dev: the same with A given by its images (psf_ntt_forward_dev, rows * inner of them per batch in A's storage order);
    hat_stride in 32-bit words, 0: one set of images for every batch."""
    check(lib().psf_matpoly_mul_hat_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner),
                                        C.c_size_t(cols), C.c_void_p(d_hat), C.c_size_t(hat_stride), C.c_int(trans_a), C.c_void_p(d_b), C.c_void_p(d_c),
                                        C.c_int(io_bits), C.c_void_p(stream or 0)), "matpoly_mul_hat_dev")


def _mul_add_host(fn, where, A, B, E, q, sign, device):
    A, B, E = np.asarray(A), np.asarray(B), np.asarray(E)
    if A.ndim != 3 or B.ndim != 3 or A.shape[1] != B.shape[0] or A.shape[2] != B.shape[2] or E.shape != (A.shape[0], B.shape[1], A.shape[2]):
        raise ValueError(f"{where}: shapes {A.shape} x {B.shape} + {E.shape}")
    rows, inner, n = A.shape
    cols = B.shape[1]
    a = np.ascontiguousarray(np.mod(A.astype(np.int64), np.int64(q)).astype(np.uint64) if A.dtype.kind == "i" else A, dtype=np.uint64)
    b = np.ascontiguousarray(np.mod(B, q).astype(np.int64) if B.dtype.kind == "u" else B, dtype=np.int64)
    e = np.ascontiguousarray(np.mod(E, q).astype(np.int64) if E.dtype.kind == "u" else E, dtype=np.int64)
    c = np.empty((rows, cols, n), dtype=np.uint64)
    check(fn(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols), _p(a, C.c_uint64), _p(b, C.c_int64),
             _p(e, C.c_int64), C.c_int(sign), _p(c, C.c_uint64)), where)
    return c


def _mul_add_dev(fn, where, d_a, d_b, d_e, d_c, q, n, count, rows, inner, cols, a_stride, trans_a, sign, io_bits, device, stream):
    check(fn(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols), C.c_void_p(d_a),
             C.c_size_t(a_stride), C.c_int(trans_a), C.c_void_p(d_b), C.c_void_p(d_e), C.c_int(sign), C.c_void_p(d_c), C.c_int(io_bits),
             C.c_void_p(stream or 0)), where)


def matpoly_mul_add(A, B, E, q, sign=1, device=0):
    """E + sign * A B mod (X^n + 1, q) on the device (psf_matpoly_mul_add_negacyclic): A (rows, inner, n), B (inner, cols, n), E (rows, cols, n), sign +1 or -1;
    returns (rows, cols, n) uint64 in [0, q).  Signed entries are read as integers, unsigned ones as residues, as in matpoly_mul."""
    return _mul_add_host(lib().psf_matpoly_mul_add_negacyclic, "matpoly_mul_add", A, B, E, q, sign, device)


def matpoly_mul_add_dev(d_a, d_b, d_e, d_c, q, n, count, rows, inner, cols, a_stride=0, trans_a=0, sign=1, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_add_negacyclic_dev on device buffers: C[c] = E[c] + sign * op(A[c]) B[c], the arguments of matpoly_mul_dev with E (laid out like C,
    in B's word type: int64 of any value or int16 in (-q, q)) and sign (+1 or -1).  d_e == d_c accumulates in place; any other overlap is an error."""
    _mul_add_dev(lib().psf_matpoly_mul_add_negacyclic_dev, "matpoly_mul_add_dev", d_a, d_b, d_e, d_c, q, n, count, rows, inner, cols, a_stride, trans_a, sign,
                 io_bits, device, stream)


def matpoly_mul_add_hat_dev(d_hat, d_b, d_e, d_c, q, n, count, rows, inner, cols, hat_stride=0, trans_a=0, sign=1, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_add_hat_dev: matpoly_mul_add_dev with A given by its images (psf_ntt_forward_dev); hat_stride in 32-bit words, 0: one set for every batch."""
    _mul_add_dev(lib().psf_matpoly_mul_add_hat_dev, "matpoly_mul_add_hat_dev", d_hat, d_b, d_e, d_c, q, n, count, rows, inner, cols, hat_stride, trans_a, sign,
                 io_bits, device, stream)


# ---- the cyclic ring Z_q[X]/(X^n - 1) ------------------------------------------------------------------------------------------------------------------

def poly_mul_cyclic(a, b, q, device=0, method=None):
    """a * b in Z_q[X]/(X^n - 1) on the device (psf_poly_mul_cyclic).  a: residues (count x n or n), b: signed integers of the same shape.
    method: None = automatic, 0 = schoolbook kernel, 1 = NTT kernel (PsfError(UNSUPPORTED) when q / n do not admit one)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.int64)
    if a.ndim not in (1, 2) or a.shape != b.shape or a.shape[-1] == 0:
        raise ValueError(f"poly_mul_cyclic: shapes {a.shape} x {b.shape}")
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    out = np.zeros_like(a2)
    check(lib().psf_poly_mul_cyclic_method(C.c_int(device), C.c_uint64(q), C.c_size_t(a2.shape[1]), C.c_size_t(a2.shape[0]), _p(a2, C.c_uint64),
                                           _p(b2, C.c_int64), _p(out, C.c_uint64), C.c_int(-1 if method is None else method)), "poly_mul_cyclic")
    return out.reshape(a.shape)


def poly_mul_cyclic_dev(d_a, d_b, d_out, q, n, count, io_bits=64, device=0, stream=None):
    """psf_poly_mul_cyclic_dev on device buffers (raw pointers), in `stream`, nothing allocated; the layouts of gadget.poly_mul_negacyclic_dev."""
    check(lib().psf_poly_mul_cyclic_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_void_p(d_a), C.c_void_p(d_b),
                                        C.c_void_p(d_out), C.c_int(io_bits), C.c_void_p(stream or 0)), "poly_mul_cyclic_dev")


def ntt_forward_cyclic_dev(d_a, d_hat, q, n, count, io_bits=64, device=0, stream=None):
    """psf_ntt_forward_cyclic_dev: count * n 32-bit words of opaque images, valid only for poly_mul_hat_cyclic_dev / matpoly_mul_hat_cyclic_dev."""
    check(lib().psf_ntt_forward_cyclic_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_void_p(d_a), C.c_int(io_bits),
                                           C.c_void_p(d_hat), C.c_void_p(stream or 0)), "ntt_forward_cyclic_dev")


def poly_mul_hat_cyclic_dev(d_hat, hat_stride, d_b, d_out, q, n, count, io_bits=64, device=0, stream=None):
    """psf_poly_mul_hat_cyclic_dev: d_out[c] = image[c * hat_stride] * d_b[c]; hat_stride in words, 0 = one image for every product."""
    check(lib().psf_poly_mul_hat_cyclic_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_void_p(d_hat), C.c_size_t(hat_stride),
                                            C.c_void_p(d_b), C.c_void_p(d_out), C.c_int(io_bits), C.c_void_p(stream or 0)), "poly_mul_hat_cyclic_dev")


def matpoly_mul_cyclic(A, B, q, device=0):
    """matpoly_mul over Z_q[X]/(X^n - 1): A (rows, inner, n) times B (inner, cols, n); returns (rows, cols, n) uint64 in [0, q)."""
    A, B = np.asarray(A), np.asarray(B)
    if A.ndim != 3 or B.ndim != 3 or A.shape[1] != B.shape[0] or A.shape[2] != B.shape[2]:
        raise ValueError(f"matpoly_mul_cyclic: shapes {A.shape} x {B.shape}")
    rows, inner, n = A.shape
    cols = B.shape[1]
    a = np.ascontiguousarray(np.mod(A.astype(np.int64), np.int64(q)).astype(np.uint64) if A.dtype.kind == "i" else A, dtype=np.uint64)
    b = np.ascontiguousarray(np.mod(B, q).astype(np.int64) if B.dtype.kind == "u" else B, dtype=np.int64)
    c = np.empty((rows, cols, n), dtype=np.uint64)
    check(lib().psf_matpoly_mul_cyclic(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols),
                                       _p(a, C.c_uint64), _p(b, C.c_int64), _p(c, C.c_uint64)), "matpoly_mul_cyclic")
    return c


def matpoly_mul_cyclic_dev(d_a, d_b, d_c, q, n, count, rows, inner, cols, a_stride=0, trans_a=0, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_cyclic_dev: matpoly_mul_dev over Z_q[X]/(X^n - 1)."""
    check(lib().psf_matpoly_mul_cyclic_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner),
                                           C.c_size_t(cols), C.c_void_p(d_a), C.c_size_t(a_stride), C.c_int(trans_a), C.c_void_p(d_b), C.c_void_p(d_c),
                                           C.c_int(io_bits), C.c_void_p(stream or 0)), "matpoly_mul_cyclic_dev")


def matpoly_mul_hat_cyclic_dev(d_hat, d_b, d_c, q, n, count, rows, inner, cols, hat_stride=0, trans_a=0, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_hat_cyclic_dev: A given by its images from ntt_forward_cyclic_dev (rows * inner per batch, in A's storage order)."""
    check(lib().psf_matpoly_mul_hat_cyclic_dev(C.c_int(device), C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner),
                                               C.c_size_t(cols), C.c_void_p(d_hat), C.c_size_t(hat_stride), C.c_int(trans_a), C.c_void_p(d_b), C.c_void_p(d_c),
                                               C.c_int(io_bits), C.c_void_p(stream or 0)), "matpoly_mul_hat_cyclic_dev")


def matpoly_mul_add_cyclic(A, B, E, q, sign=1, device=0):
    """matpoly_mul_add over Z_q[X]/(X^n - 1) (psf_matpoly_mul_add_cyclic)."""
    return _mul_add_host(lib().psf_matpoly_mul_add_cyclic, "matpoly_mul_add_cyclic", A, B, E, q, sign, device)


def matpoly_mul_add_cyclic_dev(d_a, d_b, d_e, d_c, q, n, count, rows, inner, cols, a_stride=0, trans_a=0, sign=1, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_add_cyclic_dev: matpoly_mul_add_dev over Z_q[X]/(X^n - 1)."""
    _mul_add_dev(lib().psf_matpoly_mul_add_cyclic_dev, "matpoly_mul_add_cyclic_dev", d_a, d_b, d_e, d_c, q, n, count, rows, inner, cols, a_stride, trans_a, sign,
                 io_bits, device, stream)


def matpoly_mul_add_hat_cyclic_dev(d_hat, d_b, d_e, d_c, q, n, count, rows, inner, cols, hat_stride=0, trans_a=0, sign=1, io_bits=64, device=0, stream=None):
    """psf_matpoly_mul_add_hat_cyclic_dev: A given by its images from ntt_forward_cyclic_dev."""
    _mul_add_dev(lib().psf_matpoly_mul_add_hat_cyclic_dev, "matpoly_mul_add_hat_cyclic_dev", d_hat, d_b, d_e, d_c, q, n, count, rows, inner, cols, hat_stride,
                 trans_a, sign, io_bits, device, stream)
