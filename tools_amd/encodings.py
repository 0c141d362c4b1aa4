"""utils::common_encodings (common_encodings.rs:49-151): the floor(q/base) mu message layer of lattice encryption, through the C ABI.

A value becomes its base-`base` digits mu (least significant first) in Python integers; the device scales them, out = mu floor(q/base) mod q, and
rounds them back, mu = floor((base c + floor(q/(2 base))) / q) mod base; composing the digits into a value is again Python.  Power-of-two bases
split and compose through bytes and np.unpackbits / np.packbits."""
import ctypes as C

import numpy as np

from ._ffi import ERR_PARAM, ERR_UNSUPPORTED, PsfError, _p, check, lib
from .compression import _residues


def _check_base(base, where):
    if base < 2:
        raise PsfError(ERR_PARAM, f"{where}: base {base} < 2")                       # common_encodings.rs:135-139 (and :63 through log_ceil)
    if base >= 1 << 63:
        raise PsfError(ERR_UNSUPPORTED, f"{where}: base {base} >= 2^63")


def _pow2_exponent(base):
    return base.bit_length() - 1 if base & (base - 1) == 0 else 0


def _split(values, base, n, where):
    """(count, n) uint64: the digits of each value, least significant first (common_encodings.rs:71-77)"""
    values = [int(v) for v in values]
    if any(v < 0 for v in values):
        raise PsfError(ERR_PARAM, f"{where}: a value is negative")                    # :58-62
    _check_base(base, where)
    limit = base ** n
    if any(v >= limit for v in values):
        raise PsfError(ERR_PARAM, f"{where}: a value needs more than {n} digits in base {base}")   # :64-69
    count = len(values)
    k = _pow2_exponent(base)
    if count == 0 or n == 0:
        return np.zeros((count, n), dtype=np.uint64)
    if k:
        nb = (n * k + 7) // 8
        raw = np.frombuffer(b"".join(v.to_bytes(nb, "little") for v in values), dtype=np.uint8).reshape(count, nb)
        bits = np.unpackbits(raw, axis=1, bitorder="little")[:, :n * k].reshape(count, n, k).astype(np.uint64)
        return (bits << np.arange(k, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    out = np.zeros((count, n), dtype=np.uint64)
    if max(values) < 1 << 64:
        rest, b = np.array(values, dtype=np.uint64), np.uint64(base)
        for i in range(n):
            out[:, i] = rest % b
            rest //= b
        return out
    for r, v in enumerate(values):
        for i in range(n):
            if v == 0:
                break
            v, out[r, i] = divmod(v, base)
    return out


def _compose(digits, base):
    """the values of (count, n) digit rows, most significant digit last (common_encodings.rs:143-148)"""
    digits = np.ascontiguousarray(digits, dtype=np.uint64)
    count, n = digits.shape
    k = _pow2_exponent(base)
    if k:
        bits = ((digits[:, :, None] >> np.arange(k, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(count, n * k)
        packed = np.packbits(bits, axis=1, bitorder="little")
        return [int.from_bytes(row.tobytes(), "little") for row in packed]
    t = 1                                                      # t digits per uint64 chunk: base^t <= 2^64, so a chunk never wraps
    while base ** (t + 1) <= 1 << 64:
        t += 1
    chunks = []
    for c0 in range(0, n, t):
        acc = np.zeros(count, dtype=np.uint64)
        for i in range(min(n, c0 + t) - 1, c0 - 1, -1):
            acc = acc * np.uint64(base) + digits[:, i]
        chunks.append(acc)
    big = base ** t
    out = []
    for r in range(count):
        v = 0
        for ch in reversed(chunks):
            v = v * big + int(ch[r])
        out.append(v)
    return out


def encode_digits(digits, base, q, device=0):
    """psf_encode_digits: digit floor(q/base) mod q per entry, any shape"""
    d = np.ascontiguousarray(digits, dtype=np.uint64)
    out = np.empty(d.shape, dtype=np.uint64)
    check(lib().psf_encode_digits(C.c_int(device), C.c_uint64(q), C.c_uint64(base), C.c_size_t(d.size), _p(d, C.c_uint64), _p(out, C.c_uint64)),
          "encode_digits")
    return out


def decode_digits(coeffs, base, q, device=0):
    """psf_decode_digits: floor((base c + floor(q/(2 base))) / q) mod base per coefficient (c read mod q), any shape"""
    c = _residues(coeffs, q)
    out = np.empty(c.shape, dtype=np.uint64)
    check(lib().psf_decode_digits(C.c_int(device), C.c_uint64(q), C.c_uint64(base), C.c_size_t(c.size), _p(c, C.c_uint64), _p(out, C.c_uint64)),
          "decode_digits")
    return out


def encode_values(values, base, q, n, device=0):
    """encode_value_in_polynomialringzq for many values: (count, n) uint64 coefficients, one polynomial per value"""
    digits = _split(values, base, n, "encode_values")
    return encode_digits(digits, base, q, device)


def decode_values(coeffs, base, q, device=0):
    """decode_value_from_polynomialringzq for each row of a (count, n) array of coefficients: a list of Python ints"""
    _check_base(base, "decode_values")
    c = np.asarray(coeffs)
    c = c.reshape(-1, c.shape[-1])
    return _compose(decode_digits(c, base, q, device), base)


def encode_value_in_polynomialringzq(value, base, q, n, device=0):
    """common_encodings.rs:49-91: uint64[n], the coefficients of value's base-`base` digits times floor(q/base) in Z_q[X]/(f), deg f = n.
    PsfError(PSF_ERR_PARAM) where the reference returns an error: value < 0, more than n digits, base < 2."""
    return encode_values([value], base, q, n, device)[0]


def decode_value_from_polynomialringzq(coeffs, base, q, device=0):
    """common_encodings.rs:125-151: the value whose base-`base` digits the n coefficients encode.  PsfError(PSF_ERR_PARAM) if base < 2."""
    return decode_values(np.asarray(coeffs).reshape(1, -1), base, q, device)[0]


def encode_digits_dev(d_digits, d_out, q, base, length, io_bits=64, device=0, stream=None):
    """psf_encode_digits_dev on device buffers (raw pointers), in `stream`: uint64 -> uint64 (io_bits 64) or uint16 -> uint16 (io_bits 16)."""
    check(lib().psf_encode_digits_dev(C.c_int(device), C.c_uint64(q), C.c_uint64(base), C.c_size_t(length), C.c_void_p(d_digits), C.c_void_p(d_out),
                                      C.c_int(io_bits), C.c_void_p(stream or 0)), "encode_digits_dev")


def decode_digits_dev(d_coeffs, d_digits, q, base, length, io_bits=64, device=0, stream=None):
    """psf_decode_digits_dev on device buffers (raw pointers), in `stream`: uint64 -> uint64 (io_bits 64) or uint16 -> uint16 (io_bits 16)."""
    check(lib().psf_decode_digits_dev(C.c_int(device), C.c_uint64(q), C.c_uint64(base), C.c_size_t(length), C.c_void_p(d_coeffs), C.c_void_p(d_digits),
                                      C.c_int(io_bits), C.c_void_p(stream or 0)), "decode_digits_dev")
