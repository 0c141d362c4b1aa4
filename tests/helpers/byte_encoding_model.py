"""FIPS 203 ByteEncode_d / ByteDecode_d (Algorithms 5 / 6) for a flat array of any length, in two independent forms that must agree:

  *_int  the definition: the bytes are the little-endian encoding of the integer sum_i (y_i mod 2^d) 2^(i d), ceil(len d / 8) of them
  *_np   numpy bit arrays (unpackbits / packbits with bitorder="little"), for large inputs

Bit j of value i is stream bit i d + j; byte b holds stream bits 8b ... 8b + 7, least significant first; the unused high bits of a final
partial byte are 0."""
import numpy as np


def nbytes(length, d):
    return (length * d + 7) // 8


def encode_int(ys, d):
    total = 0
    for i, y in enumerate(ys):
        total |= (int(y) & ((1 << d) - 1)) << (i * d)
    return total.to_bytes(nbytes(len(ys), d), "little")


def decode_int(data, d, length, q=0):
    """(values, noncanonical): values in [0, 2^d) for q = 0, else their residues mod q with the flag set when one was >= q"""
    total = int.from_bytes(bytes(data), "little")
    vals = [(total >> (i * d)) & ((1 << d) - 1) for i in range(length)]
    if q:
        return [v % q for v in vals], any(v >= q for v in vals)
    return vals, False


def encode_np(ys, d):
    """ys: any integer array (int64 / uint64 / uint16 bit patterns); returns uint8 (nbytes,)"""
    ys = np.ascontiguousarray(ys).ravel()
    w = ys.view(np.uint64) if ys.dtype.itemsize == 8 else ys.astype(np.uint64)
    bits = np.unpackbits(w.astype("<u8").view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :d]
    return np.packbits(bits.ravel(), bitorder="little")


def decode_np(data, d, length, q=0):
    """returns (uint64 (length,), noncanonical)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    assert data.size == nbytes(length, d)
    bits = np.unpackbits(data, bitorder="little")[:length * d].reshape(length, d)
    full = np.zeros((length, 64), dtype=np.uint8)
    full[:, :d] = bits
    vals = np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(length).astype(np.uint64)
    if q:
        return vals % np.uint64(q), bool((vals >= np.uint64(q)).any())
    return vals, False
