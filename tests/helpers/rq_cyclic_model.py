"""Python big-integer model of the products of the cyclic ring Z_q[X]/(X^n - 1) (new_cyclic, common_moduli.rs:72-79): the definition, with no modular
shortcut -- every coefficient product and sum is an exact Python integer, reduced mod q once at the end."""
import numpy as np


def cyclic(a, b):
    """a * b in Z[X]/(X^n - 1), exact (object arrays of Python ints)"""
    n = len(a)
    full = np.convolve(np.asarray(a, dtype=object), np.asarray(b, dtype=object))
    out = full[:n].copy()
    out[: n - 1] += full[n:]
    return out


def poly_mul(a, b, q):
    """rows of a times rows of b mod (X^n - 1, q) -> uint64 in [0, q); a, b: (count, n) or (n,) of any integer dtype"""
    a, b = np.asarray(a), np.asarray(b)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    out = np.array([[int(v) % q for v in cyclic(x.astype(object), y.astype(object))] for x, y in zip(a2, b2)], dtype=np.uint64).reshape(a2.shape)
    return out[0] if a.ndim == 1 else out


def matpoly_entry(A, B, q, i, j):
    """one output polynomial C[i][j] of A (rows, inner, n) times B (inner, cols, n) mod (X^n - 1, q)"""
    A, B = np.asarray(A), np.asarray(B)
    acc = np.zeros(A.shape[2], dtype=object)
    for k in range(A.shape[1]):
        acc = acc + cyclic(A[i, k].astype(object), B[k, j].astype(object))
    return np.array([int(v) % q for v in acc], dtype=np.uint64)


def matpoly_mul(A, B, q):
    """A (rows, inner, n) times B (inner, cols, n) mod (X^n - 1, q) -> (rows, cols, n) uint64 in [0, q)"""
    A, B = np.asarray(A), np.asarray(B)
    rows, inner, n = A.shape
    assert B.shape[0] == inner and B.shape[2] == n
    out = np.zeros((rows, B.shape[1], n), dtype=np.uint64)
    for i in range(rows):
        for j in range(B.shape[1]):
            out[i, j] = matpoly_entry(A, B, q, i, j)
    return out
