"""Python big-integer model of the R_q matrix product (MatPolynomialRingZq * MatPolynomialRingZq over Z_q[X]/(X^n + 1)): the definition, with no
modular shortcut -- every coefficient product and sum is an exact Python integer, reduced mod q once at the end."""
import numpy as np


def negacyclic(a, b):
    """a * b in Z[X]/(X^n + 1), exact (object arrays of Python ints)"""
    n = len(a)
    full = np.convolve(np.asarray(a, dtype=object), np.asarray(b, dtype=object))
    out = full[:n].copy()
    out[: n - 1] -= full[n:]
    return out


def matpoly_mul(A, B, q):
    """A (rows, inner, n) times B (inner, cols, n) mod (X^n + 1, q) -> (rows, cols, n) uint64 in [0, q).  Entries of any integer dtype."""
    A = np.asarray(A).astype(object)
    B = np.asarray(B).astype(object)
    rows, inner, n = A.shape
    assert B.shape[0] == inner and B.shape[2] == n
    cols = B.shape[1]
    out = np.zeros((rows, cols, n), dtype=np.uint64)
    for i in range(rows):
        for j in range(cols):
            acc = np.zeros(n, dtype=object)
            for k in range(inner):
                acc = acc + negacyclic(A[i, k], B[k, j])
            out[i, j] = [int(v) % q for v in acc]
    return out


def matpoly_entry(A, B, q, i, j):
    """one output polynomial C[i][j] of matpoly_mul (sampled checks of large products)"""
    A = np.asarray(A)
    B = np.asarray(B)
    acc = np.zeros(A.shape[2], dtype=object)
    for k in range(A.shape[1]):
        acc = acc + negacyclic(A[i, k].astype(object), B[k, j].astype(object))
    return np.array([int(v) % q for v in acc], dtype=np.uint64)
