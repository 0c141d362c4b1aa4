"""Python big-integer model of the fused R_q matrix product C = E + sign * A B (psf_matpoly_mul_add_*): the product of rq_model / rq_cyclic_model
(exact Python integers, reduced mod q once) and one exact addition or subtraction per coefficient."""
import numpy as np

from tests.helpers import rq_cyclic_model, rq_model

RINGS = {"negacyclic": rq_model.matpoly_mul, "cyclic": rq_cyclic_model.matpoly_mul}


def add_signed(E, P, q, sign):
    """E + sign * P mod q, coefficient by coefficient in Python integers -> uint64 in [0, q); E of any integer dtype, P residues"""
    if sign not in (1, -1):
        raise ValueError(f"sign {sign}")
    E, P = np.asarray(E), np.asarray(P)
    assert E.shape == P.shape, (E.shape, P.shape)
    out = [(int(e) + sign * int(p)) % q for e, p in zip(E.reshape(-1).tolist(), P.reshape(-1).tolist())]
    return np.array(out, dtype=np.uint64).reshape(P.shape)


def matpoly_mul_add(A, B, E, q, sign=1, ring="negacyclic"):
    """E (rows, cols, n) + sign * A (rows, inner, n) B (inner, cols, n) mod (X^n + 1 or X^n - 1, q) -> (rows, cols, n) uint64 in [0, q)"""
    return add_signed(E, RINGS[ring](A, B, q), q, sign)
