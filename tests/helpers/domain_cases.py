"""Rows for the exact check_domain tests (tests/test_check_domain_exact_cpu.py, tests/test_gpu_check_domain_exact.py).

The reference decides check_domain in exact rationals (mp_perturbation.rs:396-402, gpv.rs:219-224, gpv_ring.rs:274-283): a row of length m is in the
domain iff ||e||^2 <= s^2 m r^2 (r = 1 for the two GPV types), every double standing for the rational it denotes.  Everything here is Python int / Fraction:
no expected value comes from the oracle or the library."""
import math
from fractions import Fraction
from math import isqrt

import numpy as np

TWO63 = 1 << 63


def floor_bound(s, r, m):
    """floor(s^2 m r^2) of the doubles s and r as exact rationals"""
    return math.floor(Fraction(s) ** 2 * m * Fraction(r) ** 2)


def double_bound(s, r, m):
    """the bound as the library formed it before: three roundings"""
    return ((s * s) * float(m)) * (r * r)


def row_with_norm(N, m, salt=0):
    """An int64 row of length m with ||row||^2 == N exactly: greedy squares (isqrt of the remainder until it is zero, each entry capped at 2^63), the entries spread
    over the row -- the last position included, so a ragged last stride of the kernel takes part -- with mixed signs; |v| = 2^63 is the entry -2^63."""
    vals, rem = [], N
    while rem:
        a = min(isqrt(rem), TWO63)
        vals.append(a)
        rem -= a * a
    assert len(vals) <= m, (N, m, len(vals))
    pos = np.random.default_rng(1000 + salt).permutation(m - 1)[:max(len(vals) - 1, 0)].tolist()
    row = [0] * m
    for j, a in enumerate(vals):
        p = m - 1 if j == 0 else pos[j - 1]
        row[p] = -a if (a == TWO63 or (j + salt) % 2) else a
    assert sum(v * v for v in row) == N
    return row


def rows_array(rows):
    return np.array(rows, dtype=np.int64)


def expected(norms, fb):
    return np.array([n <= fb for n in norms], dtype=bool)


def on_the_bound_pairs(m, r, count=20, k0=680000):
    """(K, s) with s one of the three doubles around sqrt(K / (m r^2)) where the rounded-double bound and the exact bound disagree about an integer norm.
    Returns (wrong_accepts, wrong_rejects): lists of s with floor(double bound) > floor(exact) -- the old rule accepts floor(exact) + 1 -- and with
    double bound < floor(exact) -- the old rule rejects floor(exact)."""
    acc, rej = [], []
    K = k0
    while len(acc) < count or len(rej) < count:
        s0 = math.sqrt(K / (m * r * r))
        for s in (math.nextafter(s0, 0.0), s0, math.nextafter(s0, math.inf)):
            fb, db = floor_bound(s, r, m), double_bound(s, r, m)
            if math.floor(db) > fb and len(acc) < count:
                acc.append(s)
            elif db < fb and len(rej) < count:
                rej.append(s)
        K += 1
        assert K < k0 + 400000
    return acc, rej


def window_norms(fb, lo=-34, hi=36):
    """norms fb + d, d = lo .. hi: floor(B) - 1, floor(B), floor(B) + 1 and floor(B) + 2 among at least 70 rows, accepted and rejected mixed"""
    return [fb + d for d in range(lo, hi + 1) if fb + d >= 0]


def carry_norms(fb):
    """norms around fb whose low 64 bits are zero or all ones: a carry lost between limbs (in the norm or in the comparison) flips the answer"""
    top = fb >> 64
    out = {top << 64, ((top + 1) << 64) - 1, (top + 1) << 64, ((top + 2) << 64) - 1}
    if top:
        out |= {(top << 64) - 1, (top - 1) << 64}
    if fb >> 128:
        t2 = fb >> 128
        out |= {t2 << 128, (t2 << 128) - 1, ((t2 + 1) << 128) - 1, (t2 + 1) << 128, (t2 << 128) + (1 << 64), (t2 << 128) + (1 << 64) - 1}
    return sorted(out)


def huge_norms(fb, m):
    """norms at and above 2^53, 2^64 and 2^128 from entries of -2^63 and 2^63 - 1, including those a 128-bit sum wraps into the accepted range"""
    big = TWO63 - 1
    out = [(1 << 53) + 1, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, 1 << 126, big * big, 2 * big * big, 4 * big * big,
           (1 << 128) - 1, 1 << 128, (1 << 128) + 1, (1 << 128) + fb, (1 << 128) + fb + 1, (1 << 129) + fb,
           (m - 8) * (1 << 126), m * (1 << 126), m * big * big]
    return out


def huge_rows(fb, m):
    """(rows, norms) of huge_norms; the last two are the all -2^63 and the all 2^63 - 1 rows"""
    norms = huge_norms(fb, m)
    rows = [row_with_norm(N, m, salt=i) for i, N in enumerate(norms[:-2])]
    rows.append([-TWO63] * m)
    rows.append([TWO63 - 1] * m)
    return rows, norms


def mixed_batch(fb, m, with_huge=True):
    """one call's rows: the window around floor(B), the carry norms that fit, the huge norms; returns (int64 array, expected bool array)"""
    norms = window_norms(fb) + [n for n in carry_norms(fb) if n <= (m - 8) * (1 << 126)]
    rows = [row_with_norm(N, m, salt=i) for i, N in enumerate(norms)]
    if with_huge:
        hr, hn = huge_rows(fb, m)
        # interleave: a huge row after every fourth ordinary one, so a wrong row index shows
        mixed_r, mixed_n, it = [], [], iter(zip(hr, hn))
        for i, (rw, nn) in enumerate(zip(rows, norms)):
            mixed_r.append(rw); mixed_n.append(nn)
            if i % 4 == 3:
                nx = next(it, None)
                if nx:
                    mixed_r.append(nx[0]); mixed_n.append(nx[1])
        for nx in it:
            mixed_r.append(nx[0]); mixed_n.append(nx[1])
        rows, norms = mixed_r, mixed_n
    assert len(rows) >= 70
    exp = expected(norms, fb)
    assert exp.any() and not exp.all()
    return rows_array(rows), exp, norms
