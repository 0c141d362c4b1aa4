"""How exact are the centres the gadget walk samples around?  (The twin of tests/test_oracle_centre_precision.py for randomized_nearest_plane_gadget,
mp_perturbation.rs:173-191.)

The reference keeps c' = <c, b~_i> / |b~_i|^2 in exact rationals; the library and the oracle form it in doubles from the Gram-Schmidt table of S_k.  This
test recomputes every centre of a traced walk (orc_randomized_nearest_plane_gadget_trace) from the integer S_k with an exact Gram-Schmidt in Fraction, following
the trace's own z_i, and asserts the worst error, in units of the draw's width s_G / |b~_i|, below 2^-40 -- the bound the project asserts for single-pass
nearest plane.  It also counts the exact centres that are integers and how many of those the FP64 walk saw as non-integers (reported, not asserted: SampleZ
has one more candidate at an integer centre)."""
import math
from fractions import Fraction

import numpy as np
import pytest

CONFIGS = [  # (n, q, base, k, r)
    (8, 128, 2, 7, 3.0),
    (64, 128, 2, 7, 6.0),
    (8, 157, 2, 8, 3.0),          # not a power of the base: the last column of S_k holds q's digits
    (8, 256, 4, 4, 3.0),          # a larger base, q = base^k
    (8, 157, 3, 5, 3.0),          # a larger base, q not a power of it
]


def exact_gso_columns(Sk):
    """Gram-Schmidt of the columns of the integer matrix S_k in Fraction: (vectors, squared norms)"""
    k = Sk.shape[0]
    cols = [[Fraction(int(Sk[t, i])) for t in range(k)] for i in range(k)]
    G, n2 = [], []
    for i in range(k):
        g = list(cols[i])
        for l in range(i):
            mu = sum(x * y for x, y in zip(cols[i], G[l])) / n2[l]
            if mu:
                g = [x - mu * y for x, y in zip(g, G[l])]
        G.append(g)
        n2.append(sum(x * x for x in g))
    return G, n2


def walk_errors(oracle, n, q, base, k, r, calls, seed=77):
    """(worst |c'_fp64 - c'_exact| / width, draws, exact centres that are integers, of those seen as non-integers in FP64, draws whose value changes
    when SampleZ is given the exact centre rounded to a double)"""
    m_bar = oracle.gadget_params_default(n, q).m_bar
    psf = oracle.PSFPerturbation(oracle.GadgetParams(n, k, m_bar, base, q), r, 100.0, with_L=False)
    Sk = psf.Sk
    G, n2 = exact_gso_columns(Sk)
    v = oracle.uniform_targets(2, calls, n, q)
    worst, draws, ints, ints_missed, changed = Fraction(0), 0, 0, 0, 0
    for b in range(calls):
        z, cen, wid, coef = psf.gadget_sample_trace(seed, b, v[b])
        assert (z == psf.gadget_sample(seed, b, v[b])).all()                       # the trace is the walk
        for j in range(n):
            c = [-int(x) for x in oracle.find_solution_gadget_vec(int(v[b, j]), q, k, base)]
            for i in range(k - 1, -1, -1):
                exact = sum(x * y for x, y in zip(c, G[i])) / n2[i]
                got = float(cen[j * k + i])
                worst = max(worst, abs(Fraction(got) - exact) / Fraction(float(wid[j * k + i])))
                draws += 1
                if exact.denominator == 1:
                    ints += 1
                    ints_missed += got != math.floor(got)
                zi = int(coef[j * k + i])
                changed += oracle.sample_z(seed, oracle.TAG_GADGET, b, j * k + i, float(exact), float(wid[j * k + i])) != zi
                if zi:
                    c = [x - zi * int(Sk[t, i]) for t, x in enumerate(c)]
            assert [-x for x in c] == [int(x) for x in z[j * k:(j + 1) * k]]     # the exact walk ends on the trace's z
    return float(worst), draws, ints, ints_missed, changed


@pytest.mark.parametrize("n,q,base,k,r", CONFIGS)
def test_gadget_centres_within_2_to_minus_40_of_the_exact_ones(oracle, n, q, base, k, r):
    worst, draws, ints, missed, changed = walk_errors(oracle, n, q, base, k, r, calls=6 if n > 8 else 40)
    assert draws >= 1000
    assert worst < 2.0**-40, (worst, math.log2(worst) if worst else None)


def test_report_measured_errors(oracle, capsys):
    """not an assertion: prints the figures quoted in DESIGN.md section 2 (run with -s)"""
    rows = [(cfg, walk_errors(oracle, *cfg, calls=6 if cfg[0] > 8 else 40)) for cfg in CONFIGS]
    with capsys.disabled():
        for (n, q, base, k, r), (worst, draws, ints, missed, changed) in rows:
            w = f"2^{math.log2(worst):.1f}" if worst else "0"
            print(f"\n[gadget centre precision] n={n} q={q} base={base} k={k} r={r}: worst error {w} of the width over {draws} draws; exact centre an integer: "
                  f"{ints}, of those non-integer in FP64: {missed}; draws that change at the exact centre: {changed}", end="")
