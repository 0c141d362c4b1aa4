"""The perturbation centres x = sqrt(Sigma_2) d (mp_perturbation.rs:315) against exact rationals: the reference multiplies MatQ by MatQ; the library and the
oracle form each x_i in FP64.  Shared by tests/test_centres_exact_cpu.py (the oracle's trace) and tests/test_gpu_centres_exact.py (the device's stages)."""
from fractions import Fraction

U = Fraction(1, 2**53)                     # unit roundoff of FP64


def gamma(k):
    """gamma_k = k u / (1 - k u): the bound on the relative error of a k-term dot product in ANY summation order, with or without fused multiply-adds
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)"""
    return k * U / (1 - k * U)


def exact_dot(a, b):
    """(sum a_j b_j, sum |a_j b_j|) of two sequences of doubles as Fractions; the products are dyadic, so they are summed as integers over one power of two"""
    terms = []
    for x, y in zip(a, b):
        nx, dx = float(x).as_integer_ratio()
        ny, dy = float(y).as_integer_ratio()
        terms.append((nx * ny, (dx * dy).bit_length() - 1))
    top = max(sh for _, sh in terms)
    s = sum(n << (top - sh) for n, sh in terms)
    a_ = sum(abs(n) << (top - sh) for n, sh in terms)
    return Fraction(s, 1 << top), Fraction(a_, 1 << top)


def check_row(L_packed, d, x, p, sample_z_at):
    """One preimage.  L_packed: rows 0 .. m-1 of the factor (row i holds i + 1 entries); d, x, p: the stages.  sample_z_at(i, centre) draws coordinate i at a
    centre.  Asserts (1) |x_i - exact_i| <= gamma_{i+1} sum_j |L_ij d_j| and (2) the draw at the exact centre (rounded once to a double) is the stage's p_i.
    Returns the worst error as a fraction of its bound."""
    m, off, worst = len(x), 0, Fraction(0)
    for i in range(m):
        exact, absum = exact_dot(L_packed[off:off + i + 1], d[:i + 1])
        off += i + 1
        err, bound = abs(Fraction(float(x[i])) - exact), gamma(i + 1) * absum
        assert err <= bound, f"coordinate {i}: |x - exact| = {float(err):.3e} exceeds gamma_{i + 1} sum|L d| = {float(bound):.3e}"
        if bound:
            worst = max(worst, err / bound)
        z = sample_z_at(i, float(exact))
        assert z == int(p[i]), f"coordinate {i}: the draw at the exact centre is {z}, the stage drew {int(p[i])}"
    assert off == len(L_packed)
    return float(worst)
