"""'FP64 centres pick the integers exact-rational centres would pick'  for the perturbation centres x = sqrt(Sigma_2) d, on the
oracle's own trace: every x_i within the dot-product bound gamma_{i+1} sum |L_ij d_j| of the exact rational product, and SampleZ at the exact centre returns
the trace's p_i.  tests/test_gpu_centres_exact.py asserts the same of the device's FP64 matrix-core products."""
import pytest

from tests.helpers import centres_exact as ce


@pytest.mark.parametrize("n,q", [(8, 128), (32, 256)])
def test_oracle_centres_against_exact_rationals(oracle, n, q):
    r, s, seed = 3.0, 25.0 if n == 8 else 200.0, 77
    psf = oracle.PSFPerturbation(oracle.gadget_params_default(n, q), r, s)
    assert psf.trap_gen(5) == 0
    L = psf.L_packed
    u = oracle.uniform_targets(2, 4, n, q)
    for index in ((0, 1, 3) if n == 8 else (2,)):
        st = psf.samp_p_trace(seed, index, u[index])
        worst = ce.check_row(L, st["d"], st["x"], st["p"], lambda i, c: oracle.sample_z(seed, oracle.TAG_PERTURB, index, i, c, r))
        assert 0 < worst <= 1
