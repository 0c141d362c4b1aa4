"""'FP64 centres pick the integers exact-rational centres would pick'  for the perturbation centres x = sqrt(Sigma_2) d as the device
forms them -- the FP64 matrix-core product kernels, in every product form the plan takes over the batch sizes below -- against the exact rational product of
the device's own factor L (export_sqrt_sigma2_rows) and normals d (samp_p_stages):
  (1) |x_i - sum_j L_ij d_j| <= gamma_{i+1} sum_j |L_ij d_j|, gamma_k = k 2^-53 / (1 - k 2^-53): the bound of a k-term dot product in any order, no tuning;
  (2) SampleZ at the exact centre returns the stage's p_i, in every coordinate.
Three rows of each batch are recomputed in exact arithmetic (tests/helpers/centres_exact.py); tests/test_centres_exact_cpu.py is the oracle's twin."""
import numpy as np
import pytest

from tests.helpers import centres_exact as ce

pytestmark = pytest.mark.gpu
SEED = 77
BATCHES = (1, 16, 17, 64, 65, 130)


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module", params=[(8, 128, 3.0, 25.0), (32, 256, 3.0, 200.0)], ids=["n8-one-launch", "n32-five-panels"])
def keyed(T, request):
    n, q, r, s = request.param
    psf = T.PSFPerturbation(T.GadgetParameters.init_default(n, q), r, s)
    psf.trap_gen(seed=5, export=False)
    L = psf.export_sqrt_sigma2_rows(0, psf.m)
    yield psf, L, n, q, r
    psf.close()


@pytest.mark.parametrize("B", BATCHES)
def test_device_centres_against_exact_rationals(keyed, oracle, B):
    psf, L, n, q, r = keyed
    plan = psf.query_plan(B)
    u = oracle.uniform_targets(2, B, n, q)
    first = 1000 * B
    st = psf.samp_p_stages(u, seed=SEED, first_index=first)
    worst = 0.0
    for b in sorted({0, B // 2, B - 1}):
        w = ce.check_row(L, st["d"][b], st["x"][b], st["p"][b], lambda i, c: oracle.sample_z(SEED, oracle.TAG_PERTURB, first + b, i, c, r))
        worst = max(worst, w)
    print(f"[centres] n={n} q={q} m={psf.m} B={B}: one_launch={plan['one_launch']} product={plan['product']}; worst error / bound = {worst:.3f}")
    assert 0 < worst <= 1


def test_the_batch_sizes_cover_more_than_one_product_form(keyed):
    """what the batch sizes are for: the plan's product forms differ over them (the one-launch kernel of the small key; tasks and tiles of the five-panel key)"""
    psf, L, n, q, r = keyed
    forms = {(psf.query_plan(B)["one_launch"], psf.query_plan(B)["product"]) for B in BATCHES}
    print(f"[centres] n={n}: forms over {BATCHES}: {sorted(forms)}")
    if n == 8:
        assert any(one for one, _ in forms)
    else:
        assert len(forms) >= 2
