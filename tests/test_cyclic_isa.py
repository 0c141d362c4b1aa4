"""The schoolbook kernels of the cyclic ring (k_polymul_cyclic, k_matpoly_cyclic: psf_rq_kernels.hpp, built in psf_rq.hip) compiled for gfx950 here (no GPU
needed): one instantiation each, no scratch, spills or calls.  The NTT products of the cyclic ring run the existing wave kernels (tests/test_matpoly_isa.py)."""
import pytest

from tests.test_matpoly_isa import _asm, check_clean, kernels


@pytest.fixture(scope="module")
def rq_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "psf_rq.hip")


@pytest.mark.parametrize("pattern", [r"_ZN3psf16k_polymul_cyclic", r"_ZN3psf16k_matpoly_cyclic"])
def test_cyclic_schoolbook_kernels_are_clean(rq_asm, pattern):
    ks = kernels(rq_asm, pattern)
    assert len(ks) == 1, sorted(ks)
    check_clean(rq_asm, ks, pattern)
