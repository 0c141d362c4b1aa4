"""The R_q matrix-product kernels compiled for gfx950 here (no GPU needed): k_matpoly_mul (psf_ntt_kernels.hpp) has one instantiation per wave shape of
for_shape (psf_ntt_shapes.hpp), I/O width (16 bits only in the 16-bit Montgomery forms) and form of A (polynomials, images in global memory, images in LDS);
k_matpoly_negacyclic (psf_rq_kernels.hpp, built in psf_rq.hip) is the schoolbook route.  None of them has scratch, spills or calls."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tools_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _asm(tmp_path_factory, name):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / (name + ".s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", os.path.join(CSRC, name)], stderr=subprocess.DEVNULL)
    return out.read_text()


@pytest.fixture(scope="module")
def ntt_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "psf_ntt.hip")


@pytest.fixture(scope="module")
def rq_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "psf_rq.hip")


def kernels(asm, pattern):
    """{symbol: body} of every kernel whose symbol matches, from its label to the end of its descriptor"""
    return {m.group(1): m.group(0) for m in re.finditer(r"^(" + pattern + r"\w*):.*?^\s*\.end_amdhsa_kernel", asm, re.S | re.M)}


def spill_counts(asm, pattern):
    out = {}
    for block in re.split(r"\n\s+- \.", asm):                 # the code-object metadata: one record per kernel
        nm = re.search(r"\.name:\s+(" + pattern + r"\w*)", block)
        if nm:
            out[nm.group(1)] = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
    return out


def check_clean(asm, ks, pattern):
    assert ks
    for name, body in ks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "scratch_" not in body and "buffer_store" not in body, name
        assert "s_swappc" not in body and "s_setpc" not in body and "s_call" not in body, name
    sp = spill_counts(asm, pattern)
    assert set(sp) == set(ks), sorted(sp)
    assert all(v == [0, 0] for v in sp.values()), sp


def wave_shapes():
    src = open(os.path.join(CSRC, "psf_ntt_shapes.hpp")).read()
    body = src[src.index("template <class F> bool for_shape"):]
    body = body[:body.index("#undef PSF_SHAPE")]
    return [tuple(int(v) for v in m) for m in re.findall(r"PSF_SHAPE\((\d+), (\d+), (\d+)\)", body)]


def test_one_instantiation_per_wave_shape_io_width_and_form(ntt_asm):
    ks = kernels(ntt_asm, r"_ZN3psf3ntt13k_matpoly_mul")
    shapes = wave_shapes()
    assert len(shapes) == 25
    want = set()
    for ln, ld, qb in shapes:
        for io in ((16, 64) if qb else (64,)):
            for form in (0, 1, 2):
                want.add(f"ILi{ln}ELi{ld}ELi{qb}ELi{io}ELi{form}E")
    got = [re.search(r"I(Li\d+E){5}", k).group(0) for k in ks]
    assert sorted(got) == sorted(want), (len(got), len(want))


def test_no_scratch_spills_or_calls(ntt_asm, rq_asm):
    check_clean(ntt_asm, kernels(ntt_asm, r"_ZN3psf3ntt13k_matpoly_mul"), r"_ZN3psf3ntt13k_matpoly_mul")
    ks = kernels(rq_asm, r"_ZN3psf20k_matpoly_negacyclic")
    assert len(ks) == 1, sorted(ks)
    check_clean(rq_asm, ks, r"_ZN3psf20k_matpoly_negacyclic")
