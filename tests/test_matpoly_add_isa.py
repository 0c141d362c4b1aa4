"""The fused R_q matrix-product kernels compiled for gfx950 here (no GPU needed): k_matpoly_fma (psf_ntt_kernels.hpp, instantiated in psf_ntt_fma.hip)
has one instantiation per wave shape of for_shape (psf_ntt_shapes.hpp), I/O width (16 bits only in the 16-bit Montgomery forms) and form of A (polynomials,
images in global memory, images in LDS), exactly like k_matpoly_mul; k_matpoly_fma_negacyclic / k_matpoly_fma_cyclic (psf_rq_kernels.hpp, built in
psf_rq.hip) are the schoolbook routes.  None of them has scratch, spills or calls.  Resource checks only.

The epilogue of k_matpoly_fma reads E, sign and out from the kernel-argument segment through MatFmaKernArgs (psf_ntt_kernels.hpp): the offsets of that
struct are compared here with the offsets the code object records for every instantiation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tools_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FMA = r"_ZN3psf3ntt13k_matpoly_fma"


def _asm(tmp_path_factory, name):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa_fma") / (name + ".s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", os.path.join(CSRC, name)], stderr=subprocess.DEVNULL)
    return out.read_text()


@pytest.fixture(scope="module")
def fma_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "psf_ntt_fma.hip")


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
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0\b", body), name
        # the resource record behind the kernel: plain numbers (a callee would make them expressions over its own), nothing private, no stack
        sym = re.escape(name)
        assert re.search(r"\.set " + sym + r"\.num_vgpr, \d+\s*$", asm, re.M) and re.search(r"\.set " + sym + r"\.numbered_sgpr, \d+\s*$", asm, re.M), name
        for field in ("private_seg_size", "uses_flat_scratch", "has_dyn_sized_stack", "has_recursion", "has_indirect_call"):
            assert re.search(r"\.set " + sym + r"\." + field + r", 0\s*$", asm, re.M), (name, field)
    sp = spill_counts(asm, pattern)
    assert set(sp) == set(ks), sorted(sp)
    assert all(v == [0, 0] for v in sp.values()), sp


def wave_shapes():
    src = open(os.path.join(CSRC, "psf_ntt_shapes.hpp")).read()
    body = src[src.index("template <class F> bool for_shape"):]
    body = body[:body.index("#undef PSF_SHAPE")]
    return [tuple(int(v) for v in m) for m in re.findall(r"PSF_SHAPE\((\d+), (\d+), (\d+)\)", body)]


def test_one_instantiation_per_wave_shape_io_width_and_form(fma_asm):
    ks = kernels(fma_asm, FMA)
    shapes = wave_shapes()
    assert len(shapes) == 25
    want = set()
    for ln, ld, qb in shapes:
        for io in ((16, 64) if qb else (64,)):
            for form in (0, 1, 2):
                want.add(f"ILi{ln}ELi{ld}ELi{qb}ELi{io}ELi{form}E")
    got = [re.search(r"I(Li\d+E){5}", k).group(0) for k in ks]
    assert sorted(got) == sorted(want), (len(got), len(want))
    # and the unit holds nothing else: the products stay in psf_ntt.hip
    assert set(kernels(fma_asm, r"_Z")) == set(ks)


def test_kernel_argument_offsets_match_the_struct_the_epilogue_reads(fma_asm):
    """p 0, m 32, A 96, B 104, E 112, sign 120, out 128 (the static_assert beside MatFmaKernArgs pins the struct's side)"""
    seen = 0
    for block in re.split(r"\n  - \.", fma_asm):            # the code-object metadata: one record per kernel, its arguments nested in it
        nm = re.search(r"^    \.name:\s+(" + FMA + r"\w*)", block, re.M)
        if not nm:
            continue
        offs = [int(v) for v in re.findall(r"\.offset:\s+(\d+)", block)]
        assert offs[:7] == [0, 32, 96, 104, 112, 120, 128], (nm.group(1), offs[:8])
        seen += 1
    assert seen == 117


def test_wave_kernels_have_no_scratch_spills_or_calls(fma_asm):
    check_clean(fma_asm, kernels(fma_asm, FMA), FMA)


@pytest.mark.parametrize("pattern", [r"_ZN3psf24k_matpoly_fma_negacyclic", r"_ZN3psf20k_matpoly_fma_cyclic"])
def test_schoolbook_kernels_are_clean(rq_asm, pattern):
    ks = kernels(rq_asm, pattern)
    assert len(ks) == 1, sorted(ks)
    check_clean(rq_asm, ks, pattern)
