"""The fill kernels of tools_amd/csrc/psf_sample.hip, compiled for gfx950 here (no GPU needed): every instantiation present, none with scratch,
spills or calls; the centred-binomial, uniform and table kernels without a division and with 16-byte non-temporal stores; the table kernel
without an exponential or an f64 fma once its table is built; the failure flag raised by a vector atomic in the Gaussian kernels only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf3smp\d+k_fill_\w+"
NAMES = ("14k_fill_uniform", "10k_fill_cbd", "16k_fill_gauss_tab", "12k_fill_gauss")


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_sample.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_sample.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", src], stderr=subprocess.DEVNULL)
    return out.read_text()


def kernels(asm):
    """{symbol: body} of every fill kernel in the listing, from its label to the end of its descriptor"""
    return {m.group(1): m.group(0) for m in re.finditer(r"^(" + SYMBOL + r"):.*?^\s*\.end_amdhsa_kernel", asm, re.S | re.M)}


def streaming(name):
    """the kernels held to the no-division and vector-store rules: all but the general Gaussian one"""
    return "12k_fill_gaussILi" not in name


def test_every_instantiation_exists(device_asm):
    ks = kernels(device_asm)
    want = {f"{nm}ILi{io}E" for nm in NAMES for io in (16, 64)}
    assert {w for w in want if any(w in k for k in ks)} == want, sorted(ks)
    assert len(ks) == len(want), sorted(ks)


def test_no_scratch_spills_or_calls(device_asm):
    ks = kernels(device_asm)
    assert ks
    for name, body in ks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "scratch_" not in body and "buffer_store" not in body, name
        assert "s_swappc" not in body and "s_setpc" not in body and "s_call" not in body, name
    meta = {}                                                  # the code-object metadata: one "- .agpr_count" record per kernel
    for block in re.split(r"\n\s+- \.", device_asm):
        nm = re.search(r"\.name:\s+(" + SYMBOL + r")", block)
        if nm:
            meta[nm.group(1)] = ([int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)],
                                 int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    assert set(meta) == set(ks), sorted(meta)
    assert all(v == ([0, 0], 0) for v in meta.values()), meta


def test_no_division_and_vector_stores_in_the_streaming_kernels(device_asm):
    assert not re.search(r"__u?(div|mod)[a-z]i3", device_asm)
    for name, body in kernels(device_asm).items():
        if not streaming(name):
            continue
        assert "v_rcp_iflag_f32" not in body and "v_rcp_f32" not in body, name      # the inline expansion of an integer division
        assert re.search(r"global_store_dwordx4 .*\bnt\b", body), name


def test_table_kernel_has_no_exponential_after_its_prologue(device_asm):
    """the table is built before the kernel's only barrier; the attempt loop and the write-out behind it evaluate no exp and no f64 fma"""
    seen = 0
    for name, body in kernels(device_asm).items():
        if "16k_fill_gauss_tab" not in name:
            continue
        seen += 1
        assert "v_exp_f32" not in body, name
        assert body.count("s_barrier") == 1, name
        prologue, loop = body.split("s_barrier")
        assert "v_fma_f64" in prologue, name
        assert not re.search(r"v_(fma|mul|add)_f64", loop), name
        assert "ds_read" in loop or "ds_load" in loop, name
    assert seen == 2


def test_the_flag_is_raised_by_a_vector_atomic_in_the_gaussian_kernels_only(device_asm):
    for name, body in kernels(device_asm).items():
        if "k_fill_gauss" in name:
            assert "global_atomic_or" in body, name
        else:
            assert "atomic" not in body, name
