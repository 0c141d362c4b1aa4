"""The kernels of tools_amd/csrc/psf_compress.hip, compiled for gfx950 here (no GPU needed): each one without scratch, spills or calls -- in
particular no 128-bit division helper (__udivti3 / __umodti3 / __divti3) and no s_swappc: the divisions by q are the host's reciprocals."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_compress.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_compress.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", src], stderr=subprocess.DEVNULL)
    return out.read_text()


def kernels(asm):
    """{symbol: body} of every kernel in the listing, from its label to the end of its descriptor"""
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_ZN3psf3cmp11k_coeff_map\w+):.*?^\s*\.end_amdhsa_kernel", asm, re.S | re.M)}


def test_every_op_and_word_size_has_a_kernel(device_asm):
    ks = kernels(device_asm)
    want = {f"ILi{op}ELi{io}E" for op in range(4) for io in (16, 64)}
    assert {w for w in want if any(w in k for k in ks)} == want, sorted(ks)


def test_no_scratch_spills_or_calls(device_asm):
    ks = kernels(device_asm)
    assert ks
    for name, body in ks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "scratch_" not in body and "buffer_store" not in body, name
        assert "s_swappc" not in body and "s_setpc" not in body and "s_call" not in body, name
        for helper in ("__udivti3", "__umodti3", "__divti3", "__modti3", "__udivdi3", "__umoddi3"):
            assert helper not in body, (name, helper)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name       # 16 bytes per lane
        assert re.search(r"global_load_dwordx4 .*\bnt\b", body) and re.search(r"global_store_dwordx4 .*\bnt\b", body), name
    for helper in ("__udivti3", "__umodti3", "__divti3", "__modti3"):
        assert helper not in device_asm
    spills = {}                                                 # the code-object metadata: one "- .agpr_count" record per kernel
    for block in re.split(r"\n\s+- \.", device_asm):
        nm = re.search(r"\.name:\s+(_ZN3psf3cmp11k_coeff_map\w+)", block)
        if nm:
            spills[nm.group(1)] = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
    assert set(spills) == set(ks), sorted(spills)
    assert all(v == [0, 0] for v in spills.values()), spills
