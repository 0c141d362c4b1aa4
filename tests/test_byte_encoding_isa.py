"""The byte-encoding kernels of tools_amd/csrc/psf_compress.hip (k_pack, k_unpack), compiled for gfx950 here (no GPU needed): each one without
scratch, spills, calls or division helpers, below 128 VGPRs, with 16-byte non-temporal loads and stores on its tile path."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf3cmp(?:6k_pack|8k_unpack)\w+"


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
    """{symbol: body} of every byte-encoding kernel in the listing, from its label to the end of its descriptor"""
    return {m.group(1): m.group(0) for m in re.finditer(r"^(" + SYMBOL + r"):.*?^\s*\.end_amdhsa_kernel", asm, re.S | re.M)}


def test_every_form_and_word_size_has_a_kernel(device_asm):
    ks = kernels(device_asm)
    want = {f"6k_packILi{f}ELi{io}E" for f in (0, 1) for io in (16, 64)} | {f"8k_unpackILi{m}ELi{io}E" for m in (0, 1, 2) for io in (16, 64)}
    assert {w for w in want if any(w in k for k in ks)} == want, sorted(ks)
    assert len(ks) == len(want), sorted(ks)


def test_no_scratch_spills_calls_or_divisions(device_asm):
    ks = kernels(device_asm)
    assert ks
    for name, body in ks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "scratch_" not in body and "buffer_store" not in body, name
        assert "s_swappc" not in body and "s_setpc" not in body and "s_call" not in body, name
        assert not re.search(r"__u?(div|mod)[a-z]i3", body), name
        assert "v_rcp_iflag_f32" not in body and "v_rcp_f32" not in body, name      # the inline expansion of an integer division
        assert re.search(r"global_load_dwordx4 .*\bnt\b", body) and re.search(r"global_store_dwordx4 .*\bnt\b", body), name
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        assert vgprs < 128, (name, vgprs)
    assert not re.search(r"__u?(div|mod)[a-z]i3", device_asm)
    meta = {}                                                  # the code-object metadata: one "- .agpr_count" record per kernel
    for block in re.split(r"\n\s+- \.", device_asm):
        nm = re.search(r"\.name:\s+(" + SYMBOL + r")", block)
        if nm:
            meta[nm.group(1)] = ([int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)],
                                 int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    assert set(meta) == set(ks), sorted(meta)
    assert all(v == ([0, 0], 0) for v in meta.values()), meta


def test_the_flag_is_raised_by_a_vector_atomic(device_asm):
    for name, body in kernels(device_asm).items():
        if "8k_unpackILi1E" in name:
            assert "global_atomic_or" in body, name
        else:
            assert "atomic" not in body, name
