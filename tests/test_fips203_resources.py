"""The kernels of tools_amd/csrc/psf_keccak.hip, compiled for gfx950 here (no GPU needed): every instantiation present, and in the code-object
metadata of each no spilled register and no private segment -- the 25 lanes of a Keccak state, the second array of a round and the 24 words of
PRF_3 stay in registers.  Only the metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf2kc\d+k_\w+"
WANT = ([f"8k_keccakILi{rate}E" for rate in (72, 136, 168)] + [f"12k_sample_nttILi{io}E" for io in (16, 64)]
        + [f"12k_sample_cbdILi{eta}ELi{io}E" for eta in (2, 3) for io in (16, 64)]
        + [f"{nm}ILi{io}E" for nm in ("12k_image_from", "10k_image_to") for io in (16, 64)])


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: its metadata record} from the listing of the unit"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_keccak.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_keccak.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", src], stderr=subprocess.DEVNULL)
    meta = {}
    for block in re.split(r"\n\s+- \.", out.read_text()):
        nm = re.search(r"\.name:\s+(" + SYMBOL + r")\s", block)
        if nm:
            meta[nm.group(1)] = block
    return meta


def test_every_kernel_exists(metadata):
    assert {w for w in WANT if any(w in k for k in metadata)} == set(WANT), sorted(metadata)
    assert len(metadata) == len(WANT), sorted(metadata)


def test_no_spills_and_no_private_segment(metadata):
    assert metadata
    for name, block in metadata.items():
        spills = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spills == [0, 0] and private == 0, (name, spills, private)


def test_sampler_workgroups_are_one_wave_with_their_lds(metadata):
    for name, block in metadata.items():
        flat = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        if "k_sample_" in name:
            assert flat == 64 and lds == 256 * 66 * 2, (name, flat, lds)      # [coefficient][64 lanes + 2] 16-bit words
        else:
            assert flat == 256 and lds == 0, (name, flat, lds)
