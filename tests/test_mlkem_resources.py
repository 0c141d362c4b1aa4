"""The kernels of tools_amd/csrc/psf_mlkem.hip, compiled for gfx950 here (no GPU needed): every kernel present, and in the code-object metadata
of each no spilled register and no private segment -- the Keccak states of the gathered hashes and of the decapsulation tail, with the comparison
beside them, stay in registers.  Only the metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf5mlkem\d+k_\w+"
WANT = ["3k_g", "13k_encaps_hash", "13k_keygen_tail", "8k_unpack", "6k_pack", "7k_canon", "9k_add_msg", "13k_decaps_tail", "10k_check_ek", "10k_check_dk"]


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: its metadata record} from the listing of the unit"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_mlkem.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_mlkem.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", src], stderr=subprocess.DEVNULL)
    meta = {}
    for block in re.split(r"\n\s+- \.", out.read_text()):
        nm = re.search(r"\.name:\s+(" + SYMBOL + r")\s", block)
        if nm:
            meta[nm.group(1)] = block
    return meta


def test_every_kernel_exists(metadata):
    assert {w for w in WANT if any(k.startswith("_ZN3psf5mlkem" + w + "E") for k in metadata)} == set(WANT), sorted(metadata)
    assert len(metadata) == len(WANT), sorted(metadata)


def test_no_spills_and_no_private_segment(metadata):
    assert metadata
    for name, block in metadata.items():
        spills = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spills == [0, 0] and private == 0, (name, spills, private)


def test_workgroup_shapes(metadata):
    """every kernel runs 256 threads; only the decapsulation tail (64 comparison results) and the vote of check_ek use LDS"""
    for name, block in metadata.items():
        flat = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert flat == 256, (name, flat)
        assert lds == (256 if "k_decaps_tail" in name else lds if "k_check_ek" in name else 0), (name, lds)
