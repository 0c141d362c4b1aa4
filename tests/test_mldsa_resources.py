"""The kernels of tools_amd/csrc/psf_mldsa.hip, compiled for gfx950 here (no GPU needed): the expected kernels exactly, and in the code-object
metadata of each no spilled register and no private segment -- the Keccak states of the samplers, of the gathered hashes and of the verification
tail stay in registers, and SampleInBall's data-indexed polynomial is in LDS, not in scratch.  Every kernel runs 256 threads, and LDS is used only
where DESIGN.md "ML-DSA" says.  Only the metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf3dsa\d+k_\w+"
# name: how many instantiations
WANT = {"9k_rej_ntt": 2, "13k_rej_bounded": 2, "6k_ball": 1, "12k_image_from": 1, "6k_seed": 1, "4k_tr": 1, "4k_mu": 1, "6k_hint": 1, "8k_unpack": 1, "6k_pack": 1,
        "13k_verify_tail": 2}
BYTE_STAGE = 4 * 256 * 68                                                 # four waves, 256 coefficients, 64 lanes + 4 bytes per row
LDS = {"9k_rej_ntt": (0, 256), "13k_rej_bounded": (BYTE_STAGE,), "6k_ball": (BYTE_STAGE,)}


def _base(symbol):
    return re.match(r"_ZN3psf3dsa(\d+k_[a-z_0-9]+?)(?:I|E)", symbol).group(1)


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: its metadata record} from the listing of the unit"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_mldsa.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_mldsa.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                           "-x", "hip", src], stderr=subprocess.DEVNULL)
    meta = {}
    for block in re.split(r"\n\s+- \.", out.read_text()):
        nm = re.search(r"\.name:\s+(" + SYMBOL + r")\s", block)
        if nm:
            meta[nm.group(1)] = block
    return meta


def test_the_kernel_list_exactly(metadata):
    got = {}
    for symbol in metadata:
        got[_base(symbol)] = got.get(_base(symbol), 0) + 1
    assert got == WANT, sorted(metadata)


def test_no_spills_and_no_private_segment(metadata):
    assert metadata
    for name, block in metadata.items():
        spills = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spills == [0, 0] and private == 0, (name, spills, private)


def test_workgroup_shapes(metadata):
    """every kernel runs 256 threads; LDS: the byte staging of RejBoundedPoly and SampleInBall (17 KiB per wave) and the 256-byte permutation of the
    image form of RejNTTPoly"""
    for name, block in metadata.items():
        flat = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert flat == 256, (name, flat)
        assert lds in LDS.get(_base(name), (0,)), (name, lds)
    assert sorted(int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)) for n, b in metadata.items() if _base(n) == "9k_rej_ntt") == [0, 256]
