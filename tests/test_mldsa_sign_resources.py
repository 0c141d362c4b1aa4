"""The kernels of tools_amd/csrc/psf_mldsa_sign.hip, compiled for gfx950 here (no GPU needed): the expected kernels exactly, and in the code-object
metadata of each no spilled register and no private segment -- the Keccak states of ExpandMask, of the mu / rho'' hashes and of the c~ hash stay in
registers.  Every kernel runs 256 threads, and LDS is used only where DESIGN.md "ML-DSA signing" says: the check stage's two reduction words and hint
mask.  Only the metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf3dsa\d+k_\w+"
# name: how many instantiations
WANT = {"13k_sign_unpack": 1, "11k_sign_seed": 1, "13k_expand_mask": 2, "13k_sign_ctilde": 2, "12k_sign_check": 2, "12k_sign_match": 1, "11k_sign_move": 1,
        "13k_sign_commit": 1}
LDS = {"12k_sign_check": (2 * 4 + 8 * 32,)}                                # sh_bits, sh_cnt and 32 bytes of hint bits for each of at most 8 polynomials


def _base(symbol):
    return re.match(r"_ZN3psf3dsa(\d+k_[a-z_0-9]+?)(?:I|E)", symbol).group(1)


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: its metadata record} from the listing of the unit"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_mldsa_sign.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_mldsa_sign.hip")
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
    for name, block in metadata.items():
        flat = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert flat == 256, (name, flat)
        assert lds in LDS.get(_base(name), (0,)), (name, lds)
