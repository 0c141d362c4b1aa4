"""The kernels of tools_amd/csrc/psf_slhdsa_sha2_sign.hip, compiled for gfx950 here (no GPU needed): the expected kernels exactly, and in the code-object
metadata of each no spilled register and no private segment -- the SHA-2 states, the 16-word schedule, the midstates, HMAC's key blocks and its inner
digest stay in registers, so no secret value can reach scratch memory, and whatever is indexed by a run-time value is read from memory.  Every kernel runs
256 threads, and LDS is used only where DESIGN.md "SLH-DSA: signing for the SHA-2 sets" says: the 512 nodes of n bytes of the FORS subtree reduction and of
the packed XMSS tree reduction.  Only the metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = r"_ZN3psf4slh2\d+k_\w+"
# name: how many instantiations (NQ = n / 4 = 4, 6, 8)
WANT = {"12k_sg_prf_msg": 3, "11k_sg_digest": 3, "9k_sg_fors": 3, "13k_sg_fors_top": 3, "12k_sg_fors_pk": 3, "11k_sg_chains": 3, "9k_sg_leaf": 3, "9k_sg_tree": 3, "9k_sg_wots": 3}
LDS = {"9k_sg_fors": (512 * 16, 512 * 24, 512 * 32), "9k_sg_tree": (512 * 16, 512 * 24, 512 * 32)}


def _base(symbol):
    return re.match(r"_ZN3psf4slh2(\d+k_[a-z_0-9]+?)(?:I|E)", symbol).group(1)


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: its metadata record} from the listing of the unit"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("isa") / "psf_slhdsa_sha2_sign.s"
    src = os.path.join(ROOT, "tools_amd", "csrc", "psf_slhdsa_sha2_sign.hip")
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
    assert len(metadata) == 27
    for name, block in metadata.items():
        spills = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spills == [0, 0] and private == 0, (name, spills, private)


def test_workgroup_shapes(metadata):
    """every kernel runs 256 threads; LDS: the 512 n-byte nodes of k_sg_fors and k_sg_tree (8, 12 and 16 KiB for n = 16, 24, 32), nothing else"""
    for name, block in metadata.items():
        flat = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert flat == 256, (name, flat)
        assert lds in LDS.get(_base(name), (0,)), (name, lds)
    for kern in LDS:
        assert sorted(int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)) for n, b in metadata.items() if _base(n) == kern) == [8192, 12288, 16384], kern
