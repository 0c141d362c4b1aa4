"""The kernels of tools_amd/csrc/psf_slhdsa_sha2.hip and psf_sha2.hip, compiled for gfx950 here (no GPU needed): the expected kernels exactly, and in
the code-object metadata of each no spilled register and no private segment -- the SHA-2 state, the 16-word schedule and the midstates of every chain,
tree and T_l hash stay in registers, and whatever is indexed by a run-time value is read from memory.  Every kernel runs 256 threads, and LDS is used
only where DESIGN.md "SLH-DSA: the SHA-2 sets" says: the leaves of KeyGen's tree reduction, 512 nodes of n bytes.  Only the metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = {"psf_slhdsa_sha2": r"_ZN3psf4slh2\d+k_\w+", "psf_sha2": r"_ZN3psf4sha2\d+k_\w+"}
# name: how many instantiations (NQ = n / 4 = 4, 6, 8; SHA-256 and SHA-512)
WANT = {"psf_slhdsa_sha2": {"11k_kg_chains": 3, "9k_kg_leaf": 3, "9k_kg_tree": 3, "11k_vf_digest": 3, "9k_vf_fors": 3, "12k_vf_fors_pk": 3, "9k_vf_wots": 3,
                            "9k_vf_xmss": 3},
        "psf_sha2": {"6k_sha2": 2}}
LDS = {"9k_kg_tree": (512 * 16, 512 * 24, 512 * 32)}


def _base(symbol):
    return re.match(r"_ZN3psf4(?:slh2|sha2)(\d+k_[a-z_0-9]+?)(?:I|E)", symbol).group(1)


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{unit: {kernel symbol: its metadata record}} from the listings of the units"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc on this host")
    tmp = tmp_path_factory.mktemp("isa")
    meta = {}
    for unit, symbol in UNITS.items():
        out = tmp / (unit + ".s")
        src = os.path.join(ROOT, "tools_amd", "csrc", unit + ".hip")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(out),
                               "-x", "hip", src], stderr=subprocess.DEVNULL)
        meta[unit] = {}
        for block in re.split(r"\n\s+- \.", out.read_text()):
            nm = re.search(r"\.name:\s+(" + symbol + r")\s", block)
            if nm:
                meta[unit][nm.group(1)] = block
    return meta


def _all(metadata):
    return {name: block for unit in metadata.values() for name, block in unit.items()}


def test_the_kernel_list_exactly(metadata):
    for unit, want in WANT.items():
        got = {}
        for symbol in metadata[unit]:
            got[_base(symbol)] = got.get(_base(symbol), 0) + 1
        assert got == want, (unit, sorted(metadata[unit]))


def test_no_spills_and_no_private_segment(metadata):
    assert len(_all(metadata)) == 26
    for name, block in _all(metadata).items():
        spills = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", block)]
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spills == [0, 0] and private == 0, (name, spills, private)


def test_workgroup_shapes(metadata):
    """every kernel runs 256 threads; LDS: the 512 n-byte nodes of k_kg_tree (8, 12 and 16 KiB for n = 16, 24, 32), nothing else"""
    for name, block in _all(metadata).items():
        flat = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert flat == 256, (name, flat)
        assert lds in LDS.get(_base(name), (0,)), (name, lds)
    trees = [b for n, b in metadata["psf_slhdsa_sha2"].items() if _base(n) == "9k_kg_tree"]
    assert sorted(int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)) for b in trees) == [8192, 12288, 16384]
