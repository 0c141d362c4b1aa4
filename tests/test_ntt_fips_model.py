"""The FIPS 203 interop of the NTT images on the CPU (tests/ntt_model/ntt_fips_model.cpp): the forward transform of tools_amd/csrc/psf_ntt_core.hpp
at (3329, 256) over the 64-lane host back end, and the host map of psf_host.cpp, against Algorithm 9 written out with zeta = 17 and against the
schoolbook product -- random, all-zero, all-(q - 1) and unit-vector operands, every 24-bit multiply asserting its operand ranges."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_map_equals_algorithm_9_and_keeps_products():
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = str(pathlib.Path(tmp) / "ntt_fips_model")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "ntt_model", "ntt_fips_model.cpp"),
                               os.path.join(ROOT, "tools_amd", "csrc", "psf_host.cpp")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "NTT_FIPS_MODEL OK" in out.stdout
    assert out.stdout.count("to 0, from 0, from(to) 0 mismatches: ok") == 18      # 8 random, 3 constant and 7 unit-vector operands
    assert "FIPS 203 leaf of image leaf 0 ... 7: 61 60 63 62 58 59 57 56" in out.stdout   # the plan's zeta is 3061 = 17^189
