"""The accumulation step of the R_q matrix product (Core::acc_add / acc_tick / acc_close in tools_amd/csrc/psf_ntt_core.hpp) on the CPU, for every wave
shape: the same templates instantiated over a 64-lane array (tests/ntt_model/matpoly_model.cpp), worst-case operands summed 4099 times -- past the fold
interval of the 16-bit form -- and random ones, against a schoolbook sum; every 24-bit multiply and Montgomery step asserts its operand ranges."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matpoly_accumulation_model_equals_schoolbook(tmp_path):
    exe = str(tmp_path / "matpoly_model")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "ntt_model", "matpoly_model.cpp"),
                           os.path.join(ROOT, "tools_amd", "csrc", "psf_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "MATPOLY_MODEL OK" in out.stdout
    assert out.stdout.count(": ok (0 mismatches)") == 50          # 25 wave shapes x {extreme, random}
    # the 16-bit forms fold: the worst case ran past the interval
    for m in re.finditer(r"shape \d+ \d+ (\d+) q=\d+ inner=(\d+) T=(\d+) extreme", out.stdout):
        if m.group(1) != "0":
            assert 1 <= int(m.group(3)) < int(m.group(2)), m.group(0)
