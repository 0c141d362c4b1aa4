"""The cyclic tables (make_ntt_plan_cyclic, Z_q[X]/(X^n - 1)) through the wave-level NTT templates of tools_amd/csrc/psf_ntt_core.hpp on the CPU
(tests/ntt_model/ntt_cyclic_model.cpp): the plan has the (L, d) and the table shape of the negacyclic plan for every (q, n) of the device tests, the pair
product of the 16 shapes of the negacyclic model equals a schoolbook product mod X^n - 1 for random and extreme operands, and the accumulation step of
the matrix product stays exact on every wave shape past the fold interval.  Every 24-bit multiply and Montgomery step asserts its operand ranges."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cyclic_tables_through_the_wave_ntt_model(tmp_path):
    exe = str(tmp_path / "ntt_cyclic_model")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "ntt_model", "ntt_cyclic_model.cpp"),
                           os.path.join(ROOT, "tools_amd", "csrc", "psf_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "NTT_CYCLIC_MODEL OK" in out.stdout
    assert "DIFFERENT" not in out.stdout
    assert out.stdout.count(": same") == 30                       # every (q, n) of the plan comparison
    assert len(re.findall(r"^pair .*: ok \(0 mismatches\)$", out.stdout, re.M)) == 48      # 16 shapes x {random, extreme, extreme-flat}
    assert len(re.findall(r"^acc .*: ok \(0 mismatches\)$", out.stdout, re.M)) == 75       # 25 wave shapes x 3 operand kinds
    for m in re.finditer(r"acc shape \d+ \d+ (\d+) q=\d+ inner=(\d+) T=(\d+) extreme", out.stdout):
        if m.group(1) != "0":                                     # the 16-bit forms fold: the worst case ran past the interval
            assert 1 <= int(m.group(3)) < int(m.group(2)), m.group(0)
