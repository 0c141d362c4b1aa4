"""The signing part of the FIPS 205 core (tools_amd/csrc/psf_slhdsa_sign_core.hpp) on the CPU: g++ compiles the text the device kernels compile, over
the plain C++ back end, into the stand-alone program tests/cpp/slhdsa_sign_host_check.cpp, which signs by the decomposition of the kernels (FORS
subtrees, tops, all layers from the digest, recomputed WOTS+ values).  Its output is compared byte for byte with the pure-Python model: the hedged
signatures of the shared fixture for all six sets, and 128f's four deterministic messages around the block edge of H_msg.  A second build with
-fsanitize=address,undefined runs the 128f cases; it is a program of its own, nothing loaded into Python runs under a sanitizer.  The helper
exact_by_parts, which the device tests rely on, is checked here against the fixture and against tampered signatures."""
import os
import shutil
import subprocess

import pytest

from tests.helpers import slhdsa_cases as K
from tests.helpers import slhdsa_model as M
from tests.helpers import slhdsa_sign_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "slhdsa_sign_host_check.cpp")
F128 = "SLH-DSA-SHAKE-128f"


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host check of the SLH-DSA signing core"
    out = str(tmp / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slhdsa_sign_host_check")
    return {"plain": _build(tmp, "check", []), "san": _build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), "tmp": tmp}


def _hex(b):
    return b.hex() if b else "-"


def _case(name, sk, msg, addrnd, sig):
    return (f"sign {M.IDS[name]} {sk.hex()} {_hex(msg)} {_hex(addrnd or b'')}", sig.hex())


def _check(programs, which, cases, tag):
    path = programs["tmp"] / f"{tag}.txt"
    path.write_text("\n".join(c for c, _ in cases) + "\n")
    out = subprocess.run([programs[which], str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (tag, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases), (tag, len(got), len(cases))
    for i, (g, (line, want)) in enumerate(zip(got, cases)):
        if g != want:
            first = next(k for k in range(0, len(want), 2) if g[k:k + 2] != want[k:k + 2]) // 2
            raise AssertionError((tag, i, line[:12], "first differing byte", first))


def _edge_cases(name):
    return [_case(name, sk, msg, None, sig) for sk, msg, sig in S.edge_inputs(name)]


@pytest.mark.parametrize("name", M.NAMES)
def test_the_fixture_signatures_hedged(programs, name):
    _check(programs, "plain", [_case(name, *t) for t in S.hedged(name)], "hedged_" + name[-4:])


def test_the_deterministic_edge_messages_of_128f(programs):
    cases = _edge_cases(F128)
    assert len(cases) == 4 and any(line.split()[3] == "-" for line, _ in cases)
    _check(programs, "plain", cases, "edges")


def test_the_128f_cases_under_address_and_undefined_behaviour_sanitizers(programs):
    _check(programs, "san", [_case(F128, *t) for t in S.hedged(F128)] + _edge_cases(F128), "san")


def test_exact_by_parts_accepts_the_model_and_names_what_differs():
    for name in (F128, "SLH-DSA-SHAKE-256f"):
        sk, msg, addrnd, sig = S.hedged(name)[0]
        assert S.exact_by_parts(name, sk, msg, addrnd, sig) is None
        assert S.exact_by_parts(name, sk, msg, bytes(len(addrnd)), sig) == "R"
        assert S.exact_by_parts(name, sk, msg, None, sig) == "R"
        reg = M.regions(name)
        for lo, _ in (reg["R"], reg["fors_sk"][1], reg["fors_auth"][2], reg["wots"][3], reg["auth"][4]):
            assert S.exact_by_parts(name, sk, msg, addrnd, K.flip(sig, lo + 1, 3)) == "verify"
        assert S.exact_by_parts(name, sk, msg, addrnd, sig[:-1]) == "size"
    sk, msg, sig = S.edge_inputs(F128)[3]
    assert msg == b"" and S.exact_by_parts(F128, sk, msg, None, sig) is None
    # a signature of the same message under another SK.seed verifies under its own key but is not this key's
    ks = K.keys(F128, 3)
    assert S.exact_by_parts(F128, ks["sk"][1][:16] + ks["sk"][0][16:], msg, None, sig) in ("verify", "fors_sk0")
