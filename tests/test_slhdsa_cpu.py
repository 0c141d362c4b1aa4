"""The FIPS 205 core of the library (tools_amd/csrc/psf_slhdsa_core.hpp) on the CPU: g++ compiles the text the device kernels compile, over the plain
C++ back end, into the stand-alone program tests/cpp/slhdsa_host_check.cpp, and its output is compared with the pure-Python model
(tests/helpers/slhdsa_model.py): KeyGen of the three f sets, Verify of every signature of the shared fixture (all six sets, the message lengths around
the block edge of H_msg among them), one tampered signature per region, the digest split with an all-0xFF idx_tree for each set, and the WOTS+ digits.
A second build of the same program with -fsanitize=address,undefined runs the 128f cases; it is a program of its own, nothing loaded into Python runs
under a sanitizer.  This is the second, independent restatement that pins the model; the device is compared with the model in
tests/test_gpu_slhdsa.py."""
import os
import shutil
import subprocess

import pytest

from tests.helpers import slhdsa_cases as K
from tests.helpers import slhdsa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "slhdsa_host_check.cpp")
F128 = "SLH-DSA-SHAKE-128f"


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host check of the SLH-DSA core"
    out = str(tmp / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slhdsa_host_check")
    return {"plain": _build(tmp, "check", []), "san": _build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), "tmp": tmp}


@pytest.fixture(scope="session")
def fixture():
    return K.fixture()


def _run(programs, which, lines, tag):
    path = programs["tmp"] / f"{tag}.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([programs[which], str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (tag, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (tag, len(got), len(lines))
    return got


def _hex(b):
    return b.hex() if b else "-"


def _keygen_case(name, i=0):
    ks = K.keys(name, K.distinct(name))
    return (f"keygen {M.IDS[name]} {ks['sk_seed'][i].hex()} {ks['sk_prf'][i].hex()} {ks['pk_seed'][i].hex()}", ks["pk"][i].hex() + " " + ks["sk"][i].hex())


def _verify_case(name, pk, msg, sig):
    return (f"verify {M.IDS[name]} {pk.hex()} {_hex(msg)} {sig.hex()}", str(int(K.expect(name, pk, msg, sig))))


def _tampered_cases(name):
    pk, msg, sig = K.signed(name)[0]
    cases = [_verify_case(name, pk, msg, K.flip(sig, pos, pos % 8)) for _, pos in K.region_positions(name)]
    cases.append(_verify_case(name, pk, K.flip(msg, len(msg) - 1, 7), sig))
    cases.append(_verify_case(name, K.flip(pk, 0), msg, sig))
    cases.append(_verify_case(name, K.flip(pk, len(pk) - 1, 7), msg, sig))
    assert all(want == "0" for _, want in cases)
    return cases


def _check(programs, which, cases, tag):
    got = _run(programs, which, [c for c, _ in cases], tag)
    bad = [(i, cases[i][0][:40]) for i in range(len(cases)) if got[i] != cases[i][1]]
    assert not bad, (tag, bad[:8])


def test_keygen_of_the_f_sets_equals_the_model(programs):
    _check(programs, "plain", [_keygen_case(name, i) for name in K.F_SETS for i in range(3)], "keygen")


def test_verify_of_every_fixture_signature(programs, fixture):
    cases = [_verify_case(name, *t) for name in M.NAMES for t in fixture["signed"][name]]
    cases += [_verify_case(name, *t) for name in K.EDGE_SETS for t in fixture["edge"][name].values()]
    assert all(want == "1" for _, want in cases) and len(cases) == 3 * 3 + 3 + 8
    # each signature under the key of another instance of its set, and with the message of another
    for name in K.F_SETS:
        (pk0, m0, s0), (pk1, m1, s1) = fixture["signed"][name][:2]
        cases += [_verify_case(name, pk1, m0, s0), _verify_case(name, pk0, m1, s0)]
    _check(programs, "plain", cases, "verify")


@pytest.mark.parametrize("name", [F128, "SLH-DSA-SHAKE-256f"])
def test_one_tampered_signature_per_region(programs, name):
    _check(programs, "plain", _tampered_cases(name), "tampered_" + name[-4:])


def test_the_digest_split_and_the_digits(programs):
    lines, want = [], []
    for name in M.NAMES:
        s = M.PARAMS[name]
        c1, c2, c3 = -(-s.k * s.a // 8), -(-(s.h - s.hp) // 8), -(-s.hp // 8)
        digests = [bytes(c1) + bytes([0xFF] * c2) + bytes(c3), bytes([0xFF] * s.m), bytes(range(7, 7 + s.m)), bytes((37 * i + 11) % 256 for i in range(s.m))]
        for d in digests:
            md, idx_tree, idx_leaf = M.split_digest(name, d)
            lines.append(f"split {M.IDS[name]} {d.hex()}")
            want.append(" ".join(str(v) for v in [idx_tree, idx_leaf] + M.base_2b(md, s.a, s.k)))
        assert M.split_digest(name, digests[0])[1] == (1 << (s.h - s.hp)) - 1
        for m1 in (bytes(s.n), bytes([0xFF] * s.n), bytes((29 * i + 3) % 256 for i in range(s.n)), bytes([0x0F] * s.n), bytes([0xF0] * s.n)):
            lines.append(f"digits {M.IDS[name]} {m1.hex()}")
            want.append(" ".join(str(v) for v in M.wots_digits(name, m1)))
    got = _run(programs, "plain", lines, "split")
    assert got == want, [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w][:4]
    assert want[9 * 5].split()[0] == str((1 << 64) - 1)                    # 256f: the first of the nine cases of the sixth set, all 64 bits of idx_tree


def test_the_128f_cases_under_address_and_undefined_behaviour_sanitizers(programs, fixture):
    name = F128
    cases = [_keygen_case(name, 0)] + [_verify_case(name, *t) for t in fixture["signed"][name]] + [_verify_case(name, *t) for t in fixture["edge"][name].values()]
    cases += _tampered_cases(name)[:12]
    s = M.PARAMS[name]
    d = bytes(-(-s.k * s.a // 8)) + bytes([0xFF] * 8) + bytes(1)
    md, idx_tree, idx_leaf = M.split_digest(name, d)
    cases.append((f"split {M.IDS[name]} {d.hex()}", " ".join(str(v) for v in [idx_tree, idx_leaf] + M.base_2b(md, s.a, s.k))))
    d = bytes([0xFF] * 49)                                                 # and the shift-free mask of 256f
    md, idx_tree, idx_leaf = M.split_digest("SLH-DSA-SHAKE-256f", d)
    cases.append((f"split 5 {d.hex()}", " ".join(str(v) for v in [idx_tree, idx_leaf] + M.base_2b(md, 9, 35))))
    _check(programs, "san", cases, "san")
