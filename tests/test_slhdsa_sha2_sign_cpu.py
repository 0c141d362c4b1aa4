"""The signing part of the FIPS 205 core for the SHA-2 sets (tools_amd/csrc/psf_slhdsa_sha2_sign_core.hpp) on the CPU: g++ compiles the text the device
kernels compile, over the plain C++ back end, into the stand-alone program tests/cpp/slhdsa_sha2_sign_host_check.cpp, which signs by the decomposition of
the kernels (HMAC from two key blocks in registers, FORS subtrees and tops, all layers from the digest, trees packed 512 / 2^h' to a block, recomputed
WOTS+ values).  Its output is compared byte for byte with the pure-Python model: the hedged signatures of the shared fixture on the three f sets and on
SHA2-128s, and the deterministic messages around the block edges of H_msg; PRF_msg alone against hmac at the padding edges of its inner hash; and the
number of SHA-256 and SHA-512 compressions of every signature against the closed formulas of DESIGN.md "SLH-DSA: signing for the SHA-2 sets".  A second
build with -fsanitize=address,undefined runs the 128f and 256f cases; it is a program of its own, nothing loaded into Python runs under a sanitizer.  The
helper exact_by_parts, which the device tests rely on, is checked here against the fixture and against tampered signatures."""
import hashlib
import hmac
import os
import random
import shutil
import subprocess

import pytest

from tests.helpers import slhdsa_sha2_cases as K
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers import slhdsa_sha2_sign_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "slhdsa_sha2_sign_host_check.cpp")
S128 = "SLH-DSA-SHA2-128s"
SETS = K.F_SETS + [S128]


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host check of the SLH-DSA SHA-2 signing core"
    out = str(tmp / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slhdsa_sha2_sign_host_check")
    return {"plain": _build(tmp, "check", []), "san": _build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), "tmp": tmp}


def _hex(b):
    return b.hex() if b else "-"


def _ceil(a, b):
    return -(-a // b)


def prf_counts(name, msg_len):
    """(SHA-256, SHA-512) compressions of PRF_msg: the two key blocks, the block of the outer hash, and opt_rand || M with its padding"""
    n = M.PARAMS[name].n
    return (3 + _ceil(n + msg_len + 9, 64), 0) if n == 16 else (0, 3 + _ceil(n + msg_len + 17, 128))


def sign_counts(name, msg_len, digits):
    """(SHA-256, SHA-512) compressions of one signature with the midstate made once per stage, as DESIGN.md writes them; `digits`: the sum of the d len
    signed WOTS+ digits, the one term that depends on the data"""
    s = M.PARAMS[name]
    n, ln, leaves = s.n, M.wots_len(name)[2], 1 << s.hp
    top = 1 if s.a > 9 else 0
    f = 2 * (s.k << s.a) + 16 * s.d * leaves * ln + s.d * ln + digits       # PRF and F: the FORS leaves, the chain ends, the signed values
    h = s.k * ((1 << s.a) - 1) + s.d * (leaves - 1)                         # H: the FORS and the XMSS inner nodes
    if n == 16:
        t = _ceil(22 + s.k * n + 9, 64) + s.d * leaves * _ceil(22 + ln * n + 9, 64)
        h_msg = _ceil(3 * n + msg_len + 9, 64) + 3
        return prf_counts(name, msg_len)[0] + h_msg + f + h + t + 6 + top, 0
    t = _ceil(22 + s.k * n + 17, 128) + s.d * leaves * _ceil(22 + ln * n + 17, 128)
    h_msg = _ceil(3 * n + msg_len + 17, 128) + 2
    return f + 3, prf_counts(name, msg_len)[1] + h_msg + h + t + 4 + top


def _case(name, sk, msg, addrnd, sig):
    return (f"sign {M.IDS[name]} {sk.hex()} {_hex(msg)} {_hex(addrnd or b'')}", sig.hex(), (name, len(msg)))


def _check(programs, which, cases, tag):
    path = programs["tmp"] / f"{tag}.txt"
    path.write_text("\n".join(c[0] for c in cases) + "\n")
    out = subprocess.run([programs[which], str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (tag, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases), (tag, len(got), len(cases))
    for i, (g, (line, want, (name, msg_len))) in enumerate(zip(got, cases)):
        g, c256, c512, digits = g.split()
        if g != want:
            first = next(k for k in range(0, len(want), 2) if g[k:k + 2] != want[k:k + 2]) // 2
            raise AssertionError((tag, i, line[:12], "first differing byte", first))
        assert (int(c256), int(c512)) == sign_counts(name, msg_len, int(digits)), (tag, i, c256, c512, digits)


def _edge_cases(name):
    return [_case(name, sk, msg, None, sig) for sk, msg, sig in S.edge_inputs(name)]


@pytest.mark.parametrize("name", SETS)
def test_the_fixture_signatures_hedged_and_their_compression_counts(programs, name):
    _check(programs, "plain", [_case(name, *t) for t in S.hedged(name)], "hedged_" + name[-4:])


@pytest.mark.parametrize("name", K.EDGE_SETS)
def test_the_deterministic_edge_messages(programs, name):
    cases = _edge_cases(name)
    assert len(cases) == 4 and any(line.split()[3] == "-" for line, _, _ in cases)
    _check(programs, "plain", cases, "edges_" + name[-4:])


def _prf_lines(name, rng):
    n = M.PARAMS[name].n
    lines = []
    for ln in [0] + S.prf_edge_lens(name) + [301]:
        key, rnd, msg = rng.randbytes(n), rng.randbytes(n), rng.randbytes(ln)
        want = hmac.new(key, rnd + msg, hashlib.sha256 if n == 16 else hashlib.sha512).digest()[:n]
        assert want == M.Scheme(name).f.prf_msg(key, rnd, msg)
        lines.append((f"prf {M.IDS[name]} {key.hex()} {rnd.hex()} {_hex(msg)}", want.hex(), prf_counts(name, ln)))
    return lines


@pytest.mark.parametrize("which", ["plain", "san"])
def test_prf_msg_against_hmac_at_the_padding_edges(programs, which):
    """|M| = 0 (no pointer), n + |M| = 55, 56, 64 (SHA-256) or 111, 112, 128 (SHA-512), and a message of several blocks, on every set"""
    rng = random.Random(2104)
    lines = [x for name in M.NAMES for x in _prf_lines(name, rng)]
    assert [ln for ln in S.prf_edge_lens("SLH-DSA-SHA2-128f")] == [39, 40, 48] and S.prf_edge_lens("SLH-DSA-SHA2-256s") == [79, 80, 96]
    path = programs["tmp"] / f"prf_{which}.txt"
    path.write_text("\n".join(x[0] for x in lines) + "\n")
    out = subprocess.run([programs[which], str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    for g, (line, want, counts) in zip(got, lines):
        r, c256, c512 = g.split()
        assert r == want, line[:8]
        assert (int(c256), int(c512)) == counts, (line[:8], c256, c512, counts)


def test_the_edge_cases_under_address_and_undefined_behaviour_sanitizers(programs):
    f128 = K.F128
    _check(programs, "san", [_case(f128, *t) for t in S.hedged(f128)] + _edge_cases(f128) + _edge_cases(K.F256), "san")


def test_exact_by_parts_accepts_the_model_and_names_what_differs():
    for name in (K.F128, K.F256):
        sk, msg, addrnd, sig = S.hedged(name)[0]
        assert S.exact_by_parts(name, sk, msg, addrnd, sig) is None
        assert S.exact_by_parts(name, sk, msg, bytes(len(addrnd)), sig) == "R"
        assert S.exact_by_parts(name, sk, msg, None, sig) == "R"
        reg = M.regions(name)
        for lo, _ in (reg["R"], reg["fors_sk"][1], reg["fors_auth"][2], reg["wots"][3], reg["auth"][4]):
            assert S.exact_by_parts(name, sk, msg, addrnd, K.flip(sig, lo + 1, 3)) == "verify"
        assert S.exact_by_parts(name, sk, msg, addrnd, sig[:-1]) == "size"
    sk, msg, sig = S.edge_inputs(K.F128)[3]
    assert msg == b"" and S.exact_by_parts(K.F128, sk, msg, None, sig) is None
    # a signature of the same message under another SK.seed verifies under its own key but is not this key's
    ks = K.keys(K.F128, 3)
    assert S.exact_by_parts(K.F128, ks["sk"][1][:16] + ks["sk"][0][16:], msg, None, sig) in ("verify", "fors_sk0")
