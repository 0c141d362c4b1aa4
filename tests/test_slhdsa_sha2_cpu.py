"""The FIPS 205 section 11.2 core of the library (tools_amd/csrc/psf_slhdsa_sha2_core.hpp over psf_sha2_core.hpp) on the CPU: g++ compiles the text the
device kernels compile, over the plain C++ back end, into the stand-alone program tests/cpp/slhdsa_sha2_host_check.cpp, and its output is compared with
the pure-Python model (tests/helpers/slhdsa_sha2_model.py): KeyGen of the three f sets, Verify of every signature of the shared fixture (all six sets,
the message lengths around the padding edges of H_msg among them), one tampered signature per region on SHA2-128f and SHA2-256f, the digest split and
the WOTS+ digits, and the number of SHA-256 and SHA-512 compressions of one KeyGen and one Verify per set against the closed formulas of DESIGN.md
("SLH-DSA: the SHA-2 sets") -- which is what shows that the PK.seed block is compressed once per stage and never inside a chain or path loop.
A second build of the same program with -fsanitize=address,undefined runs the 128f and 192f cases; it is a program of its own, nothing loaded into
Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

from tests.helpers import slhdsa_sha2_cases as K
from tests.helpers import slhdsa_sha2_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "slhdsa_sha2_host_check.cpp")


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host check of the SLH-DSA SHA-2 core"
    out = str(tmp / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slhdsa_sha2_host_check")
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
    cases.append(_verify_case(K.F256, *K.full_tree_signed()))
    assert all(want == "1" for _, want in cases) and len(cases) == 3 * 3 + 3 + 8 + 1
    # each signature under the key of another instance of its set, and with the message of another
    for name in K.F_SETS:
        (pk0, m0, s0), (pk1, m1, s1) = fixture["signed"][name][:2]
        cases += [_verify_case(name, pk1, m0, s0), _verify_case(name, pk0, m1, s0)]
    _check(programs, "plain", cases, "verify")


def test_the_edge_lengths_are_the_padding_edges():
    assert [48 + ln for ln in K.edge_lens(K.F128)[:3]] == [55, 56, 64] and K.edge_lens(K.F128)[3] == 0
    assert [96 + ln for ln in K.edge_lens(K.F256)[:3]] == [111, 112, 128] and K.edge_lens(K.F256)[3] == 0


@pytest.mark.parametrize("name", [K.F128, K.F256])
def test_one_tampered_signature_per_region(programs, name):
    _check(programs, "plain", _tampered_cases(name), "tampered_" + name[-4:])


def test_the_digest_split_and_the_digits(programs):
    lines, want = [], []
    for name in M.NAMES:
        s = M.PARAMS[name]
        c1, c2, c3 = -(-s.k * s.a // 8), -(-(s.h - s.hp) // 8), -(-s.hp // 8)
        for d in (bytes(c1) + bytes([0xFF] * c2) + bytes(c3), bytes([0xFF] * s.m), bytes((37 * i + 11) % 256 for i in range(s.m))):
            md, idx_tree, idx_leaf = M.split_digest(name, d)
            lines.append(f"split {M.IDS[name]} {d.hex()}")
            want.append(" ".join(str(v) for v in [idx_tree, idx_leaf] + M.base_2b(md, s.a, s.k)))
        for m1 in (bytes(s.n), bytes([0xFF] * s.n), bytes((29 * i + 3) % 256 for i in range(s.n))):
            lines.append(f"digits {M.IDS[name]} {m1.hex()}")
            want.append(" ".join(str(v) for v in M.wots_digits(name, m1)))
    got = _run(programs, "plain", lines, "split")
    assert got == want, [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w][:4]


# ---- compressions per operation: the closed formulas of DESIGN.md "SLH-DSA: the SHA-2 sets" -----------------------------------------------------------------

def t_blocks(n, words):
    """blocks of T_l past the midstate over l = `words` n-byte strings: ADRSc, the message, the 0x80 and the length in blocks of 64 (n = 16) or 128 bytes"""
    block, pad = (64, 9) if n == 16 else (128, 17)
    return -(-(22 + words * n + pad) // block)


def keygen_compressions(name):
    """(SHA-256, SHA-512) of one slh_keygen_internal: three stages, each with the midstate(s) it needs made once"""
    s = M.PARAMS[name]
    leaves, ln = 1 << s.hp, M.wots_len(name)[2]
    chains = 1 + leaves * ln * 16                                          # the midstate; PRF and 15 F per chain
    t_and_h = (1 + leaves * t_blocks(s.n, ln)) + (1 + leaves - 1)          # the leaf stage and the tree stage, a midstate each
    return (chains + t_and_h, 0) if s.n == 16 else (chains, t_and_h)


def chain_steps(name, pk, msg, sig):
    """the F calls of wots_pkFromSig over the d layers of this signature: sum of 15 - digit, the messages of the layers from the model"""
    s, n = M.PARAMS[name], M.PARAMS[name].n
    sch = M.Scheme(name)
    ln = M.wots_len(name)[2]
    md, idx_tree, idx_leaf = M.split_digest(name, sch.f.h_msg(sig[:n], pk[:n], pk[n:], msg))
    fors_len = s.k * (1 + s.a) * n
    node = sch.fors_pk_from_sig(sig[n:n + fors_len], md, pk[:n], sch._fors_adrs(idx_tree, idx_leaf))
    ht, step, total = sig[n + fors_len:], (s.hp + ln) * n, 0
    adrs = M.Adrs()
    for j in range(s.d):
        total += sum(15 - d for d in M.wots_digits(name, node))
        adrs.set_layer(j)
        adrs.set_tree(idx_tree)
        node = sch.xmss_pk_from_sig(idx_leaf, ht[j * step:(j + 1) * step], node, pk[:n], adrs)
        idx_leaf = idx_tree % (1 << s.hp)
        idx_tree >>= s.hp
    assert node == pk[n:]
    return total


def verify_compressions(name, msg_len, steps):
    """(SHA-256, SHA-512) of one slh_verify_internal whose d WOTS+ signatures need `steps` chain steps in all"""
    s = M.PARAMS[name]
    n, ln = s.n, M.wots_len(name)[2]
    if n == 16:
        digest = -(-(3 * n + msg_len + 9) // 64) + 3                       # the inner hash; the MGF1 seed block, shared; two counters
        fors = 1 + s.k + s.k * s.a                                         # the midstate; F per tree; H per level
        fors_pk = 1 + t_blocks(n, s.k)
        layers = s.d * ((1 + 0) + (1 + t_blocks(n, ln) + s.hp))            # chains: the midstate (+ steps); T_len and the path: the midstate, blocks, H
        return digest + fors + fors_pk + layers + steps, 0
    digest = -(-(3 * n + msg_len + 17) // 128) + -(-(2 * n + 68 + 17) // 128)
    return (1 + s.k) + s.d + steps, digest + (1 + s.k * s.a) + (1 + t_blocks(n, s.k)) + s.d * (1 + t_blocks(n, ln) + s.hp)


def test_block_counts_past_the_midstate():
    assert [t_blocks(n, 2 * n + 3) for n in (16, 24, 32)] == [10, 10, 18]
    assert [t_blocks(M.PARAMS[name].n, M.PARAMS[name].k) for name in M.NAMES] == [4, 9, 4, 7, 6, 10]
    assert 22 + 14 * 16 + 9 == 255                                         # T_k of SHA2-128s fills its fourth block to the byte


def _count_case(name, fixture):
    ks = K.keys(name, K.distinct(name))
    pk, msg, sig = fixture["signed"][name][0]
    assert pk == ks["pk"][0]
    return f"count {M.IDS[name]} {ks['sk_seed'][0].hex()} {ks['sk_prf'][0].hex()} {ks['pk_seed'][0].hex()} {pk.hex()} {_hex(msg)} {sig.hex()}"


def test_compressions_per_operation_equal_the_closed_formulas(programs, fixture):
    got = _run(programs, "plain", [_count_case(name, fixture) for name in M.NAMES], "count")
    for name, line in zip(M.NAMES, got):
        pk, msg, sig = fixture["signed"][name][0]
        want = keygen_compressions(name) + verify_compressions(name, len(msg), chain_steps(name, pk, msg, sig)) + (1,)
        assert tuple(int(v) for v in line.split()) == want, (name, line, want)


def test_the_128f_and_192f_cases_under_address_and_undefined_behaviour_sanitizers(programs, fixture):
    cases = []
    for name in (K.F128, K.F192):
        cases += [_keygen_case(name, 0)] + [_verify_case(name, *t) for t in fixture["signed"][name]]
        cases += _tampered_cases(name)[:12]
    cases += [_verify_case(K.F128, *t) for t in fixture["edge"][K.F128].values()]
    _check(programs, "san", cases, "san")
