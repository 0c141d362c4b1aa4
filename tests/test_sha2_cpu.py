"""The SHA-2 core of the library (tools_amd/csrc/psf_sha2_core.hpp) on the CPU: tests/cpp/sha2_host_check.cpp includes the same text the device kernels
compile, is built with g++ as a stand-alone program, and is compared with hashlib: SHA-256 and SHA-512 at the message lengths around every padding
edge of both (pad fits, pad spills into a block of its own, whole blocks), on the 4-byte-load path and byte by byte, and the "more blocks from a
midstate" form that FIPS 205 section 11.2 needs (a prefix of whole blocks compressed first, the rest absorbed from that state).  A second build with
-fsanitize=address,undefined runs the same cases as a program of its own: every message sits in a heap block of its exact size, so a read past its end
is a report.  Nothing loaded into Python runs under a sanitizer."""
import hashlib
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sha2_host_check.cpp")
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127, 128, 129, 200, 1000]
FUNCS = [(hashlib.sha256, 64), (hashlib.sha512, 128)]


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host check of the SHA-2 core"
    out = str(tmp / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sha2_host_check")
    return {"plain": _build(tmp, "check", []), "san": _build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), "tmp": tmp}


def _run(programs, which, lines, tag):
    path = programs["tmp"] / f"{tag}.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([programs[which], str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (tag, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (tag, len(got), len(lines))
    return got


def _hash_cases():
    rng = random.Random(11)
    lines, want = [], []
    for func, (h, _) in enumerate(FUNCS):
        for n in LENGTHS:
            msg = rng.randbytes(n)
            for off in (0, 4, 1, 3):                                       # 4-byte loads (off a multiple of 4) and byte by byte
                lines.append(f"hash {func} {msg.hex() or '-'} {off}")
                want.append(h(msg).hexdigest())
    return lines, want


def _mid_cases():
    rng = random.Random(12)
    lines, want = [], []
    for func, (h, block) in enumerate(FUNCS):
        for blocks in (1, 2):
            for n in LENGTHS:
                pre, rest = rng.randbytes(blocks * block), rng.randbytes(n)
                lines.append(f"mid {func} {pre.hex()} {rest.hex() or '-'}")
                want.append(h(pre + rest).hexdigest())
        # FIPS 205's own shapes: PK.seed || zeros, then ADRSc || M with 22 + n + 9 <= 64, 22 + 32 + 9 = 63 and 22 + 2 n + 17 <= 128
        for n in (16, 24, 32):
            seed = rng.randbytes(n)
            for tail in (22 + n, 22 + 2 * n, 22 + 14 * 16):
                rest = rng.randbytes(tail)
                pre = seed + bytes(block - n)
                lines.append(f"mid {func} {pre.hex()} {rest.hex()}")
                want.append(h(pre + rest).hexdigest())
    return lines, want


def test_both_hashes_equal_hashlib_at_every_padding_edge(programs):
    lines, want = _hash_cases()
    assert len(lines) == 2 * len(LENGTHS) * 4
    assert _run(programs, "plain", lines, "hash") == want


def test_more_blocks_from_a_midstate(programs):
    lines, want = _mid_cases()
    assert _run(programs, "plain", lines, "mid") == want


def test_a_prefix_that_is_no_whole_number_of_blocks_is_refused(programs):
    path = programs["tmp"] / "bad.txt"
    path.write_text("mid 0 " + "00" * 63 + " 00\n")
    assert subprocess.run([programs["plain"], str(path)], stdout=subprocess.PIPE).returncode == 2


def test_the_same_cases_under_address_and_undefined_behaviour_sanitizers(programs):
    lines, want = _hash_cases()
    more, want2 = _mid_cases()
    assert _run(programs, "san", lines + more, "san") == want + want2
