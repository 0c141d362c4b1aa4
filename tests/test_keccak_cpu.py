"""The Keccak core of the library (tools_amd/csrc/psf_keccak_core.hpp) on the CPU: tests/cpp/keccak_host_check.cpp includes the same text the
device kernels compile, is built with g++ -fsanitize=address,undefined, and is compared with hashlib (the four functions on a grid of message
and digest lengths around the rates, on the aligned and the byte-wise path) and with the pure-Python model (the SampleNTT parse loop, its cap, and
the CBD bit fields)."""
import hashlib
import os
import random
import subprocess

import pytest

from tests.helpers import fips203_kpke_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = [(hashlib.sha3_256, 136, 32), (hashlib.sha3_512, 72, 64), (hashlib.shake_128, 168, 0), (hashlib.shake_256, 136, 0)]
FOUR_BLOCK_INPUT = bytes(range(32)) + bytes([62, 5])


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keccak") / "keccak_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "keccak_host_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return go


def test_four_functions_against_hashlib(run):
    rng = random.Random(7)
    lines, want = [], []
    for func, (h, rate, fixed) in enumerate(FUNCS):
        for in_len in (0, 1, rate - 2, rate - 1, rate, rate + 1, 2 * rate - 1, 2 * rate, 1600):
            msg = bytes(rng.randrange(256) for _ in range(in_len))
            for out_len in ([fixed] if fixed else [1, rate - 1, rate, rate + 1, 3 * rate + 5]):
                for off in (0, 3):                                      # 8-byte groups as one access, and byte by byte
                    lines.append(f"hash {func} {msg.hex() or '-'} {out_len} {off}")
                    want.append(h(msg).hexdigest() if fixed else h(msg).hexdigest(out_len))
    assert run(lines) == want


def test_parse_routines_against_the_model_on_random_inputs(run):
    rng = random.Random(8)
    lines, want = [], []
    for _ in range(200):
        seed = bytes(rng.randrange(256) for _ in range(34))
        lines.append(f"ntt {seed.hex()} 8")
        want.append(" ".join(map(str, [0] + M.sample_ntt(seed))))
    for i in range(200):
        eta, nonce = 2 + (i & 1), rng.randrange(256)
        sigma = bytes(rng.randrange(256) for _ in range(32))
        lines.append(f"cbd {eta} {sigma.hex()} {nonce}")
        want.append(" ".join(map(str, M.sample_poly_cbd(eta, M.PRF(eta, sigma, nonce)))))
    assert run(lines) == want


def test_four_block_input_and_the_cap(run):
    """rho = 0 ... 31, j = 62, i = 5 needs four SHAKE128 blocks; with the cap at 3 blocks the flag is raised and the tail is zero"""
    coef, blocks, _ = M.sample_ntt_blocks(FOUR_BLOCK_INPUT)
    assert blocks == 4
    full, capped = run([f"ntt {FOUR_BLOCK_INPUT.hex()} 8", f"ntt {FOUR_BLOCK_INPUT.hex()} 3"])
    assert [int(v) for v in full.split()] == [0] + coef
    got = [int(v) for v in capped.split()]
    want, _, failed = M.sample_ntt_blocks(FOUR_BLOCK_INPUT, 3)
    assert failed and got == [1] + want
    short = next(i for i in range(256) if want[i:] == [0] * (256 - i))
    assert 0 < short < 256 and got[1 + short:] == [0] * (256 - short) and got[1:1 + short] == coef[:short]
    exact4 = run([f"ntt {FOUR_BLOCK_INPUT.hex()} 4"])[0]
    assert [int(v) for v in exact4.split()] == [0] + coef             # the cap itself is not a failure when the last block completes the polynomial
