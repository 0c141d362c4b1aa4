"""The FIPS 204 core of the library (tools_amd/csrc/psf_mldsa_core.hpp) on the CPU: tests/cpp/mldsa_host_check.cpp includes the same text the device
kernels compile, is built with g++ -fsanitize=address,undefined as a program of its own, and is compared with the pure-Python model: the three parse
loops (on random seeds, on searched seeds whose streams reject in the first and in the last block needed or need a block more than usual, and at
their caps), HintBitUnpack on valid and on every malformed shape, Power2Round, Decompose and UseHint for both gamma2 on random and edge residues, and
every packing at its extreme field values."""
import os
import random
import subprocess

import pytest

from tests.helpers import mldsa_cases as K
from tests.helpers import mldsa_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = M.Q
G2 = ((Q - 1) // 88, (Q - 1) // 32)
# packing number of kPackTable: (bits, a, b) of BitPack(w, a, b), or (bits, None, top) of SimpleBitPack
PACKINGS = {0: (10, None, 1023), 1: (13, 4095, 4096), 2: (3, 2, 2), 3: (4, 4, 4), 4: (18, (1 << 17) - 1, 1 << 17), 5: (20, (1 << 19) - 1, 1 << 19),
            6: (6, None, 43), 7: (4, None, 15)}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mldsa") / "mldsa_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "mldsa_host_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return go


def _poly(flag, coef):
    return " ".join(str(v) for v in [flag] + list(coef))


def test_searched_seeds_have_their_properties():
    K.check()


def test_rej_ntt_poly(run):
    rng = random.Random(41)
    seeds = [rng.randbytes(34) for _ in range(24)] + K.NTT_REJECTS_FIRST_AND_LAST
    assert run([f"ntt {s.hex()} 8" for s in seeds]) == [_poly(0, M.rej_ntt_poly(s)) for s in seeds]
    # the stream needs five blocks: at a cap of five nothing changes, at four the tail is zero and the flag is raised
    s = K.NTT_REJECTS_FIRST_AND_LAST[0]
    full, capped = run([f"ntt {s.hex()} 5", f"ntt {s.hex()} 4"])
    want = M.rej_ntt_poly(s)
    assert full == _poly(0, want)
    got = [int(v) for v in capped.split()]
    have = 4 * 56 - 1                                                      # one of the 224 candidates of four blocks was rejected
    assert got[0] == 1 and got[1:1 + have] == want[:have] and got[1 + have:] == [0] * (256 - have)


def test_rej_bounded_poly(run):
    rng = random.Random(42)
    cases = [(eta, rng.randbytes(66)) for eta in (2, 4) for _ in range(16)]
    cases += [(2, K.BOUNDED2_ONE_BLOCK + bytes(2)), (2, K.BOUNDED2_TWO_BLOCKS + bytes(2)), (4, K.BOUNDED4_TWO_BLOCKS + bytes(2)),
              (4, K.BOUNDED4_THREE_BLOCKS + bytes(2))]
    assert run([f"bounded {eta} {s.hex()} 8" for eta, s in cases]) == [_poly(0, M.rej_bounded_poly(s, eta)) for eta, s in cases]
    # the three-block stream at a cap of two: the coefficients of two blocks, zeros, and the flag
    s = K.BOUNDED4_THREE_BLOCKS + bytes(2)
    st = {}
    want = M.rej_bounded_poly(s, 4, st)
    have = 2 * 272 - st["rejected"][0] - st["rejected"][1]
    assert have < 256
    got = [int(v) for v in run([f"bounded 4 {s.hex()} 2"])[0].split()]
    assert got[0] == 1 and got[1:1 + have] == want[:have] and got[1 + have:] == [0] * (256 - have)
    assert run([f"bounded 4 {s.hex()} 3"]) == [_poly(0, want)]


def test_sample_in_ball(run):
    rng = random.Random(43)
    cases = [(tau, rng.randbytes(n)) for tau, n in ((39, 32), (49, 48), (60, 64), (1, 32), (64, 64), (17, 5)) for _ in range(8)]
    lines, want = [], []
    for tau, ct in cases:
        st = {}
        c = M.sample_in_ball(ct, tau, st)
        assert st["blocks"] == 1 and (tau < 39 or st["bytes"] > 8 + tau)  # a candidate was rejected in the one block needed
        assert sum(1 for v in c if v) == tau and set(c) <= {-1, 0, 1}
        lines.append(f"ball {tau} {ct.hex()} 8")
        want.append(_poly(0, c))
    assert run(lines) == want
    assert run([f"ball 60 {cases[20][1].hex()} 1"]) == [want[20]]          # one block is enough: the cap of one is not reached


def _masks(h):
    return bytes(sum(p[8 * b + i] << i for i in range(8)) for p in h for b in range(32)).hex()


def malformed_hints(k, omega, rng):
    """a valid hint encoding and the four malformed shapes made from it"""
    while True:
        h = [[0] * 256 for _ in range(k)]
        for j in rng.sample(range(k * 256), omega - 3):
            h[j // 256][j % 256] = 1
        counts = [sum(p) for p in h]
        if counts[0] >= 2 and counts[1] >= 1:
            break
    y = M.hint_bit_pack(h, omega)
    below = bytearray(y)
    below[omega + 1] = y[omega] - 1                                        # a count byte below the running index
    above = bytearray(y)
    above[omega + k - 1] = omega + 1                                       # a count byte above omega
    order = bytearray(y)
    order[1] = order[0]                                                    # two equal indices inside the first polynomial
    tail = bytearray(y)
    tail[omega - 1] = 1                                                    # a non-zero byte after the last index
    return h, y, [bytes(below), bytes(above), bytes(order), bytes(tail)]


def test_hint_bit_unpack(run):
    rng = random.Random(44)
    lines, want = [], []
    for name, (k, l, eta, tau, cb, g1, g2, beta, omega) in M.PARAMS.items():
        h, y, bad = malformed_hints(k, omega, rng)
        assert M.hint_bit_unpack(y, k, omega) == h
        lines.append(f"hint {k} {omega} {y.hex()}")
        want.append("1 " + _masks(h))
        for b in bad:
            assert M.hint_bit_unpack(b, k, omega) is None
            lines.append(f"hint {k} {omega} {b.hex()}")
        # indices that descend across the boundary between two polynomials are valid
        h2 = [[0] * 256 for _ in range(k)]
        h2[0][200], h2[0][250], h2[1][3], h2[1][100] = 1, 1, 1, 1
        y2 = M.hint_bit_pack(h2, omega)
        assert M.hint_bit_unpack(y2, k, omega) == h2
        lines.append(f"hint {k} {omega} {y2.hex()}")
        want.append("1 " + _masks(h2))
        empty = bytes(omega + k)
        lines.append(f"hint {k} {omega} {empty.hex()}")
        want.append("1 " + _masks([[0] * 256 for _ in range(k)]))
    out = run(lines)
    good = [o for o in out if o.startswith("1 ")]
    assert good == want
    assert sum(1 for o in out if o.startswith("0 ")) == 4 * len(M.PARAMS)


def test_rounding(run):
    rng = random.Random(45)
    rs = {0, 1, Q - 1, Q - 2, 4095, 4096, 4097, 8191, 8192, (Q - 1) // 2}
    for g2 in G2:
        m = (Q - 1) // (2 * g2)
        for i in (0, 1, m // 2, m - 1, m):
            for d in (-1, 0, 1):
                for at in (i * 2 * g2 + d, i * 2 * g2 + g2 + d):
                    if 0 <= at < Q:
                        rs.add(at)
    rs = sorted(rs) + [rng.randrange(Q) for _ in range(2000)]
    want = []
    for r in rs:
        p1, p0 = M.power2round(r)
        row = [p1, p0]
        for g2 in G2:
            row += list(M.decompose(r, g2))
        for g2 in G2:
            row += [M.use_hint(0, r, g2), M.use_hint(1, r, g2)]
        want += row
    out = run(["round " + " ".join(str(r) for r in rs)])[0]
    assert [int(v) for v in out.split()] == want


def test_packings_at_their_extremes_and_at_random(run):
    rng = random.Random(46)
    lines, want = [], []
    for which, (bits, a, b) in PACKINGS.items():
        lo, hi = (0, b) if a is None else (-a, b)
        rows = [[lo] * 8, [hi] * 8, [lo, hi] * 4, [hi, lo] * 4] + [[rng.randint(lo, hi) for _ in range(8)] for _ in range(6)]
        for vals in rows:
            w = vals * 32
            data = (M.simple_bit_pack(w, b) if a is None else M.bit_pack(w, a, b))[:bits]
            lines.append(f"pack {which} " + " ".join(str(v) for v in vals))
            want.append(data.hex())
            lines.append(f"unpack {which} {data.hex()}")
            want.append(" ".join(str(v) for v in vals))
    assert run(lines) == want
