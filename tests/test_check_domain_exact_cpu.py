"""check_domain decided as the reference decides it -- exact rationals (mp_perturbation.rs:396-402, gpv.rs:219-224, gpv_ring.rs:274-283) -- on the CPU oracle,
and the library's host-side bound (psf::domain_bound_exact) against the same arithmetic.

Every expected value is a Python int / Fraction (tests/helpers/domain_cases.py); none comes from the oracle.  Until this test existed the bound was formed in
rounded doubles ((s*s)*m)*(r*r) and the norm was converted to a double: at n = 8, q = 128 (m = 121), r = 3.0, s = 24.98853731704157 the exact bound has floor
680000 and the rounded one is 680001.0, so a row of norm 680001 was accepted; a row of four entries -2^63 (norm 2^128) wrapped to 0 and was accepted."""
import ctypes as C
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import domain_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["psfp-121", "psfp-537", "gpv", "ring"]


def make(oracle, kind, s, r=3.0):
    """(handle, m, r as it enters the bound)"""
    if kind == "psfp-121":
        h = oracle.PSFPerturbation(oracle.gadget_params_default(8, 128), r, s, with_L=False)
        return h, h.m, r
    if kind == "psfp-537":
        h = oracle.PSFPerturbation(oracle.gadget_params_default(32, 256), r, s, with_L=False)
        return h, h.m, r
    if kind == "gpv":
        h = oracle.PSFGPV(oracle.gadget_params_default(6, 128), s)
        return h, h.m, 1.0
    h = oracle.PSFGPVRing(oracle.gadget_params_ring_default(8, 257), s, 1.005)
    return h, h.d, 1.0


def check_rows(h, rows, exp, what):
    """the rows in one call, then the four rows around the bound (and every row of a small set) one by one"""
    got = h.check_domain(rows)
    assert got.shape == exp.shape
    assert (got == exp).all(), f"{what}: rows {np.nonzero(got != exp)[0].tolist()[:8]} differ from the exact decision"
    for i in range(len(rows)):
        assert bool(h.check_domain(rows[i:i + 1].copy())[0]) == bool(exp[i]), f"{what}: single row {i}"


def test_sizes(oracle):
    assert make(oracle, "psfp-121", 25.0)[1] == 121 and make(oracle, "psfp-537", 25.0)[1] == 537


@pytest.mark.parametrize("kind", KINDS)
def test_on_the_bound_in_both_directions(oracle, kind):
    """at least 20 (K, s) of each kind per type: the rounded bound admits floor(B) + 1, or refuses floor(B)"""
    m = make(oracle, kind, 25.0)[1]
    rs = (3.0, 3.3, math.log2(6)) if kind == "psfp-121" else (3.0,) if kind == "psfp-537" else (1.0,)
    for r in rs:
        acc, rej = dc.on_the_bound_pairs(m, r, count=20)
        for tag, ss in (("rounded bound accepts floor(B)+1", acc), ("rounded bound rejects floor(B)", rej)):
            for s in ss:
                h, _, r_eff = make(oracle, kind, s, r)
                assert r_eff == r
                fb = dc.floor_bound(s, r, m)
                norms = dc.window_norms(fb)
                rows = dc.rows_array([dc.row_with_norm(N, m, salt=i) for i, N in enumerate(norms)])
                exp = dc.expected(norms, fb)
                assert len(rows) >= 70 and exp[norms.index(fb)] and not exp[norms.index(fb + 1)]
                got = h.check_domain(rows)
                assert (got == exp).all(), f"{kind} r={r} s={s!r} ({tag}): norms {[norms[i] - fb for i in np.nonzero(got != exp)[0]]} relative to floor(B)"
                for d in (-1, 0, 1, 2):
                    i = norms.index(fb + d)
                    assert bool(h.check_domain(rows[i:i + 1].copy())[0]) == (d <= 0), (kind, r, s, d)


def large_s_values(m, r):
    """s whose bound has 60-75 bits and 120-127 bits, mantissas with low bits set"""
    out = [2.0**30 + 0.37, 2.0**26 + 0.1, 2.0**32 * 1.2345678901234567]
    mr2 = math.log2(m * r * r)
    for bits in (120.5, 124.0, 126.9):
        e = (bits - mr2) / 2
        out.append(math.ldexp(1.0 + 0.123456789 * (bits - 119) / 8, 0) * 2.0 ** e)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_bounds_of_60_to_75_and_120_to_127_bits(oracle, kind):
    m = make(oracle, kind, 25.0)[1]
    r = 3.3 if kind.startswith("psfp") else 1.0
    seen = []
    for s in large_s_values(m, r):
        h, _, _ = make(oracle, kind, s, r)
        fb = dc.floor_bound(s, r, m)
        seen.append(fb.bit_length())
        norms = dc.window_norms(fb) + dc.carry_norms(fb)
        rows = dc.rows_array([dc.row_with_norm(N, m, salt=i) for i, N in enumerate(norms)])
        exp = dc.expected(norms, fb)
        assert exp.any() and not exp.all()
        check_rows(h, rows, exp, f"{kind} s={s!r} ({fb.bit_length()}-bit bound)")
    assert any(60 <= b <= 75 for b in seen) and any(120 <= b <= 127 for b in seen), seen


def test_issue_examples(oracle):
    """the four examples of the issue at n = 8, q = 128"""
    h, m, r = make(oracle, "psfp-121", 24.98853731704157, 3.0)
    assert dc.floor_bound(24.98853731704157, 3.0, m) == 680000 and dc.double_bound(24.98853731704157, 3.0, m) == 680001.0
    assert not h.check_domain(dc.rows_array([dc.row_with_norm(680001, m)]))[0]
    assert h.check_domain(dc.rows_array([dc.row_with_norm(680000, m)]))[0]
    wrap = np.zeros(m, dtype=np.int64)
    wrap[:4] = -2**63
    assert not h.check_domain(wrap)[0]
    s, r = 2.0**30 + 0.37, 3.3
    h, m, _ = make(oracle, "psfp-121", s, r)
    fb = dc.floor_bound(s, r, m)
    assert fb.bit_length() == 71
    got = h.check_domain(dc.rows_array([dc.row_with_norm(fb + d, m) for d in (-1, 0, 1, 2)]))
    assert got.tolist() == [True, True, False, False]


@pytest.mark.parametrize("kind", KINDS)
def test_norms_at_and_above_2_to_128(oracle, kind):
    r = 3.0 if kind.startswith("psfp") else 1.0
    # B < 2^128: every such row is rejected, mixed into one call with the rows around the bound
    h, m, _ = make(oracle, kind, 25.0, r)
    fb = dc.floor_bound(25.0, r, m)
    rows, exp, norms = dc.mixed_batch(fb, m)
    assert not exp[[i for i, N in enumerate(norms) if N >= 1 << 53]].any()
    check_rows(h, rows, exp, f"{kind} s=25")
    # B >= 2^128 (s = 2^62): norms between 2^128 and B are accepted, norms above B are rejected
    r = 1.5 if kind.startswith("psfp") else 1.0
    s = 2.0**62
    h, m, _ = make(oracle, kind, s, r)
    fb = dc.floor_bound(s, r, m)
    assert fb >= 1 << 128
    cap = (m - 8) << 126
    norms = [0, 1 << 64, (1 << 128) - 1, 1 << 128, (1 << 128) + 1, (fb + (1 << 128)) // 2] + dc.window_norms(fb, -3, 3) + dc.carry_norms(fb)
    norms = [N for N in norms if N <= cap] + [cap]
    rows = [dc.row_with_norm(N, m, salt=i) for i, N in enumerate(norms)] + [[-2**63] * m, [2**63 - 1] * m]
    norms += [m << 126, m * (2**63 - 1) ** 2]
    exp = dc.expected(norms, fb)
    assert exp[norms.index(1 << 128)] and exp[norms.index((fb + (1 << 128)) // 2)] and not exp[norms.index(fb + 1)] and not exp[-2]
    check_rows(h, dc.rows_array(rows), exp, f"{kind} s=2^62")


@pytest.mark.parametrize("kind", KINDS)
def test_other_lengths_and_a_zero_bound(oracle, kind):
    r = 3.0 if kind.startswith("psfp") else 1.0
    h, m, _ = make(oracle, kind, 25.0, r)
    for ln in (m - 1, m + 1, 1):
        assert not h.check_domain(np.zeros((1, ln), dtype=np.int64)).any()
    assert h.check_domain(np.zeros((1, m), dtype=np.int64)).all()
    s = 2.0**-8                                       # s^2 m r^2 < 1: floor(B) = 0, the zero vector is the whole domain
    h, m, _ = make(oracle, kind, s, r)
    assert dc.floor_bound(s, r, m) == 0
    rows = np.zeros((3, m), dtype=np.int64)
    rows[1, m - 1] = 1
    rows[2, 0] = -1
    assert h.check_domain(rows).tolist() == [True, False, False]


def test_f_a_reports_the_exact_decision(oracle):
    """the assert! inside f_a (mp_perturbation.rs:367, gpv.rs:191) is the same test"""
    s, r = 24.98853731704157, 3.0
    h, m, _ = make(oracle, "psfp-121", s, r)
    h.f_a(dc.rows_array([dc.row_with_norm(680000, m)]))
    with pytest.raises(AssertionError):
        h.f_a(dc.rows_array([dc.row_with_norm(680000, m), dc.row_with_norm(680001, m)]))
    acc, rej = dc.on_the_bound_pairs(make(oracle, "gpv", 25.0)[1], 1.0, count=1)
    for s in acc + rej:
        g, m, _ = make(oracle, "gpv", s)
        fb = dc.floor_bound(s, 1.0, m)
        g.f_a(dc.rows_array([dc.row_with_norm(fb, m)]))
        with pytest.raises(AssertionError):
            g.f_a(dc.rows_array([dc.row_with_norm(fb + 1, m)]))


def bound_triples():
    rnd = random.Random(5)
    out = [(25.0, 3.0, 121), (24.98853731704157, 3.0, 121), (2.0**30 + 0.37, 3.3, 121), (2.0**62, 1.0, 537), (2.0**62, 1.5, 121), (2.0**-8, 3.0, 121),
           (5e-324, 1.0, 1), (5e-324, 2.0**500, 2**64 - 1), (1.7976931348623157e308, 1.0, 1), (2.0**34, 2.0**34, 2**56 - 1), (2.0**34, 2.0**34, 2**56),
           (2.0**34, 2.0**34, 2**56 + 1), (math.nextafter(2.0**48, 0), math.nextafter(2.0**48, 0), 1), (2.0**48, 2.0**48, 1), (1.0, 1.0, 2**64 - 1)]
    for _ in range(3000):
        e = rnd.choice([rnd.uniform(-40, 70), rnd.uniform(-2, 30), rnd.uniform(-1070, 1020)])
        s = math.ldexp(rnd.uniform(1, 2), int(e))
        r = rnd.choice([1.0, 3.0, 3.3, math.log2(6), math.ldexp(rnd.uniform(1, 2), rnd.randint(-30, 30))])
        out.append((s, r, rnd.choice([1, 121, 537, rnd.randrange(1, 2**20), rnd.randrange(1, 2**64)])))
    return out


def exact_limbs(s, r, m):
    return min(math.floor(Fraction(s) ** 2 * m * Fraction(r) ** 2), 2**192 - 1)


def test_oracle_bound_limbs_are_the_exact_floor(oracle):
    L = oracle.lib()
    L.orc_domain_bound_limbs.argtypes = [C.c_double, C.c_double, C.c_uint64, C.POINTER(C.c_uint64)]
    L.orc_domain_bound_limbs.restype = None
    out = (C.c_uint64 * 3)()
    for s, r, m in bound_triples():
        L.orc_domain_bound_limbs(s, r, m, out)
        assert out[0] | (out[1] << 64) | (out[2] << 128) == exact_limbs(s, r, m), (s, r, m)


def test_library_bound_limbs_are_the_exact_floor():
    """psf::domain_bound_exact, what every k_check_domain launch is handed, built for the CPU under AddressSanitizer + UndefinedBehaviorSanitizer"""
    src = os.path.join(ROOT, "tests", "cpp", "domain_bound_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "domain_bound_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    triples = bound_triples()
    text = "".join(f"{s.hex()} {r.hex()} {m}\n" for s, r, m in triples)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    got = [int(line, 16) for line in run.stdout.split()]
    assert len(got) == len(triples)
    for (s, r, m), g in zip(triples, got):
        assert g == exact_limbs(s, r, m), (s, r, m)
