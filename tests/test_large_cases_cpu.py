"""No-GPU checks of what the suites past 2^32 bytes and words rest on (tests/helpers/large_cases.py and the windowed fill models of
tests/helpers/sample_fill_model.py): the windowed models equal the full models, also where a window straddles a Philox block, a word of the
centred-binomial rule and two polynomials; the period and crossing assertions hold for every shape of the four GPU files; and every listed
count passes the parameter checks of its entry point, asked through the ABI with a device number that does not exist (every check runs
before the first HIP call, which then fails: nothing is launched, with or without a GPU)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import large_cases as L
from tests.helpers import sample_fill_model as M

SEED = 0x5EED5EED12345678
ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 1, 7, 8
NO_DEVICE = 1 << 20


# ---- the windowed models ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [1, 2, 3, 5, 16])
def test_cbd_window_equals_the_full_model(eta):
    sw, bw = 16 // eta, 4 * (16 // eta)
    n, first = 7 * bw + 3, (1 << 32) - 2                                    # n no multiple of the block; indices across 2^32
    full = M.cbd_fill(SEED, 200, first, 4, n, eta)
    edges = [(0, n), (0, 1), (n - 1, n), (bw - 1, bw + 1), (sw - 1, sw + 1), (2 * bw - 2, 3 * bw + 2), (bw, 2 * bw), (n - 3, n), (5, 5)]
    for c in range(4):
        for i0, i1 in edges:
            got = M.cbd_window(SEED, 200, first + c, i0, i1, eta)
            assert got.dtype == np.int64 and np.array_equal(got, full[c, i0:i1]), (eta, c, i0, i1)


def test_cbd_window_far_into_a_long_polynomial():
    """a window at coefficient 2^32 - 600 needs no array of the polynomial's length, and equals the definition coefficient by coefficient"""
    i0 = (1 << 32) - 600
    got = M.cbd_window(SEED, 77, 9, i0, i0 + 40, 2)
    assert got.tolist() == [M.cbd_coeff(SEED, 77, 9, i, 2) for i in range(i0, i0 + 40)]


def test_uniform_window_equals_the_full_model():
    n, first, q = 37, (1 << 32) - 1, 3329
    full = M.uniform_fill(SEED, 70, first, 3, n, q)
    for c in range(3):
        for i0, i1 in [(0, n), (0, 1), (n - 1, n), (3, 29)]:
            got = M.uniform_window(SEED, 70, first + c, i0, i1, q)
            assert got.dtype == np.uint64 and np.array_equal(got, full[c, i0:i1]), (c, i0, i1)


@pytest.mark.parametrize("s", [8.0, 400.0])
def test_gauss_window_equals_the_full_model(s):
    n, first = 41, (1 << 32) - 1
    full, failed = M.gauss_fill(SEED, 80, first, 3, n, s, center=0.5)
    assert not failed
    cen = L.centre_period()[990:990 + 3 * n]                                # fractions, then exact integers
    full_c, failed = M.gauss_fill(SEED, 80, first, 3, n, s, centers=cen)
    assert not failed
    for c in range(3):
        for i0, i1 in [(0, n), (n - 1, n), (5, 33)]:
            got, bad = M.gauss_window(SEED, 80, first + c, i0, i1, s, center=0.5)
            assert not bad and np.array_equal(got, full[c, i0:i1]), (s, c, i0, i1)
            got, bad = M.gauss_window(SEED, 80, first + c, i0, i1, s, centers=cen[c * n + i0:c * n + i1])
            assert not bad and np.array_equal(got, full_c[c, i0:i1]), (s, c, i0, i1)
    got, bad = M.gauss_window(SEED, 80, first, 0, 2, s, centers=[2.0 ** 63, 0.25])
    assert bad and got[0] == 0


def test_pieces_cut_a_window_at_polynomial_boundaries():
    assert L.pieces(250, 262, 256) == [(0, 250, 256), (1, 0, 6)]
    assert L.pieces(0, 512, 256) == [(0, 0, 256), (1, 0, 256)]
    n = L.TWO32 - 1
    assert L.pieces(n - 512, n + 512, n) == [(0, n - 512, n), (1, 0, 512)]
    assert L.pieces(2 * n - 512, 2 * n, n) == [(1, n - 512, n)]
    for e0, e1, m in [(3, 1000, 7), (0, 1, 5), (699, 701, 700)]:
        got = L.pieces(e0, e1, m)
        assert [c * m + i for c, i0, i1 in got for i in range(i0, i1)] == list(range(e0, e1))


def test_windows_cover_the_named_places():
    for name in ("F1", "F2"):
        f = L.FILLS[name]
        wb, total = f["io_bits"] // 8, f["count"] * f["n"]
        starts = L.window_starts(total, wb, seed=3)
        word = (L.TWO32 - 1) // wb                                          # the word that holds byte 2^32 - 1
        assert starts[0] == 0 and starts[-1] == total - L.WINDOW and len(starts) >= 11
        assert any(s <= word < s + L.WINDOW for s in starts) and any(s <= word + L.WINDOW < s + L.WINDOW for s in starts)
        assert starts == L.window_starts(total, wb, seed=3) and starts != L.window_starts(total, wb, seed=4)
    n = L.FILLS["F3"]["n"]
    starts = L.f3_windows(n, seed=5)
    assert {0, (1 << 31) - 256, n - 512, n, 2 * n - 512} <= set(starts) and len(starts) == 13 and max(starts) == 2 * n - 512


# ---- periods and crossings ----------------------------------------------------------------------------------------------------------------------
def test_the_periods_never_divide_2_32():
    assert L.VALUES == 8 * 8191 == 65528 and L.TWO32 % L.VALUES == 64
    for d in (1, 4, 5, 10, 11, 12, 16, 40, 63):
        assert L.VALUES * d % 8 == 0 and L.TWO32 % (8191 * d) != 0           # whole bytes per period, and 2^32 bytes no whole number of periods
        assert L.period_ok(L.VALUES, 2, 8) and L.TWO32 % (L.VALUES * d // 8) != 0
    for k in range(64):
        assert (1 << k) % L.INSTANCES != 0 and (1 << k) % L.INSTANCES_B != 0
    assert L.period_ok(L.CENTRES, 8) and all(L.CENTRES % p for p in range(2, 256))
    with pytest.raises(AssertionError):
        L.period_ok(8, 2)
    with pytest.raises(AssertionError):
        L.period_ok(65536)
    assert L.period_ok(7, 1 << 30)                                          # an odd period fits no power of two, whatever the size of an item


def test_every_count_is_the_smallest_crossing_plus_3():
    for f in (L.FILLS["F1"], L.FILLS["F2"]):
        assert L.crossing(f["count"], f["per_item"]) and f["count"] == L.crossing_count(f["per_item"])
        assert f["per_item"] == f["n"] * (f["io_bits"] // 8 if f["unit"] == "bytes" else 1)
    f = L.FILLS["F3"]
    assert f["n"] == L.TWO32 - 1 and f["count"] == 2 and f["n"] < L.TWO32 <= 2 * f["n"]
    for name, h in {**L.HASHES, **L.RQ}.items():
        period = h["period"]
        assert L.crossing(h["count"], h["per_item"], period) and h["count"] == L.crossing_count(h["per_item"]), name
        assert L.period_ok(period, h["per_item"], h["per_item"] // 2, h["per_item"] // 8), name
        assert (period == L.INSTANCES_B) == (h["count"] % L.INSTANCES == 0), name      # 13 only where 7 divides the count
    for name, r in L.RQ.items():
        polys = r.get("rows", 1) * r.get("inner", 1)
        assert r["per_item"] == polys * r["n"] * (4 if "hat" in name else r["io_bits"] // 8), name
    with pytest.raises(AssertionError):
        L.crossing((1 << 21) + 4, 2048)
    with pytest.raises(AssertionError):
        L.crossing(1 << 21, 2048)


def test_every_flat_length_passes_2_32_by_a_ragged_end():
    for name, m in L.MAPS.items():
        assert L.ragged(m["length"], m["num"], m["den"]), name
        d = m.get("d", 8)
        assert L.TWO32 % (8191 * d) != 0, name
    assert L.MAPS["bytes12"]["length"] == -(-L.TWO32 * 8 // 12) + 77 and L.MAPS["fused10"]["length"] == -(-L.TWO32 * 8 // 10) + 77
    with pytest.raises(AssertionError):
        L.ragged(L.TWO32, 1)


def test_the_period_builders():
    v = L.value_period(3329, 1)
    assert v.shape == (L.VALUES,) and int(v.max()) == 3328 and int(v.min()) == 0 and np.array_equal(v, L.value_period(3329, 1))
    assert not np.array_equal(v[:64], v[64:128])                            # a read that wrapped by 2^32 mod 65 528 = 64 places meets other data
    assert int(L.value_period(0, 2, bits=16).max()) == 65535
    c = L.centre_period()
    assert c.shape == (L.CENTRES,) and (c[1000:1256] == np.round(c[1000:1256])).all() and ((c[2000:2256] * 2) % 2 == 1).all()
    a, b = L.poly_period(3329, 256, 3, False), L.poly_period(3329, 256, 4, True)
    assert a.shape == b.shape == (7, 256) and a.min() == 0 and a.max() == 3328 and b.min() == -3328 and b.max() == 3328
    assert len({bytes(r) for r in L.byte_period(33, 5)}) == 7


# ---- the entry points accept every count ---------------------------------------------------------------------------------------------------------
def _lib():
    from tools_amd import _ffi, sha2
    sha2._lib()
    return _ffi.lib()


def test_every_count_is_within_the_limits_of_its_entry_point():
    """ERR_HIP: every argument check passed and the first HIP call, on a device that does not exist, failed.  The pointers are never read."""
    assert L.within_limits()
    Lb, vp, sz, u64, u32, ci = _lib(), C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int
    a, b, c, e = (vp(k << 44) for k in (1, 2, 3, 4))                        # far apart: no overlap at any of the sizes
    for name, f in L.FILLS.items():
        head = (NO_DEVICE, u64(SEED), u32(70), u64(1 << 32), sz(f["count"]), sz(f["n"]))
        assert Lb.psf_sample_uniform_dev(*head, u64(3329), a, ci(f["io_bits"]), None) == ERR_HIP, name
        assert Lb.psf_sample_cbd_dev(*head, u32(3), a, ci(f["io_bits"]), None) == ERR_HIP, name
        assert Lb.psf_sample_discrete_gauss_dev(*head, C.c_double(0.5), None, C.c_double(8.0), a, None, ci(f["io_bits"]), None) == ERR_HIP, name
    f = L.FILLS["F1"]
    head = (NO_DEVICE, u64(SEED), u32(70), u64(0), sz(f["count"]), sz(f["n"]))
    assert Lb.psf_sample_discrete_gauss_dev(*head, C.c_double(0.0), b, C.c_double(8.0), a, None, ci(64), None) == ERR_HIP
    assert Lb.psf_sample_uniform_dev(NO_DEVICE, u64(SEED), u32(70), u64(0), sz(1), sz(1 << 32), u64(3329), a, ci(16), None) == ERR_PARAM    # n = 2^32: refused
    for name, m in L.MAPS.items():
        q, d, io, n = u64(m["q"]), u32(m.get("d", 0)), ci(m["io_bits"]), sz(m["length"])
        if name.startswith("compress"):
            assert Lb.psf_lossy_compress_dev(NO_DEVICE, q, d, n, a, b, io, None) == ERR_HIP, name
            assert Lb.psf_lossy_decompress_dev(NO_DEVICE, q, d, n, a, b, io, None) == ERR_HIP, name
        elif name == "digits64":
            assert Lb.psf_decode_digits_dev(NO_DEVICE, q, u64(m["base"]), n, a, b, io, None) == ERR_HIP, name
        elif name == "fused10":
            assert Lb.psf_compress_encode_dev(NO_DEVICE, q, d, n, a, b, io, None) == ERR_HIP, name
            assert Lb.psf_decode_decompress_dev(NO_DEVICE, q, d, n, b, a, io, None) == ERR_HIP, name
        else:
            assert Lb.psf_byte_encode_dev(NO_DEVICE, d, n, a, b, io, None) == ERR_HIP, name
            assert Lb.psf_byte_decode_dev(NO_DEVICE, q, d, n, b, a, c, io, None) == ERR_HIP, name
    h = L.HASHES["keccak"]
    for in_stride, out_stride in ((4096, h["out_len"]), (h["in_len"], 4096)):
        assert Lb.psf_keccak_dev(NO_DEVICE, 3, h["count"], a, h["in_len"], in_stride, b, h["out_len"], out_stride, None) == ERR_HIP
    for func, key in ((0, "sha256"), (1, "sha512")):
        h = L.HASHES[key]
        for in_stride, out_stride in ((4096, h["out_len"]), (h["in_len"], 4096)):
            assert Lb.psf_sha2_dev(NO_DEVICE, func, h["count"], a, h["in_len"], in_stride, b, h["out_len"], out_stride, None) == ERR_HIP, key
    assert Lb.psf_sample_ntt_fips203_dev(NO_DEVICE, L.HASHES["sample_ntt"]["count"], 0, a, 34, b, c, 64, None) == ERR_HIP
    assert Lb.psf_sample_cbd_fips203_dev(NO_DEVICE, L.HASHES["sample_cbd"]["count"], 2, a, 32, 0, 1, b, 64, None) == ERR_HIP
    assert Lb.psf_ntt_image_from_fips203_dev(NO_DEVICE, L.HASHES["image"]["count"], a, 16, b, None) == ERR_HIP
    assert Lb.psf_ntt_image_to_fips203_dev(NO_DEVICE, L.HASHES["image"]["count"], b, a, 16, None) == ERR_HIP
    for name in ("wave64", "wave16", "lds", "school"):
        r = L.RQ[name]
        args = (NO_DEVICE, u64(r["q"]), sz(r["n"]), sz(r["count"]), a, b, c, ci(r["io_bits"]), None)
        assert Lb.psf_poly_mul_negacyclic_dev(*args) == ERR_HIP, name
        if name in ("wave64", "school"):
            assert Lb.psf_poly_mul_cyclic_dev(*args) == ERR_HIP, name
    r = L.RQ["hat16"]
    for fwd, mul in ((Lb.psf_ntt_forward_dev, Lb.psf_poly_mul_hat_dev), (Lb.psf_ntt_forward_cyclic_dev, Lb.psf_poly_mul_hat_cyclic_dev)):
        assert fwd(NO_DEVICE, u64(r["q"]), sz(r["n"]), sz(r["count"]), a, ci(16), b, None) == ERR_HIP
        assert mul(NO_DEVICE, u64(r["q"]), sz(r["n"]), sz(r["count"]), b, sz(r["n"]), a, c, ci(16), None) == ERR_HIP
    for name in ("mat64", "matschool"):
        r = L.RQ[name]
        shape = (NO_DEVICE, u64(r["q"]), sz(r["n"]), sz(r["count"]), sz(2), sz(2), sz(1))
        for trans in (0, 1):
            assert Lb.psf_matpoly_mul_negacyclic_dev(*shape, a, sz(4), ci(trans), b, c, ci(64), None) == ERR_HIP, name
        assert Lb.psf_matpoly_mul_add_negacyclic_dev(*shape, a, sz(4), ci(0), b, c, ci(-1), c, ci(64), None) == ERR_HIP, name
    r = L.RQ["mathat16"]
    shape = (NO_DEVICE, u64(r["q"]), sz(r["n"]), sz(r["count"]), sz(2), sz(2), sz(1))
    assert Lb.psf_matpoly_mul_hat_dev(*shape, a, sz(4 * r["n"]), ci(0), b, c, ci(16), None) == ERR_HIP
