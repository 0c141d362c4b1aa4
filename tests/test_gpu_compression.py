"""Compress_d / Decompress_d and the message encodings on the MI355X, bit for bit against the big-integer model (tests/helpers/fips203_model.py):
the 16-bit words exhaustively, the 64-bit words at their edges, host form == device form == model at awkward lengths and offsets in a
non-default stream, the reference's own shapes, and the encodings of tools_amd.encodings."""
import json
import os
import random

import numpy as np
import pytest

from tests.helpers import fips203_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, arr):
    """a device copy of a uint16 / uint64 / int64 numpy array (as int16 / int64 words)"""
    arr = np.ascontiguousarray(arr)
    view = arr.view(np.int16) if arr.dtype == np.uint16 else arr.view(np.int64)
    return torch.from_numpy(view.copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


# exact vectorised forms of the model for 16-bit operands (every intermediate < 2^34 in int64); spot-checked against the model below
def _compress16(x, d, q):
    return (((x.astype(np.int64) % q) << d) + q // 2) // q % (1 << d)


def _decompress16(y, d, q):
    return (y.astype(np.int64) * q + (1 << (d - 1))) // (1 << d) % q


@pytest.mark.parametrize("q", [257, 3329, 7681, 12289, 65521])
def test_16bit_exhaustive(T, torch, q):
    C = T.compression
    xs = np.arange(q, dtype=np.uint16)
    ys = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    dx, dy = _dev(torch, xs), _dev(torch, ys)
    out_c = torch.empty_like(dx)
    out_d = torch.empty_like(dy)
    rng = random.Random(q)
    for d in range(1, 17):
        C.lossy_compress_dev(dx.data_ptr(), out_c.data_ptr(), q, d, q, io_bits=16)
        C.lossy_decompress_dev(dy.data_ptr(), out_d.data_ptr(), q, d, 1 << 16, io_bits=16)
        torch.cuda.synchronize()
        gc, gd = _host(out_c, np.uint16), _host(out_d, np.uint16)
        ec, ed = _compress16(xs, d, q), _decompress16(ys, d, q)
        for i in rng.sample(range(q), 64):
            assert ec[i] == M.compress(i, d, q)
        for i in rng.sample(range(1 << 16), 64):
            assert ed[i] == M.decompress(i, d, q) == M.decompress(i - (1 << 16), d, q)    # the word read unsigned or signed
        assert np.array_equal(gc.astype(np.int64), ec), (q, d, np.flatnonzero(gc.astype(np.int64) != ec)[:8])
        assert np.array_equal(gd.astype(np.int64), ed), (q, d, np.flatnonzero(gd.astype(np.int64) != ed)[:8])


def _edge_moduli():
    rng = random.Random(2024)
    return [2, 3, 3329, 1 << 30, 1073741789, (1 << 61) - 1, (1 << 62) - 57, rng.randrange(2, 1 << 62), rng.randrange(1 << 40, 1 << 62)]


def _rounding_boundaries(q, d, count, rng):
    """x with (x 2^d + floor(q/2)) mod q in {0, q-1}: x = (t - floor(q/2)) / 2^d mod q, when 2^d is invertible mod q"""
    out = []
    try:
        inv = pow(1 << d, -1, q)
    except ValueError:
        return out
    for t in (0, q - 1):
        base = (t - q // 2) * inv % q
        out += [base, (base + 1) % q, (base - 1) % q]
    for _ in range(count):
        t = rng.choice((0, q - 1))
        out.append((t - q // 2 + q * rng.randrange(1 << 20)) * inv % q)
    return out


@pytest.mark.parametrize("q", _edge_moduli())
def test_64bit_edges(T, q):
    C = T.compression
    rng = random.Random(q)
    for d in sorted({1, 2, 10, 11, 12, max(1, (q - 1).bit_length()), 32, 62, 63}):
        xs = [0, 1, q - 1, q // 2, q // 2 + 1, max(q // 2 - 1, 0), q, q + 1, 2 * q - 1, U64, U64 - 1, 1 << 63, (1 << 62) - 1]
        xs += _rounding_boundaries(q, d, 32, rng) + [rng.randrange(1 << 64) for _ in range(64)] + [rng.randrange(q) for _ in range(64)]
        y = C.lossy_compress(np.array(xs, dtype=np.uint64), d, q)
        assert [int(v) for v in y] == [M.compress(x, d, q) for x in xs], (q, d)
        ys = [0, 1, -1, (1 << d) - 1, 1 << (d - 1), -(1 << (d - 1)), (1 << 63) - 1, -(1 << 63), -(1 << 62) - 3]
        ys += [(1 << d) + 5 if d < 62 else 12345, -(1 << d) - 7 if d < 62 else -12345]
        ys += [rng.randrange(-(1 << 63), 1 << 63) for _ in range(64)] + [rng.randrange(1 << d) for _ in range(64)]
        x = C.lossy_decompress(np.array(ys, dtype=np.int64), d, q)
        assert [int(v) for v in x] == [M.decompress(v, d, q) for v in ys], (q, d)
        assert (x < np.uint64(q)).all()
        rt = C.lossy_decompress(y, d, q)
        assert [int(v) for v in rt] == [M.decompress(M.compress(v, d, q), d, q) for v in xs]
    E = T.encodings
    for base in (2, 3, 256, (1 << 32) + 15, rng.randrange(2, 1 << 63), (1 << 63) - 1):
        dig = [0, 1, base - 1, base, U64, q - 1] + [rng.randrange(1 << 64) for _ in range(64)] + [rng.randrange(base) for _ in range(64)]
        out = E.encode_digits(np.array(dig, dtype=np.uint64), base, q)
        assert [int(v) for v in out] == [M.encode(v, base, q) for v in dig], (q, base)
        cs = [0, 1, q - 1, q, U64, q // 2, q // (2 * base)] + [rng.randrange(1 << 64) for _ in range(64)] + [rng.randrange(q) for _ in range(64)]
        got = E.decode_digits(np.array(cs, dtype=np.uint64), base, q)
        assert [int(v) for v in got] == [M.decode(v, base, q) for v in cs], (q, base)


LENGTHS = [0, 1, 7, 8, 9, 1023, (1 << 20) + 3]
# (op, q, parameter) per word size: parameter is d for the lossy pair, base for the encodings
OPS16 = [("compress", 3329, 11), ("decompress", 3329, 11), ("encode", 7681, 3), ("decode", 12289, 5)]
OPS64 = [("compress", (1 << 62) - 57, 40), ("decompress", 1073741789, 12), ("encode", (1 << 61) - 1, 1000003), ("decode", 3329, 256)]
MODEL = {"compress": M.compress, "decompress": M.decompress, "encode": M.encode, "decode": M.decode}


def _dev_call(T, op, q, p, src, dst, n, io_bits, stream):
    if op == "compress":
        T.compression.lossy_compress_dev(src, dst, q, p, n, io_bits=io_bits, stream=stream)
    elif op == "decompress":
        T.compression.lossy_decompress_dev(src, dst, q, p, n, io_bits=io_bits, stream=stream)
    elif op == "encode":
        T.encodings.encode_digits_dev(src, dst, q, p, n, io_bits=io_bits, stream=stream)
    else:
        T.encodings.decode_digits_dev(src, dst, q, p, n, io_bits=io_bits, stream=stream)


def _host_call(T, op, q, p, arr):
    if op == "compress":
        return T.compression.lossy_compress(arr, p, q).view(np.uint64)
    if op == "decompress":
        return T.compression.lossy_decompress(arr.view(np.int64), p, q)
    if op == "encode":
        return T.encodings.encode_digits(arr, p, q)
    return T.encodings.decode_digits(arr, p, q)


@pytest.mark.parametrize("io_bits", [16, 64])
@pytest.mark.parametrize("n", LENGTHS)
def test_host_device_model_agree(T, torch, io_bits, n):
    """every length, with the device buffers at element offsets (0, 0), (1, 1), (1, 0) and (0, 3), on a non-default stream"""
    rng = np.random.default_rng(n * 7 + io_bits)
    dt = np.uint16 if io_bits == 16 else np.uint64
    stream = torch.cuda.Stream()
    for op, q, p in (OPS16 if io_bits == 16 else OPS64):
        src = rng.integers(0, 1 << 16, size=n + 3, dtype=np.uint64).astype(np.uint16) if io_bits == 16 else \
            rng.integers(0, 1 << 64, size=n + 3, dtype=np.uint64, endpoint=False)
        want_idx = sorted(set(range(min(n, 16))) | set(range(max(n - 16, 0), n)) | set(rng.integers(0, max(n, 1), size=min(n, 512)).tolist()))
        want_idx = [i for i in want_idx if i < n]
        host = None
        if io_bits == 64:
            host = _host_call(T, op, q, p, np.ascontiguousarray(src[1:n + 1]))
        for si, di in ((0, 0), (1, 1), (1, 0), (0, 3)):
            dsrc = _dev(torch, src)
            ddst = torch.full((n + 3,), -1, dtype=dsrc.dtype, device="cuda")
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                _dev_call(T, op, q, p, dsrc.data_ptr() + si * dsrc.element_size(), ddst.data_ptr() + di * ddst.element_size(), n, io_bits,
                          stream.cuda_stream)
            stream.synchronize()
            got = _host(ddst, dt)
            sentinel = np.array([-1], dtype=np.int16 if io_bits == 16 else np.int64).view(dt)[0]
            assert (got[:di] == sentinel).all() and (got[di + n:] == sentinel).all(), (op, si, di, "wrote outside the range")
            out = got[di:di + n]
            for i in want_idx:
                w = int(src[si + i])
                if op == "decompress" and io_bits == 64:
                    w = w - (1 << 64) if w >> 63 else w
                assert int(out[i]) == MODEL[op](w, p, q), (op, io_bits, n, si, di, i)
            if host is not None and si == 1:
                assert np.array_equal(out, host), (op, n, si, di)


def test_reference_shaped_round_trips(T):
    """the reference's tests: a 2x2 MatPolynomialRingZq at n = 16, q = 3329, d = 11 and a polynomial at q = 257, d = 4"""
    C = T.compression
    rng = np.random.default_rng(1)
    for shape, q, d in (((2, 2, 16), 3329, 11), ((16,), 257, 4)):
        x = rng.integers(0, q, size=shape, dtype=np.int64)
        y = C.lossy_compress(x, d, q)
        assert y.shape == shape and ((y >= 0) & (y < (1 << d))).all()
        assert [int(v) for v in y.ravel()] == [M.compress(int(v), d, q) for v in x.ravel()]
        back = C.lossy_decompress(y, d, q)
        assert back.shape == shape
        bound = 1 << ((q - 1).bit_length() - d - 1)
        dist = (back.astype(np.int64) - x) % q
        assert (np.minimum(dist, q - dist) <= bound).all()
        xneg = x - q * 3                                               # a PolyOverZ representative: read mod q
        assert np.array_equal(C.lossy_compress(xneg, d, q), y)


def test_encodings_fixture(T):
    with open(os.path.join(ROOT, "tests", "golden", "ref_encoding_kats.json")) as fh:
        kats = json.load(fh)
    E = T.encodings
    for rec in kats["encode"]:
        for c in rec["cases"]:
            got = E.encode_value_in_polynomialringzq(c["value"], rec["base"], rec["q"], rec["n"])
            assert got.dtype == np.uint64 and got.tolist() == c["expect"], (rec["source"], c)
            assert E.decode_value_from_polynomialringzq(got, rec["base"], rec["q"]) == c["value"]
    for rec in kats["encode_errors"]:
        with pytest.raises(T.PsfError) as ei:
            E.encode_value_in_polynomialringzq(rec["value"], rec["base"], rec["q"], rec["n"])
        assert ei.value.status == 1, rec["source"]
    for rec in kats["round_trips"]:
        lo, hi = rec.get("value_range", [rec.get("value"), rec.get("value")])
        vals = sorted({lo, hi, *random.Random(3).sample(range(lo, hi + 1), min(200, hi - lo + 1))})
        enc = E.encode_values(vals, rec["base"], rec["q"], rec["n"])
        assert E.decode_values(enc, rec["base"], rec["q"]) == vals, rec["source"]


@pytest.mark.parametrize("n,q", [(16, 257), (17, 257), (256, 3329), (256, 1073741789)])
@pytest.mark.parametrize("base", [2, 3, 5, 256])
def test_encodings_round_trip(T, n, q, base):
    """1000 random values: encode_values / decode_values equal the model; decoding returns the value wherever every digit survives the
    rounding, i.e. (base - 1) (q mod base) <= floor(q / (2 base)) -- it does not for base 256 at q = 257 or 3329 (floor(q/base) = 1 or 13)"""
    E = T.encodings
    rng = random.Random(n * q + base)
    vals = [0, 1, base ** n - 1] + [rng.randrange(base ** n) for _ in range(997)]
    enc = E.encode_values(vals, base, q, n)
    assert enc.shape == (1000, n)
    for i in range(0, 1000, 97):
        assert [int(v) for v in enc[i]] == M.encode_value(vals[i], base, q, n)
    dec = E.decode_values(enc, base, q)
    assert dec == [M.decode_value([int(c) for c in row], base, q) for row in enc]
    if (base - 1) * (q % base) <= q // (2 * base):
        assert dec == vals
    assert E.decode_value_from_polynomialringzq(enc[5], base, q) == dec[5]
    assert E.encode_value_in_polynomialringzq(vals[5], base, q, n).tolist() == enc[5].tolist()


def test_decode_arbitrary_words(T):
    E = T.encodings
    rng = np.random.default_rng(9)
    for q in (257, 3329, 1073741789, (1 << 62) - 57):
        for base in (2, 3, 5, 256, 65537):
            c = rng.integers(0, 1 << 64, size=4096, dtype=np.uint64, endpoint=False)
            got = E.decode_digits(c.reshape(16, 256), base, q)
            assert [int(v) for v in got.ravel()] == [M.decode(int(v), base, q) for v in c], (q, base)
            vals = E.decode_values(c.reshape(16, 256), base, q)
            assert vals == [M.decode_value([int(v) for v in row], base, q) for row in c.reshape(16, 256)]
