"""Compress_d / Decompress_d, the digit decoding and the FIPS 203 byte encodings (psf_compress.hip) on the MI355X over flat arrays that pass 2^32
words or 2^32 bytes -- in the values, or in the packed bytes.  The largest call of any other test has a length in the 2^20s, so the grid-stride
loops, the tile offsets (t * 1024 vectors, t * (TV / 8) * d bytes), the byte index of k_pack's tail and the bit index of k_unpack's have never
met an offset at or past 2^32; a truncated one stays inside the buffer and faults nothing.

Inputs repeat with a period of 8 * 8191 = 65 528 values (a whole number of bytes at every d; 2^32 is no multiple of it in values, words or
bytes: tests/helpers/large_cases.py), built on the device; the expectation is the big-integer model (tests/helpers/fips203_model.py,
byte_encoding_model.py) on one period, compared with every word and byte on the device, the ragged end included.  Every output is prefilled
with the guard byte between guard bytes.  The coefficient maps run one word past a 16-byte boundary (a head, the vectors, a ragged end); the
byte encodings run at both alignments, since only 16-byte aligned pointers take the tiles and only unaligned ones send every byte through the
tail loops.  Nothing of a buffer's size is copied to the host, and each test frees what it allocated."""
import time

import numpy as np
import pytest

from tests.helpers import byte_encoding_model as B
from tests.helpers import fips203_model as F
from tests.helpers import large_cases as L
from tests.helpers.slhdsa_gpu import release

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def report(request, torch):
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    print(f"\n{request.node.name}: {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB of device memory")


def words(torch, values, io_bits):
    """a numpy array of non-negative values as a device tensor of the call's word type (the bit patterns of uint16 / uint64)"""
    v = np.asarray(values, dtype=np.uint64)
    return torch.from_numpy(v.astype(np.uint16).view(np.int16) if io_bits == 16 else v.view(np.int64)).cuda()


def word(torch, io_bits):
    return torch.int16 if io_bits == 16 else torch.int64


def tiled_input(torch, period, length, io_bits, off):
    """`length` words that repeat `period`, the first `off` bytes past a 16-byte boundary: (buffer, view, pointer)"""
    wb = io_bits // 8
    buf, view, ptr = L.in_buffer(torch, length * wb, off)
    view = view.view(word(torch, io_bits))
    L.tile_into(torch, view, period)
    return buf, view, ptr


def checks(case):
    m = L.MAPS[case]
    assert L.ragged(m["length"], m["num"], m["den"])
    d = m.get("d", 8)
    assert L.period_ok(L.VALUES, m["io_bits"] // 8) and L.TWO32 % (8191 * d) != 0 and L.VALUES * d % 8 == 0
    return m


@pytest.mark.parametrize("case", ["compress16", "compress64"])
def test_compress_then_decompress_past_2_32(T, torch, case):
    m = checks(case)
    q, d, io, n = m["q"], m["d"], m["io_bits"], m["length"]
    wb = io // 8
    x = L.value_period(q, seed=11)
    y = [F.compress(v, d, q) for v in x.tolist()]
    x2 = [F.decompress(v, d, q) for v in y]
    assert max(y) == (1 << d) - 1 and min(y) == 0 and x2 != x.tolist()
    L.room(torch, 3 * n * wb)
    xb = yb = zb = got = None
    try:
        xb, _, xp = tiled_input(torch, words(torch, x, io), n, io, wb)
        yb, yp = L.out_buffer(torch, n * wb, wb)
        T.compression.lossy_compress_dev(xp, yp, q, d, n, io_bits=io)
        got = L.written(torch, yb, n * wb, wb, (case, "compress"), word(torch, io))
        L.same_tiled(torch, got, words(torch, y, io), (case, "compress"))
        xb = got = None
        release(torch)
        zb, zp = L.out_buffer(torch, n * wb, wb)
        T.compression.lossy_decompress_dev(yp, zp, q, d, n, io_bits=io)
        got = L.written(torch, zb, n * wb, wb, (case, "decompress"), word(torch, io))
        L.same_tiled(torch, got, words(torch, x2, io), (case, "decompress"))
    finally:
        xb = yb = zb = got = None
        release(torch)


def test_decode_digits_past_2_32_bytes(T, torch):
    m = checks("digits64")
    q, base, n = m["q"], m["base"], m["length"]
    c = L.value_period(q, seed=12)
    want = [F.decode(v, base, q) for v in c.tolist()]
    assert sorted(set(want)) == list(range(base))
    L.room(torch, 2 * n * 8)
    cb = ob = got = None
    try:
        cb, _, cp = tiled_input(torch, words(torch, c, 64), n, 64, 8)
        ob, op = L.out_buffer(torch, n * 8, 8)
        T.encodings.decode_digits_dev(cp, op, q, base, n, io_bits=64)
        got = L.written(torch, ob, n * 8, 8, "decode_digits", torch.int64)
        L.same_tiled(torch, got, words(torch, want, 64), "decode_digits")
    finally:
        cb = ob = got = None
        release(torch)


def same_bytes(torch, got, period_values, d, length, encode, what):
    """the packed bytes of `length` values that repeat `period_values`: whole periods against the period's bytes, the ragged end against its own encoding
    (the unused high bits of a final partial byte are 0)"""
    pb = L.VALUES * d // 8
    full, rem = divmod(length, L.VALUES)
    assert got.numel() == B.nbytes(length, d) == full * pb + B.nbytes(rem, d)
    L.same_tiled(torch, got[:full * pb], torch.from_numpy(encode(period_values)).cuda(), what)
    tail = torch.from_numpy(encode(period_values[:rem])).cuda()
    assert torch.equal(got[full * pb:], tail), (what, "the ragged end")


@pytest.mark.parametrize("off", [0, 1], ids=["aligned_tiles", "one_word_past"])
@pytest.mark.parametrize("case", ["bytes12", "bytes1"])
def test_byte_encode_then_decode_past_2_32(T, torch, case, off):
    m = checks(case)
    q, d, io, n = m["q"], m["d"], m["io_bits"], m["length"]
    wb, nb = io // 8, B.nbytes(n, d)
    assert nb > L.TWO32 if case == "bytes12" else n > L.TWO32
    y = L.value_period(q, seed=13)                                          # d = 12: canonical values; d = 1: any 16-bit word, read mod 2
    L.room(torch, 2 * n * wb + nb)
    yb = bb = zb = got = packed = None
    try:
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        yb, _, yp = tiled_input(torch, words(torch, y, io), n, io, off * wb)
        bb, bp = L.out_buffer(torch, nb, off)
        T.compression.byte_encode_dev(yp, bp, d, n, io_bits=io)
        packed = L.written(torch, bb, nb, off, (case, off, "encode"))
        same_bytes(torch, packed, y, d, n, lambda v: B.encode_np(v, d), (case, off, "encode"))
        yb = None
        release(torch)
        zb, zp = L.out_buffer(torch, n * wb, off * wb)
        T.compression.byte_decode_dev(bp, zp, q, d, n, d_noncanonical=flag.data_ptr(), io_bits=io)
        got = L.written(torch, zb, n * wb, off * wb, (case, off, "decode"), word(torch, io))
        L.same_tiled(torch, got, words(torch, y & np.uint64((1 << d) - 1), io), (case, off, "decode"))
        assert int(flag.item()) == 0
        if q:                                                               # one value >= q whose bytes lie past 2^32: the flag, and its residue
            at = n - 6
            b0 = at * d // 8
            assert at % 2 == 0 and d == 12 and b0 > L.TWO32 and at % L.VALUES > 6
            packed[b0] = 0xFF
            packed[b0 + 1] |= 0x0F
            zb.fill_(L.FILL)
            T.compression.byte_decode_dev(bp, zp, q, d, n, d_noncanonical=flag.data_ptr(), io_bits=io)
            got = L.written(torch, zb, n * wb, off * wb, (case, off, "decode, one value above q"), word(torch, io))
            assert int(flag.item()) == 1
            near = got[at - 2:at + 3].cpu().tolist()
            k = at % L.VALUES
            assert near == [int(y[k - 2]), int(y[k - 1]), 4095 % q, int(y[k + 1]), int(y[k + 2])], near
    finally:
        yb = bb = zb = got = packed = None
        release(torch)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned_tiles", "one_word_past"])
def test_compress_encode_then_decode_decompress_past_2_32_bytes(T, torch, off):
    m = checks("fused10")
    q, d, io, n = m["q"], m["d"], m["io_bits"], m["length"]
    wb, nb = io // 8, B.nbytes(n, d)
    assert nb > L.TWO32
    x = L.value_period(q, seed=14)
    y = np.array([F.compress(v, d, q) for v in x.tolist()], dtype=np.uint64)
    x2 = [F.decompress(v, d, q) for v in y.tolist()]
    L.room(torch, 2 * n * wb + nb)
    xb = bb = zb = got = packed = None
    try:
        xb, _, xp = tiled_input(torch, words(torch, x, io), n, io, off * wb)
        bb, bp = L.out_buffer(torch, nb, off)
        T.compression.compress_encode_dev(xp, bp, q, d, n, io_bits=io)
        packed = L.written(torch, bb, nb, off, ("compress_encode", off))
        same_bytes(torch, packed, x, d, n, lambda v: B.encode_np(y[:len(v)], d), ("compress_encode", off))
        xb = None
        release(torch)
        zb, zp = L.out_buffer(torch, n * wb, off * wb)
        T.compression.decode_decompress_dev(bp, zp, q, d, n, io_bits=io)
        got = L.written(torch, zb, n * wb, off * wb, ("decode_decompress", off), word(torch, io))
        L.same_tiled(torch, got, words(torch, x2, io), ("decode_decompress", off))
    finally:
        xb = bb = zb = got = packed = None
        release(torch)
