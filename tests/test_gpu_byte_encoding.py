"""ByteEncode_d / ByteDecode_d and their fusions with Compress_d / Decompress_d on the MI355X, bit for bit against the model
(tests/helpers/byte_encoding_model.py, tests/helpers/fips203_model.py): the 16-bit words over every value and every d, the 64-bit words at
full range, every length and pointer offset with guard bytes around each output, the non-canonical flag, streams, the host forms, and the
full-size round trip against the existing compression entry points."""
import numpy as np
import pytest

from tests.helpers import byte_encoding_model as B
from tests.helpers import fips203_model as M

pytestmark = pytest.mark.gpu

GUARD = 64                 # bytes before and after every output buffer (a multiple of 16: it does not change the alignment)
FILL = 0xA5


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _np_dtype(io_bits):
    return np.uint16 if io_bits == 16 else np.uint64


def _put(torch, raw, off):
    """a device byte buffer that holds the bytes of `raw` at byte offset `off` from a 16-byte aligned base; returns (tensor, pointer)"""
    raw = np.ascontiguousarray(raw).view(np.uint8).ravel()
    buf = torch.zeros(off + raw.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if raw.size:
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return buf, buf.data_ptr() + off


def _out(torch, nbytes, off):
    buf = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + GUARD + off


def _take(torch, buf, nbytes, off, what):
    """the nbytes the call wrote, after checking that the guard bytes on both sides are untouched"""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo = GUARD + off
    assert (host[:lo] == FILL).all(), (what, "wrote before the output")
    assert (host[lo + nbytes:] == FILL).all(), (what, "wrote beyond the output")
    return host[lo:lo + nbytes].copy()


def encode_dev(T, torch, vals, d, io_bits, q=None, voff=0, boff=0, stream=None):
    """byte_encode_dev (q None) or compress_encode_dev of the words `vals`, value pointer voff words and byte pointer boff bytes off alignment"""
    wb = io_bits // 8
    n = vals.size
    src, psrc = _put(torch, vals, voff * wb)
    nb = B.nbytes(n, d)
    dst, pdst = _out(torch, nb, boff)
    torch.cuda.synchronize()                                              # the buffers were filled on the current stream
    if q is None:
        T.compression.byte_encode_dev(psrc, pdst, d, n, io_bits=io_bits, stream=stream)
    else:
        T.compression.compress_encode_dev(psrc, pdst, q, d, n, io_bits=io_bits, stream=stream)
    return _take(torch, dst, nb, boff, ("encode", io_bits, d, q, n, voff, boff))


def decode_dev(T, torch, data, d, n, io_bits, q=0, fused=False, voff=0, boff=0, flag=None, stream=None):
    """byte_decode_dev (fused False) or decode_decompress_dev; returns the n words"""
    wb = io_bits // 8
    assert data.size == B.nbytes(n, d)
    src, psrc = _put(torch, data, boff)
    dst, pdst = _out(torch, n * wb, voff * wb)
    torch.cuda.synchronize()
    if fused:
        T.compression.decode_decompress_dev(psrc, pdst, q, d, n, io_bits=io_bits, stream=stream)
    else:
        T.compression.byte_decode_dev(psrc, pdst, q, d, n, d_noncanonical=flag, io_bits=io_bits, stream=stream)
    return _take(torch, dst, n * wb, voff * wb, ("decode", io_bits, d, q, n, voff, boff)).view(_np_dtype(io_bits))


# exact vectorised forms of the model for 16-bit operands (every intermediate < 2^34 in int64); spot-checked against the model below
def _compress16(x, d, q):
    return ((((x.astype(np.int64) % q) << d) + q // 2) // q % (1 << d)).astype(np.uint16)


def _decompress16(y, d, q):
    return ((y.astype(np.int64) % (1 << d) * q + (1 << (d - 1))) // (1 << d) % q).astype(np.uint16)


def _compress64(x, d, q):
    return np.array([M.compress(int(v), d, q) for v in x], dtype=np.uint64)


def _decompress64(y, d, q):
    return np.array([M.decompress(int(v), d, q) for v in y], dtype=np.uint64)


def _lossy_dev(T, torch, vals, d, q, io_bits, compress):
    """the existing one-word-per-value maps on the device"""
    src, psrc = _put(torch, vals, 0)
    dst, pdst = _out(torch, vals.size * (io_bits // 8), 0)
    f = T.compression.lossy_compress_dev if compress else T.compression.lossy_decompress_dev
    f(psrc, pdst, q, d, vals.size, io_bits=io_bits)
    return _take(torch, dst, vals.size * (io_bits // 8), 0, "lossy").view(_np_dtype(io_bits))


@pytest.mark.parametrize("q", [3329, 7681, 12289, 65521])
def test_16bit_words(T, torch, q):
    rng = np.random.default_rng(q)
    xs = np.concatenate([np.arange(1 << 16, dtype=np.uint32), rng.integers(0, 1 << 16, size=(1 << 16) + 77)]).astype(np.uint16)
    n = xs.size
    assert n % 128 and n > 16 * 8192                                      # whole tiles and a ragged end
    for d in range(1, 17):
        mask = (1 << d) - 1
        for i in rng.integers(0, n, size=32):
            assert _compress16(xs[i:i + 1], d, q)[0] == M.compress(int(xs[i]), d, q)
            assert _decompress16(xs[i:i + 1], d, q)[0] == M.decompress(int(xs[i]), d, q)
        want = B.encode_np(xs, d)
        got = encode_dev(T, torch, xs, d, 16)
        assert np.array_equal(got, want), (q, d, np.flatnonzero(got != want)[:8])
        # every d-bit pattern appears in `want`: decode it as it is, and mod q
        y = decode_dev(T, torch, want, d, n, 16)
        assert np.array_equal(y, xs & mask), (q, d)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        yq = decode_dev(T, torch, want, d, n, 16, q=q, flag=flag.data_ptr())
        mv, mflag = B.decode_np(want, d, n, q)
        assert np.array_equal(yq, mv.astype(np.uint16)), (q, d)
        assert bool(flag.item()) == mflag == ((1 << d) > q), (q, d)
        # the fused forms: the model, and the composition of the existing maps with the new pack / unpack
        cw = _compress16(xs, d, q)
        ce = encode_dev(T, torch, xs, d, 16, q=q)
        assert np.array_equal(ce, B.encode_np(cw, d)), (q, d)
        composed = encode_dev(T, torch, _lossy_dev(T, torch, xs, d, q, 16, True), d, 16)
        assert np.array_equal(ce, composed), (q, d)
        dd = decode_dev(T, torch, want, d, n, 16, q=q, fused=True)
        assert np.array_equal(dd, _decompress16(xs, d, q)), (q, d)
        assert np.array_equal(dd, _lossy_dev(T, torch, y, d, q, 16, False)), (q, d)


@pytest.mark.parametrize("q", [3329, 1 << 30, (1 << 62) - 57])
@pytest.mark.parametrize("d", [1, 5, 12, 31, 32, 33, 40, 63])
def test_64bit_words(T, torch, q, d):
    rng = np.random.default_rng(d * 1000 + q % 997)
    n = 2 * 2048 + 37                                                     # two whole tiles and a ragged end
    xs = rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    edge = [0, 1, q - 1, q, q + 1, 2 * q - 1, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, (1 << d) - 1, 1 << (d - 1), (1 << 64) - (1 << d)]
    xs[:len(edge)] = np.array(edge, dtype=np.uint64)
    xs[-len(edge):] = np.array(edge, dtype=np.uint64)
    assert (xs.view(np.int64) < 0).any()                                  # negative y among them
    mask = np.uint64((1 << d) - 1)
    want = B.encode_np(xs, d)
    assert want.tobytes() == B.encode_int(xs.tolist(), d)
    got = encode_dev(T, torch, xs, d, 64)
    assert np.array_equal(got, want), (q, d, np.flatnonzero(got != want)[:8])
    y = decode_dev(T, torch, want, d, n, 64)
    assert np.array_equal(y, xs & mask), (q, d)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    yq = decode_dev(T, torch, want, d, n, 64, q=q, flag=flag.data_ptr())
    mv, mflag = B.decode_np(want, d, n, q)
    assert np.array_equal(yq, mv) and bool(flag.item()) == mflag, (q, d)
    cw = _compress64(xs, d, q)
    ce = encode_dev(T, torch, xs, d, 64, q=q)
    assert np.array_equal(ce, B.encode_np(cw, d)), (q, d)
    assert np.array_equal(ce, encode_dev(T, torch, _lossy_dev(T, torch, xs, d, q, 64, True), d, 64)), (q, d)
    dd = decode_dev(T, torch, want, d, n, 64, q=q, fused=True)
    assert np.array_equal(dd, _decompress64(xs & mask, d, q)), (q, d)
    assert np.array_equal(dd, _lossy_dev(T, torch, y, d, q, 64, False)), (q, d)


def _expected(io_bits, q, d, xs):
    """(ByteEncode(xs), ByteEncode(Compress(xs)), Decompress(xs mod 2^d)) for the words xs"""
    if io_bits == 16:
        return B.encode_np(xs, d), B.encode_np(_compress16(xs, d, q), d), _decompress16(xs, d, q)
    if xs.size <= 8192:
        return B.encode_np(xs, d), B.encode_np(_compress64(xs, d, q), d), _decompress64(xs & np.uint64((1 << d) - 1), d, q)
    # large 64-bit inputs at small q and d: numpy's uint64 is exact while (x mod q) 2^d + q/2 < 2^64
    assert q < (1 << 32) and d <= 16
    c = ((xs % np.uint64(q)) << np.uint64(d)) + np.uint64(q // 2)
    c = c // np.uint64(q) % np.uint64(1 << d)
    y = xs & np.uint64((1 << d) - 1)
    dec = (y * np.uint64(q) + np.uint64(1 << (d - 1))) // np.uint64(1 << d) % np.uint64(q)
    return B.encode_np(xs, d), B.encode_np(c, d), dec


def _check_all_four(T, torch, io_bits, q, d, xs, voff, boff, stream=None):
    n = xs.size
    enc, cenc, dec = _expected(io_bits, q, d, xs)
    mask = _np_dtype(io_bits)((1 << d) - 1)
    key = (io_bits, q, d, n, voff, boff)
    got = encode_dev(T, torch, xs, d, io_bits, voff=voff, boff=boff, stream=stream)
    assert np.array_equal(got, enc), key
    if (n * d) % 8:
        assert got[-1] >> ((n * d) % 8) == 0, key                          # the high bits of the final partial byte
    assert np.array_equal(encode_dev(T, torch, xs, d, io_bits, q=q, voff=voff, boff=boff, stream=stream), cenc), key
    assert np.array_equal(decode_dev(T, torch, enc, d, n, io_bits, voff=voff, boff=boff, stream=stream), xs & mask), key
    mv, _ = B.decode_np(enc, d, n, q)
    assert np.array_equal(decode_dev(T, torch, enc, d, n, io_bits, q=q, voff=voff, boff=boff, stream=stream), mv.astype(_np_dtype(io_bits))), key
    assert np.array_equal(decode_dev(T, torch, enc, d, n, io_bits, q=q, fused=True, voff=voff, boff=boff, stream=stream), dec), key


def _words(rng, n, io_bits):
    if io_bits == 16:
        return rng.integers(0, 1 << 16, size=n).astype(np.uint16)
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)


@pytest.mark.parametrize("io_bits,q,d", [(16, 3329, 10), (16, 12289, 3), (64, 3329, 12), (64, (1 << 62) - 57, 33)])
@pytest.mark.parametrize("n", [0, 1, 7, 9, 127, 129, 4097])
def test_ragged_lengths_at_every_offset(T, torch, io_bits, q, d, n):
    """value pointer 0 ... 7 words and byte pointer 0 ... 15 bytes off a 16-byte boundary"""
    xs = _words(np.random.default_rng(n * 131 + d), n, io_bits)
    for voff in range(8):
        for boff in range(16):
            _check_all_four(T, torch, io_bits, q, d, xs, voff, boff)


@pytest.mark.parametrize("io_bits,q,d", [(16, 3329, 11), (64, 3329, 12)])
def test_long_ragged_length(T, torch, io_bits, q, d):
    """2^20 + 3 values: many whole tiles when both pointers are aligned, the plain path alone when one is not"""
    n = (1 << 20) + 3
    xs = _words(np.random.default_rng(io_bits), n, io_bits)
    aligned_voff = 8 if io_bits == 16 else 2
    for voff, boff in ((0, 0), (aligned_voff, 16), (1, 0), (0, 1), (7, 15), (aligned_voff, 5)):
        _check_all_four(T, torch, io_bits, q, d, xs, voff, boff)


@pytest.mark.parametrize("io_bits", [16, 64])
def test_noncanonical_flag(T, torch, io_bits):
    q, d = 3329, 12
    n = 3 * 8192 + 11
    rng = np.random.default_rng(4)
    dt = _np_dtype(io_bits)
    canonical = rng.integers(0, q, size=n).astype(dt)
    enc_ok = B.encode_np(canonical, d)
    cases = [("canonical", enc_ok, False)]
    for where in (5, 2 * 8192 + 100, n - 1):                             # inside a tile, in another, in the ragged end
        ys = canonical.copy()
        ys[where] = q if where != 5 else 4095
        cases.append((f"bad at {where}", B.encode_np(ys, d), True))
    for stream in (None, torch.cuda.Stream()):
        sp = None if stream is None else stream.cuda_stream
        for name, enc, bad in cases:
            for preset in (0, 1, 2):
                flag = torch.full((3,), preset, dtype=torch.int32, device="cuda")
                if stream is not None:
                    stream.wait_stream(torch.cuda.current_stream())
                y = decode_dev(T, torch, enc, d, n, io_bits, q=q, flag=flag.data_ptr() + 4, stream=sp)
                assert flag.tolist() == [preset, preset | int(bad), preset], (name, preset, io_bits)
                mv, mflag = B.decode_np(enc, d, n, q)
                assert mflag == bad and np.array_equal(y, mv.astype(dt)), name
            # q = 0: never touched, whatever the values
            flag = torch.full((3,), 6, dtype=torch.int32, device="cuda")
            decode_dev(T, torch, enc, d, n, io_bits, q=0, flag=flag.data_ptr() + 4, stream=sp)
            assert flag.tolist() == [6, 6, 6], name
            # NULL is accepted
            y = decode_dev(T, torch, enc, d, n, io_bits, q=q, flag=None, stream=sp)
            assert np.array_equal(y, B.decode_np(enc, d, n, q)[0].astype(dt)), name


def test_non_default_stream(T, torch):
    stream = torch.cuda.Stream()
    for io_bits, q, d, n in ((16, 3329, 10, 5 * 8192 + 129), (64, (1 << 62) - 57, 40, 3 * 2048 + 7)):
        xs = _words(np.random.default_rng(n), n, io_bits)
        for voff, boff in ((0, 0), (1, 3)):
            stream.wait_stream(torch.cuda.current_stream())
            _check_all_four(T, torch, io_bits, q, d, xs, voff, boff, stream=stream.cuda_stream)


@pytest.mark.parametrize("q,d", [(3329, 12), (3329, 10), ((1 << 62) - 57, 40), (1 << 30, 63), (257, 1)])
def test_host_forms(T, torch, q, d):
    """host form == device form == model, 64-bit words"""
    Cm = T.compression
    rng = np.random.default_rng(d)
    for n in (1, 9, 256, 2048 + 5):
        ys = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64, endpoint=True)
        xs = ys.view(np.uint64)
        want = B.encode_np(ys, d)
        enc = Cm.byte_encode(ys, d)
        assert enc.dtype == np.uint8 and np.array_equal(enc, want) and np.array_equal(enc, encode_dev(T, torch, xs, d, 64)), (q, d, n)
        y0, f0 = Cm.byte_decode(want, d, n)
        assert y0.dtype == np.int64 and not f0 and np.array_equal(y0.view(np.uint64), xs & np.uint64((1 << d) - 1)), (q, d, n)
        yq, fq = Cm.byte_decode(want, d, n, q=q)
        mv, mflag = B.decode_np(want, d, n, q)
        assert fq == mflag and np.array_equal(yq.view(np.uint64), mv), (q, d, n)
        assert np.array_equal(yq.view(np.uint64), decode_dev(T, torch, want, d, n, 64, q=q)), (q, d, n)
        ce = Cm.compress_encode(xs, d, q)
        assert np.array_equal(ce, B.encode_np(_compress64(xs, d, q), d)) and np.array_equal(ce, encode_dev(T, torch, xs, d, 64, q=q)), (q, d, n)
        assert np.array_equal(ce, Cm.byte_encode(Cm.lossy_compress(xs, d, q), d)), (q, d, n)
        dd = Cm.decode_decompress(want, d, q, n)
        assert dd.dtype == np.uint64 and np.array_equal(dd, _decompress64(xs & np.uint64((1 << d) - 1), d, q)), (q, d, n)
        assert np.array_equal(dd, decode_dev(T, torch, want, d, n, 64, q=q, fused=True)), (q, d, n)
    # a preset host flag is never cleared
    import ctypes as C
    L = T._ffi.lib()
    ys = np.arange(16, dtype=np.int64)
    enc = Cm.byte_encode(ys, 12)
    out = np.empty(16, dtype=np.int64)
    flag = C.c_int(1)
    assert L.psf_byte_decode(0, C.c_uint64(3329), C.c_uint32(12), C.c_size_t(16), enc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                             C.byref(flag)) == 0
    assert flag.value == 1 and np.array_equal(out, ys)


def test_known_answers_on_the_device(T):
    Cm = T.compression
    for d, values, expect in ((12, [0x123, 0xABC], "23C1AB"), (10, [0x3FF, 0, 0, 0], "FF03000000"), (4, [1, 2], "21"),
                              (1, [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], "0102"), (3, [7, 0, 7], "C701")):
        assert Cm.byte_encode(np.array(values), d).tobytes() == bytes.fromhex(expect)
        assert Cm.byte_decode(np.frombuffer(bytes.fromhex(expect), dtype=np.uint8), d, len(values))[0].tolist() == values
    # an ML-KEM-768 ciphertext: k = 3 polynomials at du = 10 and one at dv = 4
    rng = np.random.default_rng(768)
    u, v = rng.integers(0, 3329, size=(3, 256)), rng.integers(0, 3329, size=256)
    ct = np.concatenate([Cm.compress_encode(u, 10, 3329), Cm.compress_encode(v, 4, 3329)])
    assert ct.size == 1088
    assert ct[:960].tobytes() == b"".join(B.encode_int([M.compress(int(c), 10, 3329) for c in row], 10) for row in u)


def test_full_size_identity(T, torch):
    """2^26 coefficients in 16-bit words at q = 3329, d = 10: decode_decompress(compress_encode(x)) == decompress(compress(x))"""
    Cm = T.compression
    n, q, d = 1 << 26, 3329, 10
    nb = n * d // 8
    x = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device="cuda")
    enc = torch.full((GUARD + nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    Cm.compress_encode_dev(x.data_ptr(), enc.data_ptr() + GUARD, q, d, n, io_bits=16)
    torch.cuda.synchronize()
    assert B.nbytes(n, d) == nb == Cm.encoded_size(n, d)
    assert bool((enc[:GUARD] == FILL).all()) and bool((enc[GUARD + nb:] == FILL).all())      # exactly 2^26 10 / 8 bytes
    back = torch.empty_like(x)
    Cm.decode_decompress_dev(enc.data_ptr() + GUARD, back.data_ptr(), q, d, n, io_bits=16)
    y = torch.empty_like(x)
    ref = torch.empty_like(x)
    Cm.lossy_compress_dev(x.data_ptr(), y.data_ptr(), q, d, n, io_bits=16)
    Cm.lossy_decompress_dev(y.data_ptr(), ref.data_ptr(), q, d, n, io_bits=16)
    torch.cuda.synchronize()
    assert torch.equal(back, ref)
    # and the packed bytes are those of the composed route
    enc2 = torch.empty(nb, dtype=torch.uint8, device="cuda")
    Cm.byte_encode_dev(y.data_ptr(), enc2.data_ptr(), d, n, io_bits=16)
    torch.cuda.synchronize()
    assert torch.equal(enc[GUARD:GUARD + nb], enc2)
    head = enc2[:320 * 4].cpu().numpy()
    xh = x[:1024].cpu().numpy().view(np.uint16)
    assert np.array_equal(head, B.encode_np(_compress16(xh, d, q), d))
