"""SHA3 / SHAKE, the byte-exact FIPS 203 samplers and the NTT-domain interop on the MI355X (tools_amd/fips203.py), against hashlib and the
pure-Python model of tests/helpers/fips203_kpke_model.py.  Every comparison is exact equality; every output sits between guard bytes.  The last
test runs K-PKE.KeyGen, Encrypt and Decrypt of ML-KEM-512 / -768 / -1024 entirely in device calls and compares ek, dk and the ciphertext with the
model's bytes."""
import functools
import hashlib
import random

import numpy as np
import pytest

from tests.helpers import fips203_kpke_model as M

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
Q, N = 3329, 256
HASHES = [(hashlib.sha3_256, 136, 32), (hashlib.sha3_512, 72, 64), (hashlib.shake_128, 168, 0), (hashlib.shake_256, 136, 0)]
FOUR_BLOCK_INPUT = bytes(range(32)) + bytes([62, 5])


@pytest.fixture(scope="module")
def F():
    import tools_amd
    return tools_amd.fips203


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _out(torch, nbytes, off=0):
    buf = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + GUARD + off


def _take(torch, buf, nbytes, off, what):
    """the nbytes a call wrote, after checking that the guard bytes on both sides are untouched"""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo = GUARD + off
    assert (host[:lo] == FILL).all(), (what, "wrote before the output")
    assert (host[lo + nbytes:] == FILL).all(), (what, "wrote beyond the output")
    return host[lo:lo + nbytes].copy()


def _put(torch, data, off=0):
    """bytes on the device, the first one `off` bytes past a 16-byte boundary; returns (tensor, pointer)"""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).ravel()
    buf = torch.zeros((16 + data.size + off,), dtype=torch.uint8, device="cuda")
    buf[off:off + data.size] = torch.from_numpy(data.copy())
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + off


def _digest(h, msg, out_len, fixed):
    return h(msg).digest() if fixed else h(msg).digest(out_len)


def _messages(count, in_len, salt):
    rng = random.Random(salt * 1000003 + count * 7919 + in_len)
    return [rng.randbytes(in_len) for _ in range(count)]


def run_hash(F, torch, func, msgs, out_len, in_off=0, out_off=0, in_pad=0, out_pad=0, stream=None):
    """one psf_keccak_dev call on rows of len + pad bytes; returns the digests and checks that nothing else of the guarded output changed"""
    count, in_len = len(msgs), len(msgs[0])
    in_stride, out_stride = in_len + in_pad, out_len + out_pad
    rows = np.full((count, in_stride), 0x3C, dtype=np.uint8)
    for c, m in enumerate(msgs):
        rows[c, :in_len] = np.frombuffer(m, dtype=np.uint8)
    din, pin = _put(torch, rows, in_off)
    nbytes = (count - 1) * out_stride + out_len
    buf, pout = _out(torch, nbytes, out_off)
    torch.cuda.synchronize()
    F.keccak_dev(func, count, pin, in_len, pout, out_len, in_stride=in_stride, out_stride=out_stride, stream=stream)
    raw = _take(torch, buf, nbytes, out_off, (func, count, in_len, out_len))
    got = []
    for c in range(count):
        got.append(bytes(raw[c * out_stride:c * out_stride + out_len]))
        assert (raw[c * out_stride + out_len:(c + 1) * out_stride] == FILL).all(), "wrote between two digests"
    return got


# ---- hashes --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("func", range(4))
def test_four_functions_on_the_length_grid(F, torch, func):
    h, rate, fixed = HASHES[func]
    for in_len in (0, 1, rate - 2, rate - 1, rate, rate + 1, 2 * rate - 1, 2 * rate, 1600):
        for count in (1, 65, 257):
            msgs = _messages(count, in_len, func)
            if in_len >= 8:
                assert len(set(msgs)) == count
            for out_len in ([fixed] if fixed else [1, rate - 1, rate, rate + 1, 3 * rate + 5]):
                got = run_hash(F, torch, func, msgs, out_len)
                want = [_digest(h, m, out_len, fixed) for m in msgs]
                assert got == want, (func, in_len, count, out_len)


@pytest.mark.parametrize("func", range(4))
def test_unaligned_pointers_and_wide_strides(F, torch, func):
    h, rate, fixed = HASHES[func]
    out_len = fixed or rate + 9
    for in_len in (33, rate + 1):
        msgs = _messages(65, in_len, 50 + func)
        want = [_digest(h, m, out_len, fixed) for m in msgs]
        for in_off, out_off, in_pad, out_pad in ((1, 3, 0, 0), (3, 1, 5, 11), (0, 0, 8 - in_len % 8, 8 - out_len % 8), (8, 8, 3, 0)):
            assert run_hash(F, torch, func, msgs, out_len, in_off, out_off, in_pad, out_pad) == want, (func, in_len, in_off, out_off, in_pad, out_pad)


def test_stream_and_host_form(F, torch):
    msgs = _messages(70, 33, 99)
    want = [hashlib.shake_256(m).digest(128) for m in msgs]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert run_hash(F, torch, F.SHAKE256, msgs, 128, stream=s.cuda_stream) == want
    got = F.keccak(F.SHAKE256, msgs, 128)
    assert [bytes(r) for r in got] == want
    got = F.keccak(F.SHA3_512, np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(70, 33), 64)
    assert [bytes(r) for r in got] == [hashlib.sha3_512(m).digest() for m in msgs]
    assert bytes(F.keccak(F.SHA3_256, [b""], 32)[0]) == hashlib.sha3_256(b"").digest()
    j_in = _messages(3, 32 + 1568, 5)                                    # J's input in ML-KEM-1024: 10 absorb blocks
    assert [bytes(r) for r in F.keccak(F.SHAKE256, j_in, 32)] == [M.J(m) for m in j_in]


# ---- SampleNTT -----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def three_block_inputs():
    """64 random inputs that need exactly three SHAKE128 blocks"""
    rng, out = random.Random(11), []
    while len(out) < 64:
        s = rng.randbytes(34)
        if M.sample_ntt_blocks(s)[1] == 3:
            out.append(s)
    return tuple(out)


def run_sample_ntt(F, torch, seeds, io_bits, k=0, off=0, stride_pad=0, flag=None):
    """one psf_sample_ntt_fips203_dev call; returns (count [* k * k], 256) integers"""
    count, seed_len = len(seeds), 32 if k else 34
    rows = np.zeros((count, seed_len + stride_pad), dtype=np.uint8)
    for c, s in enumerate(seeds):
        rows[c, :seed_len] = np.frombuffer(s, dtype=np.uint8)
    dseed, pseed = _put(torch, rows, 1)
    polys = count * (k * k if k else 1)
    nbytes = polys * N * io_bits // 8
    buf, pout = _out(torch, nbytes, off)
    torch.cuda.synchronize()
    F.sample_ntt_dev(pout, count, pseed, k=k, seed_stride=seed_len + stride_pad, d_fail=flag.data_ptr() if flag is not None else None, io_bits=io_bits)
    raw = _take(torch, buf, nbytes, off, ("sample_ntt", count, k, io_bits))
    return raw.view(np.uint16 if io_bits == 16 else np.uint64).reshape(polys, N).astype(np.int64)


@pytest.mark.parametrize("io_bits", [16, 64])
def test_sample_ntt_raw_form_against_the_model(F, torch, io_bits):
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for count in (1, 64, 65, 300):
        rng = random.Random(count)
        seeds = [rng.randbytes(34) for _ in range(count)]
        got = run_sample_ntt(F, torch, seeds, io_bits, off=0 if count != 65 else io_bits // 8, stride_pad=count % 3, flag=flag)
        assert got.tolist() == [M.sample_ntt(s) for s in seeds], (count, io_bits)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("io_bits", [16, 64])
def test_sample_ntt_four_block_input_among_three_block_inputs(F, torch, io_bits):
    assert M.sample_ntt_blocks(FOUR_BLOCK_INPUT)[1] == 4
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for pos in (0, 17, 63, None):
        seeds = list(three_block_inputs()) if pos is not None else [FOUR_BLOCK_INPUT]
        if pos is not None:
            seeds[pos] = FOUR_BLOCK_INPUT
        got = run_sample_ntt(F, torch, seeds, io_bits, flag=flag)
        assert got.tolist() == [M.sample_ntt(s) for s in seeds], (pos, io_bits)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("io_bits", [16, 64])
def test_sample_ntt_matrix_form_is_the_raw_form_on_the_built_strings(F, torch, io_bits):
    rng = random.Random(21)
    rhos = [rng.randbytes(32) for _ in range(3)]
    for k in (2, 3, 4):
        built = [rho + bytes([j, i]) for rho in rhos for i in range(k) for j in range(k)]
        mat = run_sample_ntt(F, torch, rhos, io_bits, k=k, stride_pad=k)
        assert np.array_equal(mat, run_sample_ntt(F, torch, built, io_bits)), (k, io_bits)
        assert mat.tolist() == [M.sample_ntt(s) for s in built], (k, io_bits)
    host = F.sample_ntt(np.frombuffer(b"".join(rhos), dtype=np.uint8).reshape(3, 32), k=2)
    assert host.shape == (3, 2, 2, N) and host[1, 1, 0].tolist() == M.sample_ntt(rhos[1] + bytes([0, 1]))
    raw = F.sample_ntt(np.frombuffer(FOUR_BLOCK_INPUT, dtype=np.uint8).reshape(1, 34))
    assert raw[0].tolist() == M.sample_ntt(FOUR_BLOCK_INPUT)


# ---- CBD -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io_bits", [16, 64])
@pytest.mark.parametrize("eta", [2, 3])
def test_sample_cbd_against_the_model(F, torch, eta, io_bits):
    for count in (1, 65):
        rng = random.Random(100 * eta + count)
        sigmas = [rng.randbytes(32) for _ in range(count)]
        rows = np.zeros((count, 32 + count % 4), dtype=np.uint8)
        for c, s in enumerate(sigmas):
            rows[c, :32] = np.frombuffer(s, dtype=np.uint8)
        dsig, psig = _put(torch, rows, 3)
        for per_seed, first in ((1, 0), (4, 4), (8, 248), (1, 248), (8, 0)):
            nbytes = count * per_seed * N * io_bits // 8
            buf, pout = _out(torch, nbytes, 0)
            torch.cuda.synchronize()
            F.sample_cbd_dev(pout, count, psig, eta, first_nonce=first, per_seed=per_seed, sigma_stride=rows.shape[1], io_bits=io_bits)
            raw = _take(torch, buf, nbytes, 0, ("sample_cbd", eta, count, per_seed, first, io_bits))
            got = raw.view(np.int16 if io_bits == 16 else np.int64).reshape(count * per_seed, N).astype(np.int64)
            want = [M.sample_poly_cbd(eta, M.PRF(eta, s, first + t)) for s in sigmas for t in range(per_seed)]
            assert got.tolist() == want, (eta, count, per_seed, first, io_bits)
    host = F.sample_cbd(np.frombuffer(sigmas[0] + sigmas[1], dtype=np.uint8).reshape(2, 32), eta, first_nonce=3, per_seed=2)
    assert host.shape == (2, 2, N) and host[1, 1].tolist() == M.sample_poly_cbd(eta, M.PRF(eta, sigmas[1], 4))


# ---- interop -------------------------------------------------------------------------------------------------------------------------------------

def _dev_poly(torch, values, io_bits):
    """integers (any shape, in (-2^15, 2^15)) as device words of io_bits (the bit pattern is what counts: uint16 residues below 2^15 are int16)"""
    return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(device="cuda", dtype=torch.int16 if io_bits == 16 else torch.int64).contiguous()


@functools.lru_cache(maxsize=None)
def interop_polys():
    rng = random.Random(31)
    polys = [[rng.randrange(Q) for _ in range(N)] for _ in range(4)]
    polys += [[0] * N, [Q - 1] * N, [1] + [0] * (N - 1), [0] * (N - 1) + [Q - 1], [0] * 128 + [1] + [0] * 127]
    return tuple(tuple(p) for p in polys)


@pytest.mark.parametrize("io_bits", [16, 64])
def test_to_of_forward_is_algorithm_9(F, torch, io_bits):
    import tools_amd as T
    polys = [list(p) for p in interop_polys()]
    count = len(polys)
    da = _dev_poly(torch, polys, io_bits)
    hat = torch.empty((count, N), dtype=torch.int32, device="cuda")
    T.gadget.ntt_forward_dev(da.data_ptr(), hat.data_ptr(), Q, N, count, io_bits=io_bits)
    nbytes = count * N * io_bits // 8
    buf, pout = _out(torch, nbytes, 0)
    F.image_to_fips203_dev(pout, count, hat.data_ptr(), io_bits=io_bits)
    raw = _take(torch, buf, nbytes, 0, ("image_to", io_bits))
    got = raw.view(np.uint16 if io_bits == 16 else np.uint64).reshape(count, N).astype(np.int64)
    assert got.tolist() == [M.ntt(p) for p in polys]
    assert np.array_equal(F.image_to_fips203(hat.cpu().numpy().view(np.uint32)).astype(np.int64), got)


@pytest.mark.parametrize("io_bits", [16, 64])
def test_products_with_from_images_equal_the_schoolbook_product(F, torch, io_bits):
    import tools_amd as T
    rng = random.Random(32)
    Fh = [list(p) for p in interop_polys()]                                 # read as NTT-domain polynomials
    count = len(Fh)
    b = [[rng.randrange(-Q + 1, Q) for _ in range(N)] for _ in range(count)]
    b[4] = [Q - 1 if i & 1 else -(Q - 1) for i in range(N)]
    want = [M.schoolbook(M.ntt_inv(f), y) for f, y in zip(Fh, b)]
    dF, db = _dev_poly(torch, Fh, io_bits), _dev_poly(torch, b, io_bits)
    nb = count * N * 4
    buf, phat = _out(torch, nb, 0)
    F.image_from_fips203_dev(phat, count, dF.data_ptr(), io_bits=io_bits)
    img = _take(torch, buf, nb, 0, ("image_from", io_bits)).view(np.uint32).reshape(count, N)
    assert np.array_equal(F.image_from_fips203(np.asarray(Fh, dtype=np.uint64)), img)
    assert (np.abs(img.view(np.int32)) < Q).all()
    hat = torch.from_numpy(img.view(np.int32).copy()).cuda()
    out = torch.empty((count, N), dtype=db.dtype, device="cuda")

    def product(h):
        T.gadget.poly_mul_hat_dev(h.data_ptr(), N, db.data_ptr(), out.data_ptr(), Q, N, count, io_bits=io_bits)
        torch.cuda.synchronize()
        return (out.cpu().numpy().astype(np.int64) & (0xFFFF if io_bits == 16 else -1)).tolist()
    assert product(hat) == want
    # from(to(image)) gives identical products, for the images of `from` and for those of the forward transform
    back = torch.empty((count, N), dtype=dF.dtype, device="cuda")
    fwd = torch.empty((count, N), dtype=torch.int32, device="cuda")
    T.gadget.ntt_forward_dev(_dev_poly(torch, [M.ntt_inv(f) for f in Fh], io_bits).data_ptr(), fwd.data_ptr(), Q, N, count, io_bits=io_bits)
    for src in (hat, fwd):
        again = torch.empty_like(hat)
        F.image_to_fips203_dev(back.data_ptr(), count, src.data_ptr(), io_bits=io_bits)
        F.image_from_fips203_dev(again.data_ptr(), count, back.data_ptr(), io_bits=io_bits)
        assert product(again) == want
        assert product(src) == want


@pytest.mark.parametrize("io_bits", [16, 64])
def test_fused_product_on_a_sampled_matrix(F, torch, io_bits):
    """E + A b with the from-images of a sampled 3 x 3 A_hat: trans_a 0 and 1, one set of images for every batch and one per batch"""
    import tools_amd as T
    rng = random.Random(33)
    k, batches = 3, 2
    rhos = [rng.randbytes(32) for _ in range(batches)]
    dr, pr = _put(torch, b"".join(rhos))
    A = torch.empty((batches, k, k, N), dtype=torch.int16 if io_bits == 16 else torch.int64, device="cuda")
    F.sample_ntt_dev(A.data_ptr(), batches, pr, k=k, io_bits=io_bits)
    hat = torch.empty((batches, k, k, N), dtype=torch.int32, device="cuda")
    F.image_from_fips203_dev(hat.data_ptr(), batches * k * k, A.data_ptr(), io_bits=io_bits)
    a_coef = [[[M.ntt_inv(M.sample_ntt(rho + bytes([j, i]))) for j in range(k)] for i in range(k)] for rho in rhos]
    b = [[[rng.randrange(-3, 4) for _ in range(N)] for _ in range(k)] for _ in range(batches)]
    e = [[[rng.randrange(-Q + 1, Q) for _ in range(N)] for _ in range(k)] for _ in range(batches)]
    db, de = _dev_poly(torch, b, io_bits), _dev_poly(torch, e, io_bits)
    out = torch.empty((batches, k, N), dtype=db.dtype, device="cuda")
    for trans in (0, 1):
        for shared in (True, False):
            T.rq.matpoly_mul_add_hat_dev(hat.data_ptr(), db.data_ptr(), de.data_ptr(), out.data_ptr(), Q, N, batches, k, k, 1,
                                         hat_stride=0 if shared else k * k * N, trans_a=trans, io_bits=io_bits)
            torch.cuda.synchronize()
            got = (out.cpu().numpy().astype(np.int64) & (0xFFFF if io_bits == 16 else -1)).tolist()
            for c in range(batches):
                a = a_coef[0 if shared else c]
                for i in range(k):
                    acc = [v % Q for v in e[c][i]]
                    for j in range(k):
                        acc = M.poly_add(acc, M.schoolbook(a[j][i] if trans else a[i][j], b[c][j]))
                    assert got[c][i] == acc, (io_bits, trans, shared, c, i)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,io_bits", [("ML-KEM-512", 16), ("ML-KEM-768", 64), ("ML-KEM-768", 16), ("ML-KEM-1024", 16)])
def test_kpke_in_device_calls_equals_the_model_bytes(F, torch, name, io_bits):
    """K-PKE.KeyGen, Encrypt and Decrypt (Algorithms 13 to 15) for 3 instances, every step a device call of the library (torch only concatenates,
    adds and reduces mod q between them): ek, dk and the ciphertext are the model's bytes, and decryption returns the message."""
    import tools_amd as T
    k, eta1, eta2, du, dv = M.PARAMS[name]
    B = 3
    rng = random.Random(40 + sorted(M.PARAMS).index(name))
    ds, ms, rs = ([rng.randbytes(32) for _ in range(B)] for _ in range(3))
    want = []
    for d, m, r in zip(ds, ms, rs):
        ek, dk = M.kpke_keygen(d, name)
        c = M.kpke_encrypt(ek, m, r, name)
        assert M.kpke_decrypt(dk, c, name) == m
        want.append((ek, dk, c))
    sword = torch.int16 if io_bits == 16 else torch.int64
    dev = dict(device="cuda")
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, **dev)      # noqa: E731
    words = lambda *shape: torch.empty(shape, dtype=sword, **dev)        # noqa: E731
    images = lambda *shape: torch.empty(shape, dtype=torch.int32, **dev)  # noqa: E731
    fma = T.rq.matpoly_mul_add_hat_dev
    canon = lambda x: torch.where(x < 0, x + Q, x)                        # noqa: E731

    # K-PKE.KeyGen: (rho, sigma) = G(d || k)
    g_in = torch.from_numpy(np.frombuffer(b"".join(d + bytes([k]) for d in ds), dtype=np.uint8).copy()).cuda()
    g_out = u8(B, 64)
    F.keccak_dev(F.SHA3_512, B, g_in.data_ptr(), 33, g_out.data_ptr(), 64)
    rho_ptr, sigma_ptr = g_out.data_ptr(), g_out.data_ptr() + 32
    A_fips, A_hat = words(B, k, k, N), images(B, k, k, N)
    F.sample_ntt_dev(A_fips.data_ptr(), B, rho_ptr, k=k, seed_stride=64, io_bits=io_bits)
    F.image_from_fips203_dev(A_hat.data_ptr(), B * k * k, A_fips.data_ptr(), io_bits=io_bits)
    s, e, t = words(B, k, N), words(B, k, N), words(B, k, N)
    F.sample_cbd_dev(s.data_ptr(), B, sigma_ptr, eta1, first_nonce=0, per_seed=k, sigma_stride=64, io_bits=io_bits)
    F.sample_cbd_dev(e.data_ptr(), B, sigma_ptr, eta1, first_nonce=k, per_seed=k, sigma_stride=64, io_bits=io_bits)
    fma(A_hat.data_ptr(), s.data_ptr(), e.data_ptr(), t.data_ptr(), Q, N, B, k, k, 1, hat_stride=k * k * N, io_bits=io_bits)        # t = A s + e
    s_mod = canon(s).contiguous()
    st_hat, st_fips = images(2, B, k, N), words(2, B, k, N)
    T.gadget.ntt_forward_dev(t.data_ptr(), st_hat[0].data_ptr(), Q, N, B * k, io_bits=io_bits)
    T.gadget.ntt_forward_dev(s_mod.data_ptr(), st_hat[1].data_ptr(), Q, N, B * k, io_bits=io_bits)
    F.image_to_fips203_dev(st_fips.data_ptr(), 2 * B * k, st_hat.data_ptr(), io_bits=io_bits)
    key_bytes = u8(2, B, 384 * k)
    T.compression.byte_encode_dev(st_fips.data_ptr(), key_bytes.data_ptr(), 12, 2 * B * k * N, io_bits=io_bits)
    ek_dev = torch.cat([key_bytes[0], g_out[:, :32]], dim=1).contiguous()
    dk_dev = key_bytes[1].contiguous()
    torch.cuda.synchronize()
    for b in range(B):
        assert bytes(ek_dev[b].cpu().numpy()) == want[b][0], (name, "ek", b)
        assert bytes(dk_dev[b].cpu().numpy()) == want[b][1], (name, "dk", b)

    # K-PKE.Encrypt from the bytes of ek: t_hat crosses the boundary inwards
    t_fips, t_hat = words(B, k, N), images(B, k, N)
    ek_t = ek_dev[:, :384 * k].contiguous()
    T.compression.byte_decode_dev(ek_t.data_ptr(), t_fips.data_ptr(), Q, 12, B * k * N, io_bits=io_bits)
    F.image_from_fips203_dev(t_hat.data_ptr(), B * k, t_fips.data_ptr(), io_bits=io_bits)
    r_dev = torch.from_numpy(np.frombuffer(b"".join(rs), dtype=np.uint8).copy()).cuda()
    m_dev = torch.from_numpy(np.frombuffer(b"".join(ms), dtype=np.uint8).copy()).cuda()
    y, e1, e2, mu, u, v = words(B, k, N), words(B, k, N), words(B, 1, N), words(B, 1, N), words(B, k, N), words(B, 1, N)
    F.sample_cbd_dev(y.data_ptr(), B, r_dev.data_ptr(), eta1, first_nonce=0, per_seed=k, io_bits=io_bits)
    F.sample_cbd_dev(e1.data_ptr(), B, r_dev.data_ptr(), eta2, first_nonce=k, per_seed=k, io_bits=io_bits)
    F.sample_cbd_dev(e2.data_ptr(), B, r_dev.data_ptr(), eta2, first_nonce=2 * k, per_seed=1, io_bits=io_bits)
    T.compression.decode_decompress_dev(m_dev.data_ptr(), mu.data_ptr(), Q, 1, B * N, io_bits=io_bits)
    fma(A_hat.data_ptr(), y.data_ptr(), e1.data_ptr(), u.data_ptr(), Q, N, B, k, k, 1, hat_stride=k * k * N, trans_a=1, io_bits=io_bits)   # u = A^T y + e1
    e2mu = (e2 + mu).contiguous()
    fma(t_hat.data_ptr(), y.data_ptr(), e2mu.data_ptr(), v.data_ptr(), Q, N, B, 1, k, 1, hat_stride=k * N, trans_a=1, io_bits=io_bits)      # v = t^T y + e2 + mu
    c1, c2 = u8(B, 32 * du * k), u8(B, 32 * dv)
    T.compression.compress_encode_dev(u.data_ptr(), c1.data_ptr(), Q, du, B * k * N, io_bits=io_bits)
    T.compression.compress_encode_dev(v.data_ptr(), c2.data_ptr(), Q, dv, B * N, io_bits=io_bits)
    torch.cuda.synchronize()
    for b in range(B):
        assert bytes(c1[b].cpu().numpy()) + bytes(c2[b].cpu().numpy()) == want[b][2], (name, "ciphertext", b)

    # K-PKE.Decrypt from the bytes of dk and c
    s_fips, s_hat, u2, v2, w = words(B, k, N), images(B, k, N), words(B, k, N), words(B, 1, N), words(B, 1, N)
    T.compression.byte_decode_dev(dk_dev.data_ptr(), s_fips.data_ptr(), Q, 12, B * k * N, io_bits=io_bits)
    F.image_from_fips203_dev(s_hat.data_ptr(), B * k, s_fips.data_ptr(), io_bits=io_bits)
    T.compression.decode_decompress_dev(c1.data_ptr(), u2.data_ptr(), Q, du, B * k * N, io_bits=io_bits)
    T.compression.decode_decompress_dev(c2.data_ptr(), v2.data_ptr(), Q, dv, B * N, io_bits=io_bits)
    fma(s_hat.data_ptr(), u2.data_ptr(), v2.data_ptr(), w.data_ptr(), Q, N, B, 1, k, 1, hat_stride=k * N, trans_a=1, sign=-1, io_bits=io_bits)   # w = v - s^T u
    m_out = u8(B, 32)
    T.compression.compress_encode_dev(w.data_ptr(), m_out.data_ptr(), Q, 1, B * N, io_bits=io_bits)
    torch.cuda.synchronize()
    for b in range(B):
        assert bytes(m_out[b].cpu().numpy()) == ms[b], (name, "message", b)
