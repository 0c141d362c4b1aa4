"""The uniform, centred-binomial and discrete-Gaussian fills on the MI355X, bit for bit against the CPU oracle (orc_uniform_mod, orc_sample_z)
and the centred-binomial model (tests/helpers/sample_fill_model.py): every word size, shapes that leave partial blocks, tiles and vectors,
every pointer offset with guard bytes around each output, the attempt cap and the failure flag, indices across 2^32, sharding, streams, the
host forms, and A s + e composed with the R_q products.  Every comparison is exact equality; there is no statistical threshold."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.helpers import rq_model
from tests.helpers import sample_fill_model as M

pytestmark = pytest.mark.gpu

GUARD = 64                 # bytes before and after every output buffer (a multiple of 16: it does not change the alignment)
FILL = 0xA5
SEED = 0x5EED5EED12345678
ERR_SAMPLER = 9


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


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


def _flag(torch, value=0):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


def fill(T, torch, kind, count, n, io_bits, off=0, stream=None, **kw):
    """one device fill into a guarded buffer whose pointer is `off` words past a 16-byte boundary; returns the (count, n) array"""
    wb = io_bits // 8
    nbytes = count * n * wb
    buf, ptr = _out(torch, nbytes, off * wb)
    torch.cuda.synchronize()
    {"uniform": T.sample.sample_uniform_dev, "cbd": T.sample.sample_cbd_dev, "gauss": T.sample.sample_discrete_gauss_dev}[kind](
        ptr, count, n, io_bits=io_bits, stream=stream, **kw)
    raw = _take(torch, buf, nbytes, off * wb, (kind, count, n, io_bits, off, kw))
    if kind == "uniform":
        return raw.view(np.uint16 if io_bits == 16 else np.uint64).reshape(count, n)
    return raw.view(np.int16 if io_bits == 16 else np.int64).reshape(count, n).astype(np.int64)


# ---- uniform -------------------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (3, 255), (5, 256), (2, 1031), (64, 256)]


Q_REDRAW = (1 << 64) // 5 + 1      # 2^64 mod q = q - 5: a fifth of the draws are redrawn (at 2^62 - 57 it is 228: practically never)


@pytest.mark.parametrize("q", [2, 3329, 65521, 1 << 30, 1073741789, (1 << 62) - 57, Q_REDRAW])
def test_uniform_against_the_oracle(T, torch, q):
    redrawn = 0
    for count, n in SHAPES:
        want = M.uniform_fill(SEED, 70, 5, count, n, q)
        assert int(want.max()) < q
        got = fill(T, torch, "uniform", count, n, 64, q=q, seed=SEED, tag=70, first_index=5)
        assert np.array_equal(got, want), (q, count, n)
        if q <= 1 << 16:
            got16 = fill(T, torch, "uniform", count, n, 16, off=3, q=q, seed=SEED, tag=70, first_index=5)
            assert np.array_equal(got16.astype(np.uint64), want), (q, count, n)
        if (count, n) == (64, 256) and q == Q_REDRAW:                       # 2^14 coefficients: about a fifth take the redraw path
            w = M.philox_np(SEED, np.arange(n, dtype=np.uint64)[None, :], (5 + np.arange(count, dtype=np.uint64))[:, None], np.uint64(0), np.uint64(70))
            first = [(int(hi) << 32 | int(lo)) * q >> 64 for lo, hi in zip(w[0].ravel(), w[1].ravel())]
            redrawn = int((np.array(first, dtype=np.uint64) != want.ravel()).sum())
    if q == Q_REDRAW:
        assert redrawn > 2000, redrawn


def test_uniform_long_ragged_fill(T, torch):
    """2^20 + 77 coefficients at 64-bit words: more vectors than the largest grid has lanes, so the grid-stride loop runs, with a ragged end"""
    n = (1 << 20) + 77
    want = M.uniform_fill(SEED, 64, 0, 1, n, 3329)
    got = fill(T, torch, "uniform", 1, n, 64, off=1, q=3329, seed=SEED, tag=64)
    assert np.array_equal(got, want)


# ---- centred binomial ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io_bits", [16, 64])
@pytest.mark.parametrize("eta", [1, 2, 3, 5, 8, 16])
def test_cbd_against_the_model(T, torch, eta, io_bits):
    for n in (1, 19, 20, 21, 23, 256, 257):
        for count in (1, 3, 65):
            want = M.cbd_fill(SEED, 100 + eta, 7, count, n, eta)
            got = fill(T, torch, "cbd", count, n, io_bits, eta=eta, seed=SEED, tag=100 + eta, first_index=7)
            assert np.array_equal(got, want), (eta, io_bits, n, count)
    want = M.cbd_fill(SEED, 100 + eta, 7, 65, 257, eta)                     # 16 705 values: whole tiles, a head and a ragged end
    assert abs(int(want.min())) <= eta and int(want.max()) <= eta and want.min() < 0 < want.max()
    for off in range(16 // (io_bits // 8)):
        got = fill(T, torch, "cbd", 65, 257, io_bits, off=off, eta=eta, seed=SEED, tag=100 + eta, first_index=7)
        assert np.array_equal(got, want), (eta, io_bits, off)


def test_cbd_long_fill(T, torch):
    n = (1 << 22) + 77
    want = M.cbd_fill(SEED, 64, 0, 1, n, 3)
    got = fill(T, torch, "cbd", 1, n, 16, eta=3, seed=SEED, tag=64)
    assert np.array_equal(got, want)


# ---- discrete Gaussian, shared centre ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gauss_ref(count, n, center, s, tag, first_index=0):
    return M.gauss_fill(SEED, tag, first_index, count, n, s, center=center)


@pytest.mark.parametrize("center,s,count", [(0.0, 8.0, 1024), (0.5, 8.0, 1024), (-3.25, 1.5, 1024), (1000.75, 300.0, 1024), (0.0, 341.2, 1024),
                                            (0.0, 341.4, 1024), (12345.5, 50000.0, 64)])
def test_gauss_shared_centre_against_the_oracle(T, torch, center, s, count):
    """2^18 coefficients per case (2^14 at the widest).  The narrow cases replay their attempts in the model and assert that the fill met ties
    (wb == floor(rho 2^16)) and Lemire voids, so the inputs provably reach those paths.  At s = 341.2 there are exactly 4096 candidates and
    2^16 mod 4096 = 0: no attempt can be void there, whatever the size of the fill, and the test asserts that count is 0."""
    n = 256
    want, failed = _gauss_ref(count, n, center, s, 80)
    assert not failed
    narrow = s <= 341.2
    if narrow:
        traced, ties, voids = M.gauss_narrow_trace(SEED, 80, 0, count, n, center, s)
        assert np.array_equal(traced, want)
        print(f"c = {center}, s = {s}: {ties} ties, {voids} voids")
        assert ties > 0
        if s == 341.2:
            assert voids == 0 and 65536 % 4096 == 0
        else:
            assert voids > 0
    flag = _flag(torch)
    got = fill(T, torch, "gauss", count, n, 64, s=s, center=center, seed=SEED, tag=80, d_fail=flag.data_ptr())
    assert np.array_equal(got, want), (center, s)
    if abs(center) + 6 * s + 1 < 32768:
        got16 = fill(T, torch, "gauss", count, n, 16, off=5, s=s, center=center, seed=SEED, tag=80, d_fail=flag.data_ptr())
        assert np.array_equal(got16, want), (center, s)
    assert int(flag.item()) == 0


# ---- discrete Gaussian, per-element centres -------------------------------------------------------------------------------------------------------

def _centres():
    rng = np.random.default_rng(2024)
    cen = rng.uniform(-50.0, 50.0, size=1 << 16)
    cen[1000:1256] = np.round(cen[1000:1256])                               # exact integers
    cen[2000:2256] = np.floor(cen[2000:2256]) + 0.5                         # half integers
    big = np.where(rng.integers(0, 2, size=256) == 1, 1.0, -1.0) * 2.0 ** 40
    cen[3000:3256] = big + np.round(rng.uniform(-8.0, 8.0, size=256) * 4) / 4
    return cen


@pytest.mark.parametrize("s", [1.5, 8.0, 400.0])
def test_gauss_per_element_centres(T, torch, s):
    cen = _centres()
    count, n = 256, 256
    want, failed = M.gauss_fill(SEED, 90, 3, count, n, s, centers=cen)
    assert not failed
    d_cen = torch.from_numpy(cen).cuda()
    flag = _flag(torch)
    got = fill(T, torch, "gauss", count, n, 64, off=1, s=s, center=float("nan"), d_centers=d_cen.data_ptr(), seed=SEED, tag=90, first_index=3,
               d_fail=flag.data_ptr())
    assert np.array_equal(got, want), s
    assert int(flag.item()) == 0
    assert np.abs(got.ravel()[3000:3256]).min() > 2 ** 39


def test_gauss_centre_beyond_2_62_writes_0_and_raises_the_flag(T, torch):
    cen = _centres()[:4096].copy()
    cen[1234] = 2.0 ** 63
    want, failed = M.gauss_fill(SEED, 91, 0, 16, 256, 8.0, centers=cen)
    assert failed and want.ravel()[1234] == 0
    d_cen = torch.from_numpy(cen).cuda()
    flag = _flag(torch)
    got = fill(T, torch, "gauss", 16, 256, 64, s=8.0, d_centers=d_cen.data_ptr(), seed=SEED, tag=91, d_fail=flag.data_ptr())
    assert np.array_equal(got, want)
    assert int(flag.item()) == 1
    with pytest.raises(T.PsfError) as ei:
        T.sample.sample_discrete_gauss(16, 256, 8.0, seed=SEED, centers=cen, tag=91)
    assert ei.value.status == ERR_SAMPLER


# ---- the attempt cap ------------------------------------------------------------------------------------------------------------------------------

def test_attempt_cap(T, torch):
    """s = 0.05, c = 0.5: one candidate, acceptance ~e^-314, every draw runs the contract's 65 536 attempts and ends with floor(c + 1/2) = 1.
    A defined result of the contract, not a fault; 64 coefficients."""
    for per_element in (False, True):
        d_cen = torch.full((64,), 0.5, dtype=torch.float64, device="cuda") if per_element else None
        for before in (0, 1):
            flag = _flag(torch, before)
            got = fill(T, torch, "gauss", 1, 64, 64, s=0.05, center=0.5, d_centers=d_cen.data_ptr() if per_element else None, seed=SEED, tag=64,
                       d_fail=flag.data_ptr())
            assert (got == 1).all()
            assert int(flag.item()) == 1
        got = fill(T, torch, "gauss", 1, 64, 64, s=0.05, center=0.5, d_centers=d_cen.data_ptr() if per_element else None, seed=SEED, tag=64)
        assert (got == 1).all()                                             # a NULL flag
    with pytest.raises(T.PsfError) as ei:
        T.sample.sample_discrete_gauss(1, 64, 0.05, seed=SEED, center=0.5)
    assert ei.value.status == ERR_SAMPLER
    flag = _flag(torch, 0)                                                  # the same fill at c = 0: candidate 0 always accepts
    got = fill(T, torch, "gauss", 1, 64, 64, s=0.05, center=0.0, seed=SEED, tag=64, d_fail=flag.data_ptr())
    want, failed = M.gauss_fill(SEED, 64, 0, 1, 64, 0.05, center=0.0)
    assert not failed and np.array_equal(got, want) and (got == 0).all()
    assert int(flag.item()) == 0
    assert (T.sample.sample_discrete_gauss(1, 64, 0.05, seed=SEED, center=0.0) == 0).all()


# ---- index and sharding ----------------------------------------------------------------------------------------------------------------------------

def _three(T, torch, count, n, first_index, tag, io_bits=64, off=0):
    return (fill(T, torch, "uniform", count, n, io_bits, off=off, q=3329, seed=SEED, tag=tag, first_index=first_index),
            fill(T, torch, "cbd", count, n, io_bits, off=off, eta=3, seed=SEED, tag=tag, first_index=first_index),
            fill(T, torch, "gauss", count, n, io_bits, off=off, s=8.0, center=0.5, seed=SEED, tag=tag, first_index=first_index),
            fill(T, torch, "gauss", count, n, 64, off=off, s=400.0, center=0.5, seed=SEED, tag=tag, first_index=first_index))


def test_index_across_2_32(T, torch):
    first, count, n = (1 << 32) - 2, 4, 300
    for io_bits in (64, 16):
        u, c, g, gw = _three(T, torch, count, n, first, 200, io_bits)
        assert np.array_equal(u.astype(np.uint64), M.uniform_fill(SEED, 200, first, count, n, 3329))
        assert np.array_equal(c, M.cbd_fill(SEED, 200, first, count, n, 3))
        assert np.array_equal(g, M.gauss_fill(SEED, 200, first, count, n, 8.0, center=0.5)[0])
        assert np.array_equal(gw, M.gauss_fill(SEED, 200, first, count, n, 400.0, center=0.5)[0])
        assert not np.array_equal(u[1], u[2]) and not np.array_equal(c[1], c[2])


def test_sharding_and_tags(T, torch):
    n = 261
    whole = _three(T, torch, 8, n, 40, 64)
    a = _three(T, torch, 3, n, 40, 64, off=1)
    b = _three(T, torch, 5, n, 43, 64)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))
    other = _three(T, torch, 8, n, 40, 65)
    for w, o in zip(whole, other):
        assert not np.array_equal(w, o)
        assert (w != o).mean() > 0.5


def test_a_fill_leaves_the_handles_streams_alone(T, torch):
    from oracle import oracle as O
    n, q, B = 8, 64, 6
    psf = T.PSFPerturbation(T.GadgetParameters.init_default(n, q), 3.0, 25.0, device=0)
    psf.trap_gen(seed=1)
    u = torch.from_numpy(O.uniform_targets(7, B, n, q).astype(np.int64)).cuda()
    e0 = torch.zeros((B, psf.m), dtype=torch.int64, device="cuda")
    e1 = torch.zeros_like(e0)
    psf.samp_p_dev(u.data_ptr(), e0.data_ptr(), B, seed=SEED, first_index=0)
    torch.cuda.synchronize()
    fill(T, torch, "cbd", 16, 256, 64, eta=2, seed=SEED, tag=64)
    psf.samp_p_dev(u.data_ptr(), e1.data_ptr(), B, seed=SEED, first_index=0)
    torch.cuda.synchronize()
    assert torch.equal(e0, e1) and bool((e0 != 0).any())


# ---- streams and host forms ------------------------------------------------------------------------------------------------------------------------

def test_stream_order(T, torch):
    """a kernel that overwrites the buffer precedes the fill on a non-default stream: the fill's values must be what is left"""
    count, n = 512, 256
    want = M.cbd_fill(SEED, 64, 0, count, n, 2)
    wantg = M.gauss_fill(SEED, 64, 0, 16, n, 8.0)[0]
    s = torch.cuda.Stream()
    big = torch.zeros(1 << 24, dtype=torch.int64, device="cuda")
    out = torch.zeros(count * n, dtype=torch.int16, device="cuda")
    outg = torch.zeros(16 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big.add_(1)                                                         # keeps the stream busy
        out.fill_(77)
        outg.fill_(77)
        T.sample.sample_cbd_dev(out.data_ptr(), count, n, 2, SEED, io_bits=16, stream=s.cuda_stream)
        T.sample.sample_discrete_gauss_dev(outg.data_ptr(), 16, n, 8.0, SEED, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(count, n).astype(np.int64), want)
    assert np.array_equal(outg.cpu().numpy().reshape(16, n), wantg)


def test_host_forms_equal_the_device_forms(T, torch):
    count, n, first = 5, 259, 11
    u, c, g, gw = _three(T, torch, count, n, first, 130)
    assert np.array_equal(T.sample.sample_uniform(count, n, 3329, SEED, tag=130, first_index=first), u)
    assert np.array_equal(T.sample.sample_cbd(count, n, 3, SEED, tag=130, first_index=first), c)
    assert np.array_equal(T.sample.sample_discrete_gauss(count, n, 8.0, SEED, center=0.5, tag=130, first_index=first), g)
    assert np.array_equal(T.sample.sample_discrete_gauss(count, n, 400.0, SEED, center=0.5, tag=130, first_index=first), gw)
    cen = _centres()[: count * n]
    d_cen = torch.from_numpy(cen).cuda()
    dev = fill(T, torch, "gauss", count, n, 64, s=8.0, d_centers=d_cen.data_ptr(), seed=SEED, tag=130, first_index=first)
    assert np.array_equal(T.sample.sample_discrete_gauss(count, n, 8.0, SEED, centers=cen, tag=130, first_index=first), dev)
    for n in (1, 7, 9):                                                 # below one 16-byte vector, and no whole number of them
        u, c, g, gw = _three(T, torch, 1, n, first, 130)
        assert np.array_equal(T.sample.sample_uniform(1, n, 3329, SEED, tag=130, first_index=first), u), n
        assert np.array_equal(T.sample.sample_cbd(1, n, 3, SEED, tag=130, first_index=first), c), n
        assert np.array_equal(T.sample.sample_discrete_gauss(1, n, 8.0, SEED, center=0.5, tag=130, first_index=first), g), n
        assert np.array_equal(T.sample.sample_discrete_gauss(1, n, 400.0, SEED, center=0.5, tag=130, first_index=first), gw), n


# ---- composition ------------------------------------------------------------------------------------------------------------------------------------

def test_a_s_plus_e(T, torch):
    """b = A s + e at n = 256, q = 3329, k = 2: uniform A, centred-binomial s and e from two tags, the hat product, the addition in torch"""
    n, q, k = 256, 3329, 2
    dA = torch.zeros(k * k * n, dtype=torch.int64, device="cuda")
    ds = torch.zeros(k * n, dtype=torch.int64, device="cuda")
    de = torch.zeros(k * n, dtype=torch.int64, device="cuda")
    dhat = torch.zeros(k * k * n, dtype=torch.int32, device="cuda")
    dc = torch.zeros(k * n, dtype=torch.int64, device="cuda")
    T.sample.sample_uniform_dev(dA.data_ptr(), k * k, n, q, SEED, tag=64)
    T.sample.sample_cbd_dev(ds.data_ptr(), k, n, 2, SEED, tag=65)
    T.sample.sample_cbd_dev(de.data_ptr(), k, n, 2, SEED, tag=66)
    T.gadget.ntt_forward_dev(dA.data_ptr(), dhat.data_ptr(), q, n, k * k, io_bits=64)
    T.rq.matpoly_mul_hat_dev(dhat.data_ptr(), ds.data_ptr(), dc.data_ptr(), q, n, 1, k, k, 1, io_bits=64)
    b = torch.remainder(dc + de, q)
    torch.cuda.synchronize()
    A, sv, ev = dA.cpu().numpy().reshape(k, k, n), ds.cpu().numpy().reshape(k, 1, n), de.cpu().numpy().reshape(k, 1, n)
    assert np.array_equal(A.astype(np.uint64), M.uniform_fill(SEED, 64, 0, k * k, n, q).reshape(k, k, n))
    assert np.array_equal(sv.ravel(), M.cbd_fill(SEED, 65, 0, k, n, 2).ravel()) and not np.array_equal(sv, ev)
    want = (rq_model.matpoly_mul(A, sv, q).astype(np.int64) + ev) % q
    assert np.array_equal(b.cpu().numpy().reshape(k, 1, n), want)
