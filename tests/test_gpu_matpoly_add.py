"""Fused R_q matrix products on the device, C = E + sign * op(A) B (psf_matpoly_mul_add_*): bit for bit against the big-integer model
(tests/helpers/rq_fma_model.py) in every wave shape class, both word widths, both rings, both signs, every form of A; operands past the fold interval
with E at both ends of its range; the extremes of a 64-bit E; in-place accumulation; the degenerate cases against the product entry points; stream
order; and a K-PKE key generation, encryption and decryption that never leaves the device."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import rq_cyclic_model as MC
from tests.helpers import rq_fma_model as F
from tests.helpers import rq_model as M

pytestmark = pytest.mark.gpu

OK, ERR_PARAM, ERR_UNSUPPORTED = 0, 1, 8
RINGS = ("negacyclic", "cyclic")
# (q, n) with a wave kernel among the cases below: 2^(L+1) | q - 1 with a leaf degree n >> L of at most 4
WAVE = {(q, n) for q in (3329, 7681, 12289, 2013265921) for n in (128, 256, 512, 1024)} - {(3329, 1024)}
ROWS = {128: 9, 256: 9, 512: 5, 1024: 3}                                   # one full and one ragged row tile


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _dev(torch):
    return torch.device("cuda", 0)


def _t(torch, x):
    x = np.array(x, copy=True, order="C")
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    if x.dtype == np.uint16:
        x = x.view(np.int16)
    return torch.from_numpy(x).to(_dev(torch))


def _np(t, io):
    return t.cpu().numpy().view(np.uint64 if io == 64 else np.uint16).astype(np.uint64)


def _words(x, io, signed):
    return np.asarray(x).astype((np.int16 if signed else np.uint16) if io == 16 else (np.int64 if signed else np.uint64))


def _store(A, trans):
    return np.ascontiguousarray(np.transpose(A, (0, 2, 1, 3))) if trans else A


def _forward(T, ring, da, dh, q, n, count, io):
    if ring == "cyclic":
        T.rq.ntt_forward_cyclic_dev(da.data_ptr(), dh.data_ptr(), q, n, count, io_bits=io)
    else:
        T.gadget.ntt_forward_dev(da.data_ptr(), dh.data_ptr(), q, n, count, io_bits=io)


def run_fma(T, torch, ring, A_store, B, E, sign, q, n, rows, inner, cols, trans, shared, io=64, hat=False, in_place=False):
    """C through psf_matpoly_mul_add_*; A_store in storage order ((count or 1), rows x inner or inner x rows, n), B (count, inner, cols, n), E like C"""
    count, per = B.shape[0], rows * inner
    da, db, de = _t(torch, _words(A_store, io, False)), _t(torch, _words(B, io, True)), _t(torch, _words(E, io, True))
    dc = de if in_place else torch.full((count, rows, cols, n), -1, dtype=de.dtype, device=_dev(torch))
    suffix = "_cyclic" if ring == "cyclic" else ""
    if hat:
        dh = torch.empty((A_store.shape[0] * per, n), dtype=torch.int32, device=_dev(torch))
        _forward(T, ring, da, dh, q, n, A_store.shape[0] * per, io)
        getattr(T.rq, "matpoly_mul_add_hat" + suffix + "_dev")(dh.data_ptr(), db.data_ptr(), de.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols,
                                                                hat_stride=0 if shared else per * n, trans_a=trans, sign=sign, io_bits=io)
    else:
        getattr(T.rq, "matpoly_mul_add" + suffix + "_dev")(da.data_ptr(), db.data_ptr(), de.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols,
                                                            a_stride=0 if shared else per, trans_a=trans, sign=sign, io_bits=io)
    torch.cuda.synchronize()
    if not in_place:
        assert (_np(de, io) == _np(_t(torch, _words(E, io, True)), io)).all()      # E is only read
    return _np(dc, io)


def run_mul(T, torch, ring, A_store, B, q, n, rows, inner, cols, trans, shared, io=64):
    count, per = B.shape[0], rows * inner
    da, db = _t(torch, _words(A_store, io, False)), _t(torch, _words(B, io, True))
    dc = torch.full((count, rows, cols, n), -1, dtype=db.dtype, device=_dev(torch))
    fn = T.rq.matpoly_mul_cyclic_dev if ring == "cyclic" else T.rq.matpoly_mul_dev
    fn(da.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols, a_stride=0 if shared else per, trans_a=trans, io_bits=io)
    torch.cuda.synchronize()
    return _np(dc, io)


def _products(ring, A, B, q, shared):
    """the model's products of every batch: A (count, rows, inner, n) in its logical layout, batch 0 of it for every batch when shared"""
    return np.stack([F.RINGS[ring](A[0 if shared else c], B[c], q) for c in range(B.shape[0])])


@pytest.mark.parametrize("inner", [1, 3])
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("q", [3329, 7681, 12289, 2013265921])
@pytest.mark.parametrize("n", [128, 256, 512, 1024])
def test_every_wave_shape_against_the_model(T, torch, n, q, ring, inner):
    """rows = RT + 1, cols = 2, count = 3; trans_a 0 and 1, A shared and per batch, sign +1 and -1, 16- and 64-bit words.  (3329, 1024) has no wave
    kernel (leaf degree 8): its 64-bit words run the schoolbook kernel and its 16-bit words are PSF_ERR_UNSUPPORTED."""
    rng = np.random.default_rng([n, q % 65521, inner, ring == "cyclic"])
    rows, cols, count = ROWS[n], 2, 3
    A = rng.integers(0, q, size=(count, rows, inner, n), dtype=np.uint64)
    B = rng.integers(-q + 1, q, size=(count, inner, cols, n), dtype=np.int64)
    E = rng.integers(-q + 1, q, size=(count, rows, cols, n), dtype=np.int64)
    for shared in (True, False):
        P = _products(ring, A, B, q, shared)
        Au = A[:1] if shared else A
        for sign in (1, -1):
            want = F.add_signed(E, P, q, sign)
            for io in ((64, 16) if q < (1 << 14) else (64,)):
                for trans in (0, 1):
                    if io == 16 and (q, n) not in WAVE:
                        with pytest.raises(T.PsfError) as ei:
                            run_fma(T, torch, ring, _store(Au, trans), B, E, sign, q, n, rows, inner, cols, trans, shared, io)
                        assert ei.value.status == ERR_UNSUPPORTED
                        continue
                    got = run_fma(T, torch, ring, _store(Au, trans), B, E, sign, q, n, rows, inner, cols, trans, shared, io)
                    assert (got == want).all(), (shared, sign, io, trans)


@pytest.mark.parametrize("q,n,io", [(3329, 256, 64), (3329, 256, 16), (12289, 1024, 64), (12289, 1024, 16), (2013265921, 256, 64)])
def test_worst_case_operands_past_the_fold_interval(T, torch, q, n, io):
    """a = q - 1 everywhere, b = +-(q - 1) by coefficient parity, inner = 120 summands; E = q - 1 everywhere, then -(q - 1): e + x and e - x reach both
    corrections and both ends of their range.  The model's sum of 120 equal products is one exact product with 120 b."""
    rows, inner, cols = 2, 120, 1
    A = np.full((1, rows, inner, n), q - 1, dtype=np.uint64)
    par = np.where(np.arange(n) % 2 == 0, 1, -1)
    B = np.broadcast_to((q - 1) * par, (1, inner, cols, n)).astype(np.int64)
    for ring, conv in (("negacyclic", M.negacyclic), ("cyclic", MC.cyclic)):
        prod = conv(np.full(n, q - 1, dtype=object), (inner * (q - 1) * par).astype(object))
        P = np.broadcast_to(np.array([int(v) % q for v in prod], dtype=np.uint64), (1, rows, cols, n))
        for e in (q - 1, -(q - 1)):
            E = np.full((1, rows, cols, n), e, dtype=np.int64)
            for sign in (1, -1):
                want = F.add_signed(E, P, q, sign)
                for trans in (0, 1):
                    for hat in (False, True):
                        got = run_fma(T, torch, ring, _store(A, trans), B, E, sign, q, n, rows, inner, cols, trans, True, io, hat=hat)
                        assert (got == want).all(), (ring, e, sign, trans, hat)


@pytest.mark.parametrize("q,n", [(3329, 256), (2013265921, 256), (1 << 30, 8), (1 << 30, 256), ((1 << 62) - 57, 8), ((1 << 62) - 57, 256)])
def test_extremes_of_a_64_bit_addend(T, torch, q, n):
    """E cycles through INT64_MIN, INT64_MAX, -1, 0, q - 1 and q: the 16-bit and 32-bit wave forms and the schoolbook kernels of both rings"""
    rng = np.random.default_rng(n + q % 1000)
    rows, inner, cols, count = 2, 2, 1, 2
    A = rng.integers(0, q, size=(count, rows, inner, n), dtype=np.uint64)
    B = rng.integers(-q + 1, q, size=(count, inner, cols, n), dtype=np.int64)
    vals = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0, q - 1, q], dtype=np.int64)
    E = vals[(np.arange(count * rows * cols * n) + np.arange(count * rows * cols * n) // n) % 6].reshape(count, rows, cols, n)
    for ring in RINGS:
        P = _products(ring, A, B, q, False)
        for sign in (1, -1):
            got = run_fma(T, torch, ring, A, B, E, sign, q, n, rows, inner, cols, 0, False)
            assert (got == F.add_signed(E, P, q, sign)).all(), (ring, sign)


def test_hat_forms_equal_the_plain_form(T, torch):
    """images staged in LDS (one A for every batch, small), images in global memory per batch, and a shared A of 14 x 14 images of 1024 words that
    does not fit LDS; each against the plain fused form, and that against the product followed by the model's addition"""
    rng = np.random.default_rng(31)
    cases = [(3329, 256, 3, 5, 2, 3, 16), (3329, 256, 3, 5, 2, 3, 64), (7681, 512, 4, 4, 1, 2, 16), (2013265921, 1024, 3, 2, 2, 2, 64), (12289, 1024, 14, 14, 1, 2, 64),
             (12289, 1024, 14, 14, 1, 2, 16)]
    for q, n, rows, inner, cols, count, io in cases:
        A = rng.integers(0, q, size=(count, rows, inner, n), dtype=np.uint64)
        B = rng.integers(-q + 1, q, size=(count, inner, cols, n), dtype=np.int64)
        E = rng.integers(-q + 1, q, size=(count, rows, cols, n), dtype=np.int64)
        for ring in RINGS:
            for shared in (True, False):
                if rows == 14 and not shared:
                    continue
                Au = A[:1] if shared else A
                for trans, sign in ((0, 1), (1, -1)):
                    plain = run_fma(T, torch, ring, _store(Au, trans), B, E, sign, q, n, rows, inner, cols, trans, shared, io)
                    hat = run_fma(T, torch, ring, _store(Au, trans), B, E, sign, q, n, rows, inner, cols, trans, shared, io, hat=True)
                    assert (plain == hat).all(), (q, n, ring, shared, trans, io)
                    prod = run_mul(T, torch, ring, _store(Au, trans), B, q, n, rows, inner, cols, trans, shared, io)
                    assert (plain == F.add_signed(E, prod, q, sign)).all(), (q, n, ring, shared, trans, io)


def test_in_place_and_partial_overlap(T, torch):
    from tools_amd._ffi import lib
    rng = np.random.default_rng(32)
    for q, n, io in [(3329, 256, 16), (3329, 256, 64), (2013265921, 512, 64), (1 << 30, 64, 64)]:
        rows, inner, cols, count = 5, 3, 2, 3
        A = rng.integers(0, q, size=(count, rows, inner, n), dtype=np.uint64)
        B = rng.integers(-q + 1, q, size=(count, inner, cols, n), dtype=np.int64)
        E = rng.integers(0, q, size=(count, rows, cols, n), dtype=np.int64)
        for ring in RINGS:
            for sign in (1, -1):
                out = run_fma(T, torch, ring, A, B, E, sign, q, n, rows, inner, cols, 0, False, io)
                inp = run_fma(T, torch, ring, A, B, E, sign, q, n, rows, inner, cols, 0, False, io, in_place=True)
                assert (out == inp).all(), (q, n, io, ring, sign)
                if (q, n) in WAVE:
                    inh = run_fma(T, torch, ring, A, B, E, sign, q, n, rows, inner, cols, 0, False, io, hat=True, in_place=True)
                    assert (out == inh).all(), (q, n, io, ring, sign)
    # partial overlap: E one word into C
    q, n = 3329, 256
    da = torch.zeros((2 * 3, n), dtype=torch.int64, device=_dev(torch))
    db = torch.zeros((3, n), dtype=torch.int64, device=_dev(torch))
    buf = torch.full((2 * n + 8,), 12345, dtype=torch.int64, device=_dev(torch))
    for name in ("psf_matpoly_mul_add_negacyclic_dev", "psf_matpoly_mul_add_cyclic_dev"):
        for e_off in (8, 8 * (2 * n - 1)):
            rc = getattr(lib(), name)(0, q, n, 1, 2, 3, 1, C.c_void_p(da.data_ptr()), 0, 0, C.c_void_p(db.data_ptr()), C.c_void_p(buf.data_ptr() + e_off), 1,
                                      C.c_void_p(buf.data_ptr()), 64, None)
            torch.cuda.synchronize()
            assert rc == ERR_PARAM, (name, e_off)
            assert (buf == 12345).all(), (name, e_off)


def test_degenerate_cases_equal_the_products(T, torch):
    rng = np.random.default_rng(33)
    for q, n, io in [(3329, 256, 16), (12289, 512, 64), (2013265921, 128, 64), (17, 8, 64)]:
        rows, inner, cols, count = 3, 4, 2, 2
        A = rng.integers(0, q, size=(count, rows, inner, n), dtype=np.uint64)
        B = rng.integers(-q + 1, q, size=(count, inner, cols, n), dtype=np.int64)
        for ring in RINGS:
            # E = 0, sign = +1: the product, word for word
            zero = np.zeros((count, rows, cols, n), dtype=np.int64)
            assert (run_fma(T, torch, ring, A, B, zero, 1, q, n, rows, inner, cols, 0, False, io) ==
                    run_mul(T, torch, ring, A, B, q, n, rows, inner, cols, 0, False, io)).all(), (q, n, io, ring)
            # rows = inner = cols = 1: the pair product plus the model's addition
            a, b = A[:, 0, 0], B[:, 0, 0]
            e = rng.integers(-q + 1, q, size=(count, n), dtype=np.int64)
            da, db = _t(torch, _words(a, io, False)), _t(torch, _words(b, io, True))
            do = torch.empty_like(db)
            (T.rq.poly_mul_cyclic_dev if ring == "cyclic" else T.gadget.poly_mul_negacyclic_dev)(da.data_ptr(), db.data_ptr(), do.data_ptr(), q, n, count, io_bits=io)
            torch.cuda.synchronize()
            pair = _np(do, io)
            for sign in (1, -1):
                got = run_fma(T, torch, ring, a.reshape(count, 1, 1, n), b.reshape(count, 1, 1, n), e.reshape(count, 1, 1, n), sign, q, n, 1, 1, 1, 0, False, io)
                assert (got.reshape(count, n) == F.add_signed(e, pair, q, sign)).all(), (q, n, io, ring, sign)


def test_stream_order(T, torch):
    """fill, fused product, fused product in place: enqueued on one non-default stream without a host synchronisation in between"""
    dev = _dev(torch)
    q, n, k, count, eta, seed = 3329, 256, 3, 16, 2, 77
    from tests.helpers import sample_fill_model as S
    A = S.uniform_fill(seed, 64, 0, k * k, n, q)
    Bv, E1, E2 = (S.cbd_fill(seed, tag, 0, count * k, n, eta) for tag in (65, 66, 67))
    B2 = S.cbd_fill(seed, 68, 0, count * k, n, eta)
    s = torch.cuda.Stream()
    dA = torch.empty((k * k, n), dtype=torch.int16, device=dev)
    dB, dE1, dE2, dB2 = (torch.empty((count * k, n), dtype=torch.int16, device=dev) for _ in range(4))
    dC = torch.full((count * k, n), -1, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    sp = s.cuda_stream
    with torch.cuda.stream(s):
        big = torch.ones((1 << 26,), dtype=torch.float32, device=dev)
        for _ in range(4):
            big = big * 1.0001                                       # keeps the stream busy in front of the fills
        T.sample.sample_uniform_dev(dA.data_ptr(), k * k, n, q, seed, tag=64, io_bits=16, stream=sp)
        for d, tag in ((dB, 65), (dE1, 66), (dE2, 67), (dB2, 68)):
            T.sample.sample_cbd_dev(d.data_ptr(), count * k, n, eta, seed, tag=tag, io_bits=16, stream=sp)
        T.rq.matpoly_mul_add_dev(dA.data_ptr(), dB.data_ptr(), dE1.data_ptr(), dC.data_ptr(), q, n, count, k, k, 1, a_stride=0, io_bits=16, stream=sp)
        T.rq.matpoly_mul_add_dev(dA.data_ptr(), dB2.data_ptr(), dC.data_ptr(), dC.data_ptr(), q, n, count, k, k, 1, a_stride=0, trans_a=1, sign=-1, io_bits=16,
                                 stream=sp)
    s.synchronize()
    Am = A.reshape(k, k, n)
    want = np.empty((count, k, 1, n), dtype=np.uint64)
    for c in range(count):
        first = F.matpoly_mul_add(Am, Bv[c * k:(c + 1) * k].reshape(k, 1, n), E1[c * k:(c + 1) * k].reshape(k, 1, n), q, 1)
        want[c] = F.matpoly_mul_add(np.transpose(Am, (1, 0, 2)), B2[c * k:(c + 1) * k].reshape(k, 1, n), first, q, -1)
    assert (_np(dC, 16).reshape(count, k, 1, n) == want).all()


# ---- K-PKE (FIPS 203 without compression) on the device -------------------------------------------------------------------------------------------------
KPKE = dict(n=256, q=3329, k=3, eta=2, pairs=64, seed=20261018)
TAGS = dict(A=64, s=65, e=66, r=67, e1=68, e2=69)


def _decode_bits(w, q):
    """decode_digits at base 2: floor((2 c + floor(q / 4)) / q) mod 2"""
    return ((2 * w.astype(np.int64) + q // 4) // q) % 2


def kpke_cpu():
    """the whole flow through the fill model and the big-integer model: (bits, t, u, v, w) per pair"""
    from tests.helpers import sample_fill_model as S
    n, q, k, eta, pairs, seed = (KPKE[x] for x in ("n", "q", "k", "eta", "pairs", "seed"))
    A = S.uniform_fill(seed, TAGS["A"], 0, pairs * k * k, n, q).reshape(pairs, k, k, n)
    s, e, r, e1 = (S.cbd_fill(seed, TAGS[x], 0, pairs * k, n, eta).reshape(pairs, k, 1, n) for x in ("s", "e", "r", "e1"))
    e2 = S.cbd_fill(seed, TAGS["e2"], 0, pairs, n, eta).reshape(pairs, 1, 1, n)
    bits = np.random.default_rng(seed).integers(0, 2, size=(pairs, 1, 1, n), dtype=np.int64)
    mu = bits * (q // 2)
    t, u, v, w = (np.empty(sh, dtype=np.uint64) for sh in ((pairs, k, 1, n), (pairs, k, 1, n), (pairs, 1, 1, n), (pairs, 1, 1, n)))
    for c in range(pairs):
        t[c] = F.matpoly_mul_add(A[c], s[c], e[c], q, 1)
        u[c] = F.matpoly_mul_add(np.transpose(A[c], (1, 0, 2)), r[c], e1[c], q, 1)
        v[c] = F.matpoly_mul_add(np.transpose(t[c], (1, 0, 2)), r[c], e2[c] + mu[c], q, 1)
        w[c] = F.matpoly_mul_add(np.transpose(u[c], (1, 0, 2)), s[c], v[c], q, -1)
    return bits, t, u, v, w


def test_kpke_round_trip(T, torch):
    """n = 256, q = 3329, k = 3, eta = 2, 16-bit words, 64 independent key / message pairs: t = A s + e, u = A^T r + e1, v = t^T r + (e2 + mu),
    w = v - u^T s, every fill, product and coding on the device.  The seeded inputs decode without error in the CPU flow (checked here first, so the
    test rests on no probability), the device's t, u, v, w equal that flow word for word, and the decoded bits are the message: zero wrong bits."""
    n, q, k, eta, pairs, seed = (KPKE[x] for x in ("n", "q", "k", "eta", "pairs", "seed"))
    bits, t, u, v, w = kpke_cpu()
    assert (_decode_bits(w, q) == bits).all()
    dev = _dev(torch)
    i16 = dict(dtype=torch.int16, device=dev)
    dA = torch.empty((pairs, k, k, n), **i16)
    ds, de, dr, de1, dt, du = (torch.empty((pairs, k, 1, n), **i16) for _ in range(6))
    de2, dmu, dv, dw, dbits, dgot = (torch.empty((pairs, 1, 1, n), **i16) for _ in range(6))
    dbits.copy_(torch.from_numpy(bits.astype(np.int16)))
    T.sample.sample_uniform_dev(dA.data_ptr(), pairs * k * k, n, q, seed, tag=TAGS["A"], io_bits=16)
    for d, x in ((ds, "s"), (de, "e"), (dr, "r"), (de1, "e1")):
        T.sample.sample_cbd_dev(d.data_ptr(), pairs * k, n, eta, seed, tag=TAGS[x], io_bits=16)
    T.sample.sample_cbd_dev(de2.data_ptr(), pairs, n, eta, seed, tag=TAGS["e2"], io_bits=16)
    T.encodings.encode_digits_dev(dbits.data_ptr(), dmu.data_ptr(), q, 2, pairs * n, io_bits=16)
    fma = T.rq.matpoly_mul_add_dev
    fma(dA.data_ptr(), ds.data_ptr(), de.data_ptr(), dt.data_ptr(), q, n, pairs, k, k, 1, a_stride=k * k, io_bits=16)                       # t = A s + e
    fma(dA.data_ptr(), dr.data_ptr(), de1.data_ptr(), du.data_ptr(), q, n, pairs, k, k, 1, a_stride=k * k, trans_a=1, io_bits=16)           # u = A^T r + e1
    de2.add_(dmu)                                                                                                                          # E = e2 + mu, in (-q, q)
    fma(dt.data_ptr(), dr.data_ptr(), de2.data_ptr(), dv.data_ptr(), q, n, pairs, 1, k, 1, a_stride=k, trans_a=1, io_bits=16)               # v = t^T r + E
    fma(du.data_ptr(), ds.data_ptr(), dv.data_ptr(), dw.data_ptr(), q, n, pairs, 1, k, 1, a_stride=k, trans_a=1, sign=-1, io_bits=16)       # w = v - u^T s
    T.encodings.decode_digits_dev(dw.data_ptr(), dgot.data_ptr(), q, 2, pairs * n, io_bits=16)
    torch.cuda.synchronize()
    for name, d, want in (("t", dt, t), ("u", du, u), ("v", dv, v), ("w", dw, w)):
        assert (_np(d, 16).reshape(want.shape) == want).all(), name
    assert (_np(dgot, 16).reshape(bits.shape) == bits.astype(np.uint64)).all()


# ---- the schoolbook matrix kernels above the default LDS limit --------------------------------------------------------------------------------------------
BIG = dict(n=8192, q=1 << 30, rows=1, inner=2, cols=2, seed=20260731)


def _big_case():
    """A dense residues; every polynomial of B with at most 8 non-zero signed coefficients, degrees 0 and n - 1 among them; E any int64"""
    n, q, rows, inner, cols = (BIG[x] for x in ("n", "q", "rows", "inner", "cols"))
    rng = np.random.default_rng(BIG["seed"])
    A = rng.integers(0, q, size=(rows, inner, n), dtype=np.uint64)
    B = np.zeros((inner, cols, n), dtype=np.int64)
    for k in range(inner):
        for j in range(cols):
            deg = np.concatenate(([0, n - 1], rng.choice(np.arange(1, n - 1), size=6, replace=False)))
            mag = rng.integers(1, q, size=deg.size, dtype=np.int64)
            B[k, j, deg] = mag * rng.choice(np.array([-1, 1], dtype=np.int64), size=deg.size)
    B[0, 0, 0], B[0, 0, n - 1], B[1, 1, 0], B[1, 1, n - 1] = q - 1, -(q - 1), -(q - 1), q - 1     # both signs at both ends
    E = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=(rows, cols, n), dtype=np.int64, endpoint=True)
    return A, B, E


def _sparse_product(A, B, q, wrap):
    """A B mod (X^n - wrap, q) by one shifted add per non-zero coefficient of B.  Exact in int64: a term a * |b| is below 2^60 and is reduced mod q
    before it is added to a sum that is kept in [0, q)."""
    rows, inner, n = A.shape
    cols = B.shape[1]
    assert q <= 1 << 30 and int(A.max()) < q and int(np.abs(B).max()) < q
    out = np.zeros((rows, cols, n), dtype=np.int64)
    for i in range(rows):
        for j in range(cols):
            for k in range(inner):
                for d in np.flatnonzero(B[k, j]).tolist():
                    b = int(B[k, j, d])
                    t = np.roll(((A[i, k] * np.uint64(abs(b))) % np.uint64(q)).astype(np.int64), d)      # X^d a: coefficient c - d at c, the last d wrapped
                    t[:d] *= wrap
                    out[i, j] = np.mod(out[i, j] + (t if b > 0 else -t), q)
    return out


@pytest.fixture(scope="module")
def big_case():
    A, B, E = _big_case()
    q = BIG["q"]
    return A, B, E, {ring: _sparse_product(A, B, q, wrap) for ring, wrap in (("negacyclic", -1), ("cyclic", 1))}


def test_shifted_add_reference_equals_the_model_at_a_small_size():
    """the reference of the next test against the big-integer models, where those are quick (n = 64, the same modulus and kind of operands)"""
    q, n = BIG["q"], 64
    rng = np.random.default_rng(5)
    A = rng.integers(0, q, size=(2, 2, n), dtype=np.uint64)
    B = np.zeros((2, 2, n), dtype=np.int64)
    for k in range(2):
        for j in range(2):
            deg = np.concatenate(([0, n - 1], rng.choice(np.arange(1, n - 1), size=6, replace=False)))
            B[k, j, deg] = rng.integers(1, q, size=8, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=8)
    assert (_sparse_product(A, B, q, -1).astype(np.uint64) == M.matpoly_mul(A, B, q)).all()
    assert (_sparse_product(A, B, q, 1).astype(np.uint64) == MC.matpoly_mul(A, B, q)).all()


def test_schoolbook_matrix_kernels_above_the_default_lds_limit(T, big_case):
    """n = 8192 at q = 2^30 (no NTT; 128-bit accumulation): the four schoolbook matrix kernels run with 128 KiB of dynamic LDS, above the 64 KiB a
    kernel gets by default.  Host forms, bit for bit; each entry twice -- the first call raises the kernel's limit, the second finds it raised."""
    A, B, E, P = big_case
    q = BIG["q"]
    want = {
        "matpoly_mul": P["negacyclic"],
        "matpoly_mul_cyclic": P["cyclic"],
        "matpoly_mul_add": np.mod(np.mod(E, q) - P["negacyclic"], q),
        "matpoly_mul_add_cyclic": np.mod(np.mod(E, q) + P["cyclic"], q),
    }
    calls = {
        "matpoly_mul": lambda: T.rq.matpoly_mul(A, B, q),
        "matpoly_mul_cyclic": lambda: T.rq.matpoly_mul_cyclic(A, B, q),
        "matpoly_mul_add": lambda: T.rq.matpoly_mul_add(A, B, E, q, sign=-1),
        "matpoly_mul_add_cyclic": lambda: T.rq.matpoly_mul_add_cyclic(A, B, E, q, sign=1),
    }
    for name, call in calls.items():
        for attempt in (1, 2):
            got = call()
            assert got.dtype == np.uint64 and (got == want[name].astype(np.uint64)).all(), (name, attempt)
