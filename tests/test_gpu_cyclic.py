"""Products of the cyclic ring Z_q[X]/(X^n - 1) on the device (psf_*_cyclic*, new_cyclic of common_moduli.rs:72-79) against the big-integer model
(tests/helpers/rq_cyclic_model.py): pair products on every wave shape, the generic LDS route and schoolbook-only moduli, in both word widths, the NTT
method against the schoolbook method; image products; matrix products in the plain, image and host forms; full-size identities at X = 1 and X = -1 and
against the negacyclic ring; plans of both rings for the same (device, q, n) in one process; a non-default stream."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import rq_cyclic_model as M
from tests.helpers import rq_model as MN
from tests.test_gpu_matpoly import DIMS, GENERIC, WAVE, _np, _store, _t

pytestmark = pytest.mark.gpu

SCHOOL = [(1 << 30, 64), ((1 << 61) - 1, 32), (64, 16), ((1 << 62) - 57, 24)]      # no NTT: the cyclic schoolbook kernel
I64 = np.iinfo(np.int64)
U64 = np.iinfo(np.uint64)


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


def _route16(q, n):
    return q < (1 << 14) and (q, n) in WAVE


def _out(t, io):
    return _np(t, np.uint64 if io == 64 else np.uint16).astype(np.uint64)


def _pair_operands(rng, q, n, count, io, kind):
    """kind 0: random in range; 1: a = q - 1, b = +-(q - 1) by parity; 2: a = q - 1, b = q - 1; 3 (64-bit): any uint64 / int64 with the extremes"""
    if kind == 0:
        a = rng.integers(0, q, size=(count, n), dtype=np.uint64)
        b = rng.integers(-q + 1, q, size=(count, n), dtype=np.int64)
    elif kind in (1, 2):
        a = np.full((count, n), q - 1, dtype=np.uint64)
        sign = np.where(np.arange(n) % 2 == 0, 1, -1) if kind == 1 else np.ones(n, dtype=np.int64)
        b = np.ascontiguousarray(np.broadcast_to((q - 1) * sign, (count, n))).astype(np.int64)
    else:
        a = rng.integers(0, U64.max, size=(count, n), dtype=np.uint64, endpoint=True)
        b = rng.integers(I64.min, I64.max, size=(count, n), dtype=np.int64, endpoint=True)
        a.reshape(-1)[:3] = [U64.max, 0, q - 1]
        b.reshape(-1)[:4] = [I64.min, I64.max, -(q - 1), q - 1]
    if io == 16:
        a, b = a.astype(np.uint16), b.astype(np.int16)
    return a, b


def pair_dev(T, torch, a, b, q, n, io=64):
    da, db = _t(torch, a), _t(torch, b)
    do = torch.full(a.shape, -1, dtype=da.dtype, device=_dev(torch))
    T.rq.poly_mul_cyclic_dev(da.data_ptr(), db.data_ptr(), do.data_ptr(), q, n, a.shape[0], io_bits=io)
    torch.cuda.synchronize()
    return _out(do, io)


def test_pair_products_against_the_model(T, torch):
    rng = np.random.default_rng(31)
    for q, n in WAVE + GENERIC + SCHOOL:
        count = 2 if n >= 1024 else 3
        for io in ((64, 16) if _route16(q, n) else (64,)):
            for kind in ((0, 1, 2, 3) if io == 64 else (0, 1, 2)):
                a, b = _pair_operands(rng, q, n, count, io, kind)
                assert (pair_dev(T, torch, a, b, q, n, io) == M.poly_mul(a, b, q)).all(), (q, n, io, kind)
        # the host form, and the NTT method against the schoolbook method bit for bit
        a, b = _pair_operands(rng, q, n, count, 64, 3)
        want = M.poly_mul(a, b, q)
        assert (T.rq.poly_mul_cyclic(a, b, q) == want).all(), (q, n)
        assert (T.rq.poly_mul_cyclic(a, b, q, method=0) == want).all(), (q, n)
        if (q, n) in WAVE or (q, n) in GENERIC:
            assert (T.rq.poly_mul_cyclic(a, b, q, method=1) == want).all(), (q, n)
        else:
            with pytest.raises(T.PsfError):
                T.rq.poly_mul_cyclic(a, b, q, method=1)


def test_largest_n_both_methods_and_evaluations(T, torch):
    """n = 8192 (the schoolbook kernel's LDS above the default limit): the NTT (LDS route) and the schoolbook method agree for q = 12289; for
    schoolbook-only moduli the product's values at X = 1 and X = -1 are a(1) b(1) and a(-1) b(-1)"""
    rng = np.random.default_rng(32)
    n = 8192
    a, b = _pair_operands(rng, 12289, n, 2, 64, 0)
    assert (T.rq.poly_mul_cyclic(a, b, 12289, method=0) == T.rq.poly_mul_cyclic(a, b, 12289, method=1)).all()
    alt = np.where(np.arange(n) % 2 == 0, 1, -1).astype(object)
    for q in (1 << 30, (1 << 61) - 1):
        a, b = _pair_operands(rng, q, n, 2, 64, 3)
        c = T.rq.poly_mul_cyclic(a, b, q)
        for r in range(2):
            A, B, Cc = a[r].astype(object), b[r].astype(object), c[r].astype(object)
            assert int(Cc.sum()) % q == int(A.sum()) * int(B.sum()) % q
            assert int((Cc * alt).sum()) % q == int((A * alt).sum()) * int((B * alt).sum()) % q


def test_image_products_equal_the_direct_product(T, torch):
    rng = np.random.default_rng(33)
    dev = _dev(torch)
    for q, n in WAVE:
        for io in ((64, 16) if _route16(q, n) else (64,)):
            count = 5
            a, b = _pair_operands(rng, q, n, count, io, 0)
            direct = pair_dev(T, torch, a, b, q, n, io)
            da, db = _t(torch, a), _t(torch, b)
            dh = torch.empty((count, n), dtype=torch.int32, device=dev)
            T.rq.ntt_forward_cyclic_dev(da.data_ptr(), dh.data_ptr(), q, n, count, io_bits=io)
            do = torch.full((count, n), -1, dtype=da.dtype, device=dev)
            T.rq.poly_mul_hat_cyclic_dev(dh.data_ptr(), n, db.data_ptr(), do.data_ptr(), q, n, count, io_bits=io)     # one image per product
            torch.cuda.synchronize()
            assert (_out(do, io) == direct).all(), (q, n, io)
            do.fill_(-1)
            T.rq.poly_mul_hat_cyclic_dev(dh.data_ptr(), 0, db.data_ptr(), do.data_ptr(), q, n, count, io_bits=io)     # one image for all
            torch.cuda.synchronize()
            shared = M.poly_mul(np.broadcast_to(a[:1], a.shape), b, q)
            assert (_out(do, io) == shared).all(), (q, n, io)


def composed(T, torch, A, B, q, n, shared, io):
    """C[c][i][j] = sum_k cyclic pair products through psf_poly_mul_cyclic_dev, summed mod q on the host; A (count or 1, rows, inner, n) logical"""
    count, inner, cols = B.shape[0], B.shape[1], B.shape[2]
    rows = A.shape[1]
    Ab = np.broadcast_to(A, (count,) + A.shape[1:]) if shared else A
    pa = np.ascontiguousarray(np.broadcast_to(Ab[:, :, None, :, :], (count, rows, cols, inner, n))).reshape(-1, n)
    pb = np.ascontiguousarray(np.broadcast_to(np.transpose(B, (0, 2, 1, 3))[:, None], (count, rows, cols, inner, n))).reshape(-1, n)
    prod = pair_dev(T, torch, pa, pb, q, n, io).reshape(count, rows, cols, inner, n)
    acc = np.zeros((count, rows, cols, n), dtype=np.uint64)
    for k in range(inner):
        acc = (acc + prod[..., k, :]) % np.uint64(q)
    return acc


def mat_dev(T, torch, A_store, B, q, n, rows, inner, cols, trans, shared, io=64, hat=False):
    count = B.shape[0]
    dev = _dev(torch)
    da, db = _t(torch, A_store), _t(torch, B)
    dc = torch.full((count, rows, cols, n), -1, dtype=torch.int64 if io == 64 else torch.int16, device=dev)
    per = rows * inner
    if hat:
        dh = torch.empty((A_store.shape[0] * per, n), dtype=torch.int32, device=dev)
        T.rq.ntt_forward_cyclic_dev(da.data_ptr(), dh.data_ptr(), q, n, A_store.shape[0] * per, io_bits=io)
        T.rq.matpoly_mul_hat_cyclic_dev(dh.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols, hat_stride=0 if shared else per * n,
                                        trans_a=trans, io_bits=io)
    else:
        T.rq.matpoly_mul_cyclic_dev(da.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols, a_stride=0 if shared else per,
                                    trans_a=trans, io_bits=io)
    torch.cuda.synchronize()
    return _out(dc, io)


MAT_QN = [(3329, 256), (3329, 512), (12289, 1024), (7937, 512), (1153, 128), (2013265921, 256), (20353, 256), (17, 8), (3329, 1024), (1 << 30, 64),
          ((1 << 61) - 1, 32), ((1 << 62) - 57, 16)]


def test_matrix_products_every_form_against_the_model(T, torch):
    rng = np.random.default_rng(34)
    for q, n in MAT_QN:
        for rows, inner, cols in DIMS:
            for trans in (0, 1):
                for shared in (True, False):
                    for io in ((64, 16) if _route16(q, n) else (64,)):
                        count = 2
                        na = 1 if shared else count
                        if io == 16:
                            A = rng.integers(0, q, size=(na, rows, inner, n)).astype(np.uint16)
                            B = rng.integers(-q + 1, q, size=(count, inner, cols, n)).astype(np.int16)
                        else:
                            A = rng.integers(0, U64.max, size=(na, rows, inner, n), dtype=np.uint64, endpoint=True)
                            B = rng.integers(I64.min, I64.max, size=(count, inner, cols, n), dtype=np.int64, endpoint=True)
                        got = mat_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, shared, io)
                        assert (got == composed(T, torch, A, B, q, n, shared, io)).all(), (q, n, rows, inner, cols, trans, shared, io)
                        if n * n * inner <= (1 << 20):                 # the big-integer model on one sampled output
                            c, i, j = rng.integers(count), rng.integers(rows), rng.integers(cols)
                            assert (M.matpoly_entry(A[0 if shared else c], B[c], q, i, j) == got[c, i, j]).all(), (q, n, rows, inner, cols, c, i, j)
                        if (q, n) in WAVE:
                            goth = mat_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, shared, io, hat=True)
                            assert (goth == got).all(), (q, n, rows, inner, cols, trans, shared, io)
                        if io == 64 and trans == 0 and shared:
                            assert (T.rq.matpoly_mul_cyclic(A[0], B[0], q) == got[0]).all(), (q, n, rows, inner, cols)
        # the host form over a whole product against the model (small n: the model is exact Python integers)
        if n <= 64:
            A = rng.integers(0, q, size=(3, 5, n), dtype=np.uint64)
            B = rng.integers(-(1 << 40), 1 << 40, size=(5, 2, n), dtype=np.int64)
            assert (T.rq.matpoly_mul_cyclic(A, B, q) == M.matpoly_mul(A, B, q)).all(), (q, n)


@pytest.mark.parametrize("q,n,io", [(3329, 256, 64), (3329, 256, 16), (12289, 1024, 16), (2013265921, 256, 64), (1 << 30, 64, 64)])
def test_inner_past_the_fold_interval(T, torch, q, n, io):
    """a = q - 1 everywhere, b = +-(q - 1) by parity (and b = q - 1 everywhere), 4099 times: the fastest growth of the accumulators"""
    inner, rows, cols = 4099, 2, 1
    A = np.full((1, rows, inner, n), q - 1, dtype=np.uint16 if io == 16 else np.uint64)
    for sign in (np.where(np.arange(n) % 2 == 0, 1, -1), np.ones(n, dtype=np.int64)):
        B = np.ascontiguousarray(np.broadcast_to((q - 1) * sign, (1, inner, cols, n))).astype(np.int16 if io == 16 else np.int64)
        want = M.cyclic(np.full(n, q - 1, dtype=object), (inner * (q - 1) * sign).astype(object))
        want = np.array([int(v) % q for v in want], dtype=np.uint64)
        for trans in (0, 1):
            got = mat_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, True, io)
            assert (got == want).all(), (inner, trans)
            if (q, n) in WAVE:
                assert (mat_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, True, io, hat=True) == want).all(), (inner, trans)


def test_full_size_identities(T, torch):
    """65 536 products at n = 256, q = 3329 (16-bit words), without the Python model: c(1) = a(1) b(1), c(-1) = a(-1) b(-1), and
    cyclic + negacyclic = 2 (low half of the integer product a b) mod q on a sampled subset"""
    dev = _dev(torch)
    q, n, count = 3329, 256, 65536
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    da = torch.randint(0, q, (count, n), dtype=torch.int16, device=dev, generator=g)
    db = torch.randint(-q + 1, q, (count, n), dtype=torch.int16, device=dev, generator=g)
    dc, dn = torch.empty_like(da), torch.empty_like(da)
    T.rq.poly_mul_cyclic_dev(da.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, io_bits=16)
    T.gadget.poly_mul_negacyclic_dev(da.data_ptr(), db.data_ptr(), dn.data_ptr(), q, n, count, io_bits=16)
    torch.cuda.synchronize()
    a, b, c = da.to(torch.int64), db.to(torch.int64), dc.to(torch.int64)
    assert int(c.min()) >= 0 and int(c.max()) < q
    assert torch.equal(c.sum(1) % q, (a.sum(1) % q) * (b.sum(1) % q) % q)
    alt = torch.where(torch.arange(n, device=dev) % 2 == 0, 1, -1).to(torch.int64)
    assert torch.equal((c * alt).sum(1) % q, ((a * alt).sum(1) % q) * ((b * alt).sum(1) % q) % q)
    rng = np.random.default_rng(35)
    an, bn, cn, nn = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy(), dn.to(torch.int64).cpu().numpy()
    for r in rng.choice(count, size=64, replace=False):
        low = np.convolve(an[r], bn[r])[:n]
        assert ((cn[r] + nn[r]) % q == (2 * low) % q).all(), r


def _negacyclic(a, b, q):
    return np.array([[int(v) % q for v in MN.negacyclic(x.astype(object), y.astype(object))] for x, y in zip(a, b)], dtype=np.uint64)


def test_plans_of_both_rings_in_one_process(T, torch):
    """the plan cache is keyed by the ring: alternate cyclic and negacyclic calls on (q, n) that no other test uses, each against its own model"""
    rng = np.random.default_rng(36)
    dev = _dev(torch)
    for q, n in [(7681, 512), (7681, 64), (40961, 128)]:
        for step in range(4):
            cyc = step % 2 == 0
            a, b = _pair_operands(rng, q, n, 3, 64, 0)
            want = M.poly_mul(a, b, q) if cyc else _negacyclic(a, b, q)
            da, db = _t(torch, a), _t(torch, b)
            do = torch.full_like(da, -1)
            (T.rq.poly_mul_cyclic_dev if cyc else T.gadget.poly_mul_negacyclic_dev)(da.data_ptr(), db.data_ptr(), do.data_ptr(), q, n, 3)
            torch.cuda.synchronize()
            assert (_np(do, np.uint64) == want).all(), (q, n, step)
            if n >= 128:                                             # a wave shape: the image forms too
                dh = torch.empty((3, n), dtype=torch.int32, device=dev)
                (T.rq.ntt_forward_cyclic_dev if cyc else T.gadget.ntt_forward_dev)(da.data_ptr(), dh.data_ptr(), q, n, 3)
                do.fill_(-1)
                (T.rq.poly_mul_hat_cyclic_dev if cyc else T.gadget.poly_mul_hat_dev)(dh.data_ptr(), n, db.data_ptr(), do.data_ptr(), q, n, 3)
                torch.cuda.synchronize()
                assert (_np(do, np.uint64) == want).all(), (q, n, step, "hat")
            mm = (T.rq.matpoly_mul_cyclic if cyc else T.rq.matpoly_mul)(a.reshape(1, 3, n), b.reshape(3, 1, n), q)
            wsum = np.zeros(n, dtype=np.uint64)
            for k in range(3):
                wsum = (wsum + want[k]) % np.uint64(q)
            assert (mm[0, 0] == wsum).all(), (q, n, step, "matpoly")


def test_dev_forms_on_a_non_default_stream(T, torch):
    dev = _dev(torch)
    rng = np.random.default_rng(37)
    s = torch.cuda.Stream()
    for q, n, io in [(3329, 256, 16), (2013265921, 256, 64), (17, 8, 64), (1 << 30, 64, 64)]:
        count = 64
        a, b = _pair_operands(rng, q, n, count, io, 0)
        want = M.poly_mul(a, b, q)
        ha, hb = _t(torch, a), _t(torch, b)
        da, db, do = torch.zeros_like(ha), torch.zeros_like(hb), torch.zeros_like(ha)
        dc = torch.zeros((count, 1, 1, n), dtype=ha.dtype, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            big = torch.ones((1 << 24,), dtype=torch.float32, device=dev)
            for _ in range(4):
                big = big * 1.0001                                   # keeps the stream busy before the writes
            da.copy_(ha + (big[:1].to(ha.dtype) * 0))
            db.copy_(hb)
            T.rq.poly_mul_cyclic_dev(da.data_ptr(), db.data_ptr(), do.data_ptr(), q, n, count, io_bits=io, stream=s.cuda_stream)
            T.rq.matpoly_mul_cyclic_dev(da.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, 1, 1, 1, a_stride=1, io_bits=io, stream=s.cuda_stream)
        s.synchronize()
        assert (_out(do, io) == want).all(), (q, n, io)
        assert (_out(dc, io).reshape(count, n) == want).all(), (q, n, io)
        if (q, n) in WAVE:
            dh = torch.empty((count, n), dtype=torch.int32, device=dev)
            do2 = torch.zeros_like(ha)
            dc2 = torch.zeros((count, 1, 1, n), dtype=ha.dtype, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                T.rq.ntt_forward_cyclic_dev(da.data_ptr(), dh.data_ptr(), q, n, count, io_bits=io, stream=s.cuda_stream)
                T.rq.poly_mul_hat_cyclic_dev(dh.data_ptr(), n, db.data_ptr(), do2.data_ptr(), q, n, count, io_bits=io, stream=s.cuda_stream)
                T.rq.matpoly_mul_hat_cyclic_dev(dh.data_ptr(), db.data_ptr(), dc2.data_ptr(), q, n, count, 1, 1, 1, hat_stride=n, io_bits=io,
                                                stream=s.cuda_stream)
            s.synchronize()
            assert (_out(do2, io) == want).all(), (q, n, io)
            assert (_out(dc2, io).reshape(count, n) == want).all(), (q, n, io)


def test_unsupported_shapes_write_nothing(T, torch):
    from tools_amd._ffi import lib
    dev = _dev(torch)
    for q, n, io, hat in [(3329, 2048, 64, True), (1 << 30, 256, 16, False), (1 << 30, 256, 16, True), (17, 8, 16, False)]:
        da = torch.zeros((2 * 3, n), dtype=torch.int64, device=dev)
        db = torch.zeros((3, n), dtype=torch.int64, device=dev)
        dc = torch.full((2, n), 12345, dtype=torch.int64, device=dev)
        fn = lib().psf_matpoly_mul_hat_cyclic_dev if hat else lib().psf_matpoly_mul_cyclic_dev
        rc = fn(0, C.c_uint64(q), C.c_size_t(n), C.c_size_t(1), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1), C.c_void_p(da.data_ptr()), C.c_size_t(0), 0,
                C.c_void_p(db.data_ptr()), C.c_void_p(dc.data_ptr()), io, None)
        torch.cuda.synchronize()
        assert rc == 8, (q, n, io, hat)
        assert (dc == 12345).all(), (q, n, io, hat)
