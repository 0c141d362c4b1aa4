"""R_q matrix products on the device (psf_matpoly_mul_negacyclic_dev / psf_matpoly_mul_hat_dev / psf_matpoly_mul_negacyclic; MatPolynomialRingZq *
MatPolynomialRingZq at gpv_ring.rs:245, gadget_ring.rs:78 and :190-202, short_basis_ring.rs:183-198): the wave kernel and the schoolbook kernel against
the composed route (pair products through psf_poly_mul_negacyclic_dev, summed mod q) and the big-integer model, in both I/O widths, for every shape
class; worst-case operands past the fold interval of the 16-bit accumulators; the reference's identities at full size; psfring_f_a_dev."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import rq_model as M

pytestmark = pytest.mark.gpu

OK, ERR_UNSUPPORTED = 0, 8
WAVE = [(3329, 128), (3329, 256), (3329, 512), (7681, 256), (12289, 512), (12289, 1024), (257, 128), (7937, 256), (7937, 512), (1153, 128), (1153, 256),
        (13313, 1024), (2013265921, 256), (1073479681, 512), (22273, 256), (20353, 256), (2013265921, 1024)]
GENERIC = [(17, 8), (5, 2), (257, 64), (3329, 1024), (12289, 2048), (13, 64), (2013265921, 32)]
OTHER = [(1 << 30, 64), ((1 << 61) - 1, 32), (64, 16), (17, 8)]            # no NTT: the schoolbook kernel
DIMS = [(1, 1, 1), (4, 4, 1), (3, 5, 2), (1, 14, 37)]


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


def _np(t, dtype):
    return t.cpu().numpy().view(dtype)


def _route16(q, n):
    return q < (1 << 14) and (q, n) in WAVE


def composed(T, torch, A, B, q, n, trans, shared, io_bits=64):
    """C[c][i][j] = sum_k pair products A[c][i][k] * B[c][k][j] through psf_poly_mul_negacyclic_dev, summed mod q on the host.
    A: (count or 1, rows, inner, n) in its logical layout (already transposed back), B: (count, inner, cols, n)."""
    count, inner, cols = B.shape[0], B.shape[1], B.shape[2]
    rows = A.shape[1]
    Ab = np.broadcast_to(A, (count,) + A.shape[1:]) if shared else A
    pa = np.ascontiguousarray(np.broadcast_to(Ab[:, :, None, :, :], (count, rows, cols, inner, n)))
    pb = np.ascontiguousarray(np.broadcast_to(np.transpose(B, (0, 2, 1, 3))[:, None], (count, rows, cols, inner, n)))
    P = count * rows * cols * inner
    da, db = _t(torch, pa.reshape(P, n)), _t(torch, pb.reshape(P, n))
    do = torch.empty((P, n), dtype=da.dtype, device=_dev(torch))
    T.gadget.poly_mul_negacyclic_dev(da.data_ptr(), db.data_ptr(), do.data_ptr(), q, n, P, io_bits=io_bits)
    torch.cuda.synchronize()
    prod = _np(do, np.uint64 if io_bits == 64 else np.uint16).astype(np.uint64).reshape(count, rows, cols, inner, n)
    acc = np.zeros((count, rows, cols, n), dtype=np.uint64)
    for k in range(inner):
        acc = (acc + prod[..., k, :]) % np.uint64(q)
    return acc


def run_dev(T, torch, A_store, B, q, n, rows, inner, cols, trans, shared, io_bits=64, hat=False):
    """C through psf_matpoly_mul_*_dev; A_store in storage order ((count or 1), rows x inner or inner x rows, n)"""
    count = B.shape[0]
    da, db = _t(torch, A_store), _t(torch, B)
    dc = torch.full((count, rows, cols, n), -1, dtype=torch.int64 if io_bits == 64 else torch.int16, device=_dev(torch))
    per = rows * inner
    if hat:
        dh = torch.empty((A_store.shape[0] * per, n), dtype=torch.int32, device=_dev(torch))
        T.gadget.ntt_forward_dev(da.data_ptr(), dh.data_ptr(), q, n, A_store.shape[0] * per, io_bits=io_bits)
        T.rq.matpoly_mul_hat_dev(dh.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols, hat_stride=0 if shared else per * n,
                                 trans_a=trans, io_bits=io_bits)
    else:
        T.rq.matpoly_mul_dev(da.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, count, rows, inner, cols, a_stride=0 if shared else per,
                             trans_a=trans, io_bits=io_bits)
    torch.cuda.synchronize()
    return _np(dc, np.uint64 if io_bits == 64 else np.uint16).astype(np.uint64)


def _operands(rng, q, n, count, rows, inner, cols, shared, io_bits, wide):
    na = 1 if shared else count
    if io_bits == 16:
        A = rng.integers(0, q, size=(na, rows, inner, n)).astype(np.uint16)
        B = rng.integers(-q + 1, q, size=(count, inner, cols, n)).astype(np.int16)
    elif wide:                                               # the 64-bit contract: any uint64 / int64
        A = rng.integers(0, np.iinfo(np.uint64).max, size=(na, rows, inner, n), dtype=np.uint64, endpoint=True)
        B = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=(count, inner, cols, n), dtype=np.int64, endpoint=True)
    else:
        A = rng.integers(0, q, size=(na, rows, inner, n), dtype=np.uint64)
        B = rng.integers(-q + 1, q, size=(count, inner, cols, n), dtype=np.int64)
    return A, B


def _store(A, trans):
    return np.ascontiguousarray(np.transpose(A, (0, 2, 1, 3))) if trans else A


def test_every_shape_against_the_composed_route_and_the_model(T, torch):
    rng = np.random.default_rng(21)
    case = 0
    for q, n in WAVE + GENERIC + OTHER:
        for rows, inner, cols in DIMS:
            trans, shared, count = case % 2, (case // 2) % 2, 1 + case % 7
            ios = (64, 16) if _route16(q, n) else (64,)
            for io in ios:
                if n * n * inner * count * rows * cols > (1 << 31):
                    count = 1
                A, B = _operands(rng, q, n, count, rows, inner, cols, shared, io, wide=case % 3 == 0)
                got = run_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, shared, io)
                want = composed(T, torch, A, B, q, n, trans, shared, io)
                assert (got == want).all(), (q, n, rows, inner, cols, trans, shared, count, io)
                if n * n * inner <= (1 << 20):                     # the big-integer model on one sampled output
                    c, i, j = rng.integers(count), rng.integers(rows), rng.integers(cols)
                    Ac = A[0 if shared else c]
                    assert (M.matpoly_entry(Ac, B[c], q, i, j) == got[c, i, j]).all(), (q, n, rows, inner, cols, c, i, j)
            case += 1
    A, B = _operands(rng, 3329, 128, 1, 1, 1, 1, 0, 64, wide=False)        # the host-pointer form at a single product of n = 128
    assert (T.rq.matpoly_mul(A[0], B[0], 3329)[0, 0] == M.matpoly_entry(A[0], B[0], 3329, 0, 0)).all()


@pytest.mark.parametrize("q,n,io", [(3329, 256, 64), (3329, 256, 16), (12289, 1024, 64), (12289, 1024, 16), (2013265921, 256, 64)])
def test_worst_case_operands_past_the_fold_interval(T, torch, q, n, io):
    """a = q - 1 everywhere, b = +-(q - 1) by coefficient parity: every summand's leaf products are the same, at the largest magnitudes"""
    for inner in (1024, 4099):
        rows, cols = 2, 1
        A = np.full((1, rows, inner, n), q - 1, dtype=np.uint16 if io == 16 else np.uint64)
        sign = np.where(np.arange(n) % 2 == 0, 1, -1)
        B = np.broadcast_to((q - 1) * sign, (1, inner, cols, n)).astype(np.int16 if io == 16 else np.int64)
        want = M.negacyclic(np.full(n, q - 1, dtype=object), (inner * (q - 1) * sign).astype(object))
        want = np.array([int(v) % q for v in want], dtype=np.uint64)
        for trans in (0, 1):
            got = run_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, True, io)
            assert (got == want).all(), (inner, trans)
            if (q, n) in WAVE:
                goth = run_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, True, io, hat=True)
                assert (goth == want).all(), (inner, trans)


def test_hat_form_equals_the_plain_form(T, torch):
    rng = np.random.default_rng(8)
    for q, n in WAVE:
        for rows, inner, cols in [(3, 5, 2), (4, 4, 1), (1, 14, 3)]:
            for trans in (0, 1):
                for shared in (True, False):
                    count = 3
                    for io in ((64, 16) if _route16(q, n) else (64,)):
                        A, B = _operands(rng, q, n, count, rows, inner, cols, shared, io, wide=False)
                        plain = run_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, shared, io)
                        hat = run_dev(T, torch, _store(A, trans), B, q, n, rows, inner, cols, trans, shared, io, hat=True)
                        assert (plain == hat).all(), (q, n, rows, inner, cols, trans, shared, io)


def test_hat_form_large_shared_a_in_global_memory(T, torch):
    """a shared A whose images do not fit in LDS (14 x 14 images of 1024 words) is read from global memory"""
    rng = np.random.default_rng(9)
    q, n, rows, inner, cols, count = 12289, 1024, 14, 14, 1, 2
    A, B = _operands(rng, q, n, count, rows, inner, cols, True, 64, wide=False)
    plain = run_dev(T, torch, A, B, q, n, rows, inner, cols, 0, True)
    hat = run_dev(T, torch, A, B, q, n, rows, inner, cols, 0, True, hat=True)
    assert (plain == hat).all()
    assert (plain == composed(T, torch, A, B, q, n, 0, True)).all()


def _trapdoor(r, e):
    k, n = r.shape
    t = np.zeros((k + 2, k, n), dtype=np.int64)
    t[0], t[1] = e, r
    for j in range(k):
        t[2 + j, j, 0] = 1
    return t


def _check_identities(T, gp, a, r, e, basis_cols=None):
    n, k, q = gp.n, gp.k, gp.q
    res = T.rq.matpoly_mul(a.reshape(1, k + 2, n), _trapdoor(r, e), q)              # is_trapdoor: a [e; r; I] = g^t
    for j in range(k):
        want = np.zeros(n, dtype=np.uint64)
        want[0] = pow(int(gp.base), j, q)
        assert (res[0, j] == want).all(), (n, q, j)
    S = T.gadget.gen_short_basis_for_trapdoor_ring(gp, a, r, e)                     # is_basis: a S = 0
    if basis_cols is not None:
        S = np.ascontiguousarray(S[:, :basis_cols])
    assert not T.rq.matpoly_mul(a.reshape(1, k + 2, n), S, q).any(), (n, q)


def test_reference_identities(T):
    rng = np.random.default_rng(4)
    # C4 (n = 256, q = 3329): the wave kernel; the full short basis, (k + 2) x 256 (k + 2) polynomials
    gp = T.GadgetParametersRing.init_default(256, 3329)
    a_bar = rng.integers(0, 3329, size=256, dtype=np.uint64)
    a, r, e = T.gadget.gen_trapdoor_ring_lwe(gp, a_bar, 2.0, seed=7)
    _check_identities(T, gp, a, r, e)
    # the reference's own cases: is_trapdoor n = 6, q = 32 and is_basis n = 5, 10, 12, q = 16 (the schoolbook kernel)
    for n, q in [(6, 32), (5, 16), (10, 16), (12, 16)]:
        gp = T.GadgetParametersRing.init_default(n, q)
        a_bar = rng.integers(0, q, size=n, dtype=np.uint64)
        a, r, e = T.gadget.gen_trapdoor_ring_lwe(gp, a_bar, 5.0, seed=n)
        _check_identities(T, gp, a, r, e)


def test_ring_f_a_dev_equals_the_matrix_product(T, torch):
    """psfring_f_a_dev (u_b = a sigma_b, gpv_ring.rs:243-247) = the product with one shared 1 x (k + 2) A over count = B batches"""
    from tools_amd._ffi import lib
    gp = T.GadgetParametersRing.init_default(256, 3329)
    ring = T.PSFGPVRing(gp, 600.0, 1.005)
    a, _ = ring.trap_gen(seed=3)
    K, n, Bn = gp.k + 2, gp.n, 257
    rng = np.random.default_rng(2)
    sigma = rng.integers(-40, 41, size=(Bn, K, 1, n), dtype=np.int64)
    ds = _t(torch, sigma)
    du = torch.zeros((Bn, n), dtype=torch.int64, device=_dev(torch))
    dok = torch.zeros(Bn, dtype=torch.uint8, device=_dev(torch))
    assert lib().psfring_f_a_dev(ring._h, C.c_size_t(Bn), C.c_void_p(ds.data_ptr()), C.c_void_p(du.data_ptr()), C.c_void_p(dok.data_ptr()), None) == OK
    torch.cuda.synchronize()
    got = run_dev(T, torch, np.asarray(a, dtype=np.uint64).reshape(1, 1, K, n), sigma, 3329, n, 1, K, 1, 0, True)
    assert (got.reshape(Bn, n) == _np(du, np.uint64)).all()


def test_unsupported_shapes_write_nothing(T, torch):
    from tools_amd._ffi import lib
    dev = _dev(torch)
    for q, n, io, hat in [(3329, 2048, 64, True), (1 << 30, 256, 16, False), (1 << 30, 256, 16, True), (17, 8, 16, False)]:
        da = torch.zeros((2 * 3, n), dtype=torch.int64, device=dev)
        db = torch.zeros((3, n), dtype=torch.int64, device=dev)
        dc = torch.full((2, n), 12345, dtype=torch.int64, device=dev)
        fn = lib().psf_matpoly_mul_hat_dev if hat else lib().psf_matpoly_mul_negacyclic_dev
        rc = fn(0, C.c_uint64(q), C.c_size_t(n), C.c_size_t(1), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1), C.c_void_p(da.data_ptr()), C.c_size_t(0), 0,
                C.c_void_p(db.data_ptr()), C.c_void_p(dc.data_ptr()), io, None)
        torch.cuda.synchronize()
        assert rc == ERR_UNSUPPORTED, (q, n, io, hat)
        assert (dc == 12345).all(), (q, n, io, hat)


def test_stream_order_and_large_counts(T, torch):
    dev = _dev(torch)
    q, n = 3329, 256
    # ordering: on a non-default stream, behind a kernel that writes the inputs
    rng = np.random.default_rng(5)
    A, B = _operands(rng, q, n, 64, 3, 4, 2, False, 64, wide=False)
    want = composed(T, torch, A, B, q, n, 0, False)
    s = torch.cuda.Stream()
    da, db = torch.zeros(A.shape, dtype=torch.int64, device=dev), torch.zeros(B.shape, dtype=torch.int64, device=dev)
    dc = torch.zeros((64, 3, 2, n), dtype=torch.int64, device=dev)
    ha, hb = _t(torch, A), _t(torch, B)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big = torch.ones((1 << 26,), dtype=torch.float32, device=dev)
        for _ in range(4):
            big = big * 1.0001                                       # keeps the stream busy before the writes
        da.copy_(ha * 1 + (big[:1].to(torch.int64) * 0))
        db.copy_(hb * 1)
        T.rq.matpoly_mul_dev(da.data_ptr(), db.data_ptr(), dc.data_ptr(), q, n, 64, 3, 4, 2, a_stride=12, io_bits=64, stream=s.cuda_stream)
    s.synchronize()
    assert (_np(dc, np.uint64) == want).all()
    # 65 536 batches of 4 x 4 . 4 x 1 (16-bit words, A per batch) against the composed route, on the device
    count, rows, inner, cols = 65536, 4, 4, 1
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    dA = torch.randint(0, q, (count, rows, inner, n), dtype=torch.int16, device=dev, generator=g)
    dB = torch.randint(-q + 1, q, (count, inner, cols, n), dtype=torch.int16, device=dev, generator=g)
    dC = torch.empty((count, rows, cols, n), dtype=torch.int16, device=dev)
    T.rq.matpoly_mul_dev(dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), q, n, count, rows, inner, cols, a_stride=rows * inner, io_bits=16)
    pb = dB[:, None, :, 0, :].expand(count, rows, inner, n).contiguous()
    dP = torch.empty((count * rows * inner, n), dtype=torch.int16, device=dev)
    T.gadget.poly_mul_negacyclic_dev(dA.data_ptr(), pb.data_ptr(), dP.data_ptr(), q, n, count * rows * inner, io_bits=16)
    want = dP.view(count, rows, inner, n).to(torch.int64).sum(2) % q
    torch.cuda.synchronize()
    assert torch.equal(dC.view(count, rows, n).to(torch.int64), want)
