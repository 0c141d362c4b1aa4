"""No-GPU checks of the R_q matrix product (psf_matpoly_mul_*, include/psf_mi355x.h): the big-integer model (tests/helpers/rq_model.py) against
the integer product of rot^- embeddings, the reference's is_trapdoor (gadget_ring.rs:190-202) and is_basis (short_basis_ring.rs:183-198)
identities through the model, and every argument error of the three entry points (checked before any HIP call).  The device results are compared
with the model in tests/test_gpu_matpoly.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import rq_model as M

OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _rot_blocks(X):
    """(r, c, n) polynomials -> the (r n) x (c n) integer matrix of rot^- blocks (rotation_matrix.rs:85-96 per polynomial)"""
    from tools_amd import gadget
    r, c, n = X.shape
    out = np.zeros((r * n, c * n), dtype=object)
    for i in range(r):
        for j in range(c):
            out[i * n:(i + 1) * n, j * n:(j + 1) * n] = gadget.rot_minus_matrix(X[i, j].astype(np.int64).reshape(n, 1)).astype(object)
    return out


def test_model_equals_the_product_of_rot_embeddings():
    rng = np.random.default_rng(3)
    for q, n, rows, inner, cols in [(17, 4, 2, 3, 2), (3329, 8, 3, 5, 2), ((1 << 61) - 1, 6, 2, 2, 3), (64, 5, 1, 4, 3), (2, 1, 1, 1, 1)]:
        A = rng.integers(0, q, size=(rows, inner, n), dtype=np.uint64)
        B = rng.integers(-(1 << 40), 1 << 40, size=(inner, cols, n), dtype=np.int64)
        want = M.matpoly_mul(A, B, q)
        # column j of C, as one long vector: rot(A) times the stacked coefficient vectors of column j of B
        RA = _rot_blocks(A)
        for j in range(cols):
            bj = np.concatenate([B[k, j].astype(object) for k in range(inner)])
            cj = RA.dot(bj)
            got = np.array([int(v) % q for v in cj], dtype=np.uint64).reshape(rows, n)
            assert (got == want[:, j]).all(), (q, n, j)
        for i in range(rows):
            for j in range(cols):
                assert (M.matpoly_entry(A, B, q, i, j) == want[i, j]).all()


def _ring_key(n, q, rng):
    """a = [1 | a_bar | g^t - (a_bar r + e)] (gadget_ring.rs:62-81) with the model's products, r and e small"""
    import tools_amd as T
    gp = T.GadgetParametersRing.init_default(n, q)
    k = gp.k
    a_bar = rng.integers(0, q, size=n, dtype=np.uint64)
    r = rng.integers(-3, 4, size=(k, n), dtype=np.int64)
    e = rng.integers(-3, 4, size=(k, n), dtype=np.int64)
    abr = M.matpoly_mul(a_bar.reshape(1, 1, n), r.reshape(1, k, n), q)[0]
    a = np.zeros((k + 2, n), dtype=np.uint64)
    a[0, 0] = 1 % q
    a[1] = a_bar
    for j in range(k):
        g = np.zeros(n, dtype=object)
        g[0] = pow(int(gp.base), j)
        a[2 + j] = [int(v) % q for v in g - abr[j].astype(object) - e[j].astype(object)]
    return gp, a, r, e


def _trapdoor(r, e):
    """[e; r; I_k] (compute_trapdoor, gadget_ring.rs:181-185): (k + 2) x k polynomials"""
    k, n = r.shape
    t = np.zeros((k + 2, k, n), dtype=np.int64)
    t[0], t[1] = e, r
    for j in range(k):
        t[2 + j, j, 0] = 1
    return t


def test_model_reproduces_is_trapdoor_and_is_basis():
    from tools_amd import gadget
    rng = np.random.default_rng(5)
    # is_trapdoor: n = 6, q = 32 (gadget_ring.rs:191); a . [e; r; I] = g^t
    gp, a, r, e = _ring_key(6, 32, rng)
    res = M.matpoly_mul(a.reshape(1, gp.k + 2, gp.n), _trapdoor(r, e), gp.q)
    assert res.shape == (1, gp.k, gp.n)
    for j in range(gp.k):
        want = np.zeros(gp.n, dtype=np.uint64)
        want[0] = pow(int(gp.base), j, gp.q)
        assert (res[0, j] == want).all(), j
    # is_basis: n = 5, 10, 12, q = 16 (short_basis_ring.rs:184-186); a . S = 0 for the short basis of the key
    for n in (5, 10, 12):
        gp, a, r, e = _ring_key(n, 16, rng)
        S = gadget.gen_short_basis_for_trapdoor_ring(gp, a, r, e)
        assert S.shape == (gp.k + 2, n * (gp.k + 2), n)
        res = M.matpoly_mul(a.reshape(1, gp.k + 2, n), S, gp.q)
        assert not res.any(), n
        # and a perturbed basis is not in the kernel
        S[0, 0, 0] += 1
        assert M.matpoly_mul(a.reshape(1, gp.k + 2, n), S[:, :1], gp.q).any()


def _calls(L):
    vp = C.c_void_p

    def dev(q=3329, n=256, count=1, rows=2, inner=3, cols=1, a=0x100000, a_stride=0, trans=0, b=0x200000, c=0x300000, io=64, device=0):
        return L.psf_matpoly_mul_negacyclic_dev(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols),
                                                vp(a), C.c_size_t(a_stride), C.c_int(trans), vp(b), vp(c), C.c_int(io), None)

    def hat(q=3329, n=256, count=1, rows=2, inner=3, cols=1, a=0x100000, a_stride=0, trans=0, b=0x200000, c=0x300000, io=64, device=0):
        return L.psf_matpoly_mul_hat_dev(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols),
                                         vp(a), C.c_size_t(a_stride), C.c_int(trans), vp(b), vp(c), C.c_int(io), None)
    return dev, hat


def test_argument_errors_through_the_abi():
    """every check returns before the first HIP call, so these codes hold on any host.  The pointers are never dereferenced: every call here fails a
    check, has count = 0, or names a device that does not exist."""
    L = _lib()
    for f in _calls(L):
        for kw in ({"a": 0}, {"b": 0}, {"c": 0}):
            assert f(**kw) == ERR_PARAM, kw                                     # NULL with count > 0
            assert f(count=0, **kw) == OK, kw                                   # count = 0: nothing to do
        for kw in ({"rows": 0}, {"inner": 0}, {"cols": 0}, {"trans": 2}, {"trans": -1}, {"io": 32}, {"io": 8}, {"io": 0}):
            assert f(**kw) == ERR_PARAM, kw
            assert f(count=0, **kw) == ERR_PARAM, kw                            # the shape is checked before count = 0
        for q in (0, 1, 1 << 62, (1 << 64) - 1):                                # the codes of the pair product
            want = L.psf_poly_mul_negacyclic_dev(0, C.c_uint64(q), C.c_size_t(256), C.c_size_t(1), C.c_void_p(0x100000), C.c_void_p(0x200000),
                                                 C.c_void_p(0x300000), 64, None)
            assert want == ERR_PARAM and f(q=q) == want, q
        for n in (0, 8193):
            assert f(n=n) == ERR_PARAM, n
        # byte counts that overflow size_t
        assert f(rows=1 << 40, inner=1 << 30) == ERR_PARAM
        assert f(cols=1 << 60) == ERR_PARAM
        assert f(count=1 << 60) == ERR_PARAM
        assert f(count=1 << 20, a_stride=1 << 50) == ERR_PARAM
        assert f(a=(1 << 64) - 1024) == ERR_PARAM                               # the range of A wraps the address space
        # the output overlaps an input: B = 3 x 1 x 256 int64 = 6144 bytes, C = 2 x 1 x 256 x 8 = 4096 bytes
        assert f(c=0x200000 + 6143) == ERR_PARAM
        assert f(c=0x200000 - 4095) == ERR_PARAM
        assert f(c=0x100000) == ERR_PARAM
        assert f(c=0x100000 - 4095) == ERR_PARAM
        assert f(count=0, c=0x100000) == OK
    dev, hat = _calls(L)
    # A of the plain form: 2 x 3 x 256 uint64 = 12 288 bytes; of the hat form: 2 x 3 x 256 words = 6144 bytes
    assert dev(c=0x100000 + 12287) == ERR_PARAM
    assert hat(c=0x100000 + 6143) == ERR_PARAM
    assert hat(c=0x100000 + 6144, b=0x800000, device=-1) == ERR_HIP              # adjacent, not overlapping: past the checks
    assert dev(count=2, a_stride=6, c=0x100000 + 12288 + 6 * 2048 - 1) == ERR_PARAM   # the second batch's A reaches that far
    # outside the kernels: nothing is launched
    assert hat(q=3329, n=2048) == ERR_UNSUPPORTED                               # no wave kernel for n = 2048
    assert hat(q=1 << 30) == ERR_UNSUPPORTED                                    # no NTT
    assert hat(q=2013265921, io=16) == ERR_UNSUPPORTED                          # 16-bit words: q < 2^14
    assert dev(q=1 << 30, io=16) == ERR_UNSUPPORTED
    assert dev(q=3329, n=2048, io=16) == ERR_UNSUPPORTED
    assert dev(q=17, n=8, io=16) == ERR_UNSUPPORTED
    assert dev(inner=(1 << 20) + 1, a=1 << 40, b=2 << 40, c=3 << 40) == ERR_UNSUPPORTED                         # past the documented exact range
    # the host form
    a, b, c = np.zeros(2 * 3 * 8, dtype=np.uint64), np.zeros(3 * 8, dtype=np.int64), np.zeros(2 * 8, dtype=np.uint64)
    pa, pb, pc = a.ctypes.data_as(C.POINTER(C.c_uint64)), b.ctypes.data_as(C.POINTER(C.c_int64)), c.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.psf_matpoly_mul_negacyclic(0, C.c_uint64(17), C.c_size_t(8), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1), None, pb, pc) == ERR_PARAM
    assert L.psf_matpoly_mul_negacyclic(0, C.c_uint64(17), C.c_size_t(8), C.c_size_t(0), C.c_size_t(3), C.c_size_t(1), pa, pb, pc) == ERR_PARAM
    assert L.psf_matpoly_mul_negacyclic(0, C.c_uint64(1), C.c_size_t(8), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1), pa, pb, pc) == ERR_PARAM
    assert L.psf_matpoly_mul_negacyclic(0, C.c_uint64(17), C.c_size_t(8), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1), pa, pb,
                                        a.ctypes.data_as(C.POINTER(C.c_uint64))) == ERR_PARAM                # C on top of A


def test_valid_call_without_a_device_is_a_hip_error():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 too on a host without a GPU)"""
    L = _lib()
    a, b, c = np.zeros(2 * 3 * 8, dtype=np.uint64), np.zeros(3 * 8, dtype=np.int64), np.zeros(2 * 8, dtype=np.uint64)
    devices = [-1, 4096] + ([] if _have_device() else [0])
    for dev in devices:
        for q in (17, 3329):
            assert L.psf_matpoly_mul_negacyclic(dev, C.c_uint64(q), C.c_size_t(8), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1),
                                                a.ctypes.data_as(C.POINTER(C.c_uint64)), b.ctypes.data_as(C.POINTER(C.c_int64)),
                                                c.ctypes.data_as(C.POINTER(C.c_uint64))) == ERR_HIP, (dev, q)
        for fn in (L.psf_matpoly_mul_negacyclic_dev, L.psf_matpoly_mul_hat_dev):
            assert fn(dev, C.c_uint64(3329), C.c_size_t(256), C.c_size_t(1), C.c_size_t(2), C.c_size_t(3), C.c_size_t(1), C.c_void_p(0x100000),
                      C.c_size_t(0), 0, C.c_void_p(0x200000), C.c_void_p(0x300000), 64, None) == ERR_HIP, dev
    if not _have_device():
        import tools_amd as T
        with pytest.raises(T.PsfError) as ei:
            T.rq.matpoly_mul(np.zeros((2, 3, 8), dtype=np.uint64), np.zeros((3, 1, 8), dtype=np.int64), 17)
        assert ei.value.status == ERR_HIP
