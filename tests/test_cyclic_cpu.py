"""No-GPU checks of the products of the cyclic ring Z_q[X]/(X^n - 1) (psf_*_cyclic*, include/psf_mi355x.h): the big-integer model
(tests/helpers/rq_cyclic_model.py) against the integer product of circulant embeddings; every argument error of the eight entry points returns the code
of its X^n + 1 twin, before any HIP call; a valid call without a device is PSF_ERR_HIP; the Python wrappers reject bad shapes.  The device results are
compared with the model in tests/test_gpu_cyclic.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import rq_cyclic_model as M

OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
VP = C.c_void_p


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _circulant(X):
    """(r, c, n) polynomials -> the (r n) x (c n) integer matrix of circulant blocks: block (i, k)[s][t] = X[i][k][(s - t) mod n]"""
    r, c, n = X.shape
    out = np.zeros((r * n, c * n), dtype=object)
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
    for i in range(r):
        for k in range(c):
            out[i * n:(i + 1) * n, k * n:(k + 1) * n] = X[i, k].astype(object)[idx]
    return out


def test_model_equals_the_product_of_circulant_embeddings():
    rng = np.random.default_rng(13)
    for q, n, rows, inner, cols in [(17, 4, 2, 3, 2), (3329, 8, 3, 5, 2), ((1 << 61) - 1, 6, 2, 2, 3), (64, 5, 1, 4, 3), (2, 1, 1, 1, 1), (3329, 16, 1, 1, 1)]:
        A = rng.integers(0, q, size=(rows, inner, n), dtype=np.uint64)
        B = rng.integers(-(1 << 40), 1 << 40, size=(inner, cols, n), dtype=np.int64)
        want = M.matpoly_mul(A, B, q)
        RA = _circulant(A)
        for j in range(cols):
            bj = np.concatenate([B[k, j].astype(object) for k in range(inner)])
            got = np.array([int(v) % q for v in RA.dot(bj)], dtype=np.uint64).reshape(rows, n)
            assert (got == want[:, j]).all(), (q, n, j)
        # the pair product is the 1 x 1 case
        assert (M.poly_mul(A[0, 0], B[0, 0], q) == M.matpoly_mul(A[:1, :1], B[:1, :1], q)[0, 0]).all()
    # X^n = 1: multiplying by X rotates the coefficients up, the top one wraps to the constant term with a plus sign
    a = np.arange(1, 9, dtype=np.int64)
    x = np.zeros(8, dtype=np.int64)
    x[1] = 1
    assert list(M.cyclic(a, x)) == [8, 1, 2, 3, 4, 5, 6, 7]


# ---- the entry points and their X^n + 1 twins ---------------------------------------------------------------------------------------------------------
def _pairs(L):
    """(name, negacyclic call, cyclic call) with one keyword interface each; pointers are fake and never dereferenced: every call below either fails a
    check or names device -1 / 4096, which no HIP call accepts"""
    def poly_dev(f):
        def call(q=3329, n=256, count=1, a=0x100000, b=0x200000, o=0x300000, io=64, device=-1, **_):
            return f(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), VP(a), VP(b), VP(o), C.c_int(io), None)
        return call

    def fwd(f):
        def call(q=3329, n=256, count=1, a=0x100000, o=0x300000, io=64, device=-1, **_):
            return f(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), VP(a), C.c_int(io), VP(o), None)
        return call

    def hat(f):
        def call(q=3329, n=256, count=1, a=0x100000, a_stride=0, b=0x200000, o=0x300000, io=64, device=-1, **_):
            return f(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), VP(a), C.c_size_t(a_stride), VP(b), VP(o), C.c_int(io), None)
        return call

    def mat(f):
        def call(q=3329, n=256, count=1, rows=2, inner=3, cols=1, a=0x100000, a_stride=0, trans=0, b=0x200000, o=0x300000, io=64, device=-1, **_):
            return f(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols), VP(a),
                     C.c_size_t(a_stride), C.c_int(trans), VP(b), VP(o), C.c_int(io), None)
        return call

    # host buffers shared by both twins, so that the range and overlap checks see the same addresses (the pointers keep the arrays alive)
    HA, HB, HO = np.zeros(1 << 17, dtype=np.uint64), np.zeros(1 << 17, dtype=np.int64), np.zeros(1 << 17, dtype=np.uint64)
    pa, pb, po = HA.ctypes.data_as(C.POINTER(C.c_uint64)), HB.ctypes.data_as(C.POINTER(C.c_int64)), HO.ctypes.data_as(C.POINTER(C.c_uint64))

    def host_poly(f, method=None):
        def call(q=17, n=8, count=2, a=1, b=1, o=1, device=-1, method_=method, **_):
            args = [device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(count), pa if a else None, pb if b else None, po if o else None]
            if method_ is not None:
                args.append(C.c_int(method_))
            return f(*args)
        return call

    def host_mat(f):
        def call(q=17, n=8, rows=2, inner=3, cols=1, a=1, b=1, o=1, device=-1, overlap=False, **_):
            return f(device, C.c_uint64(q), C.c_size_t(n), C.c_size_t(rows), C.c_size_t(inner), C.c_size_t(cols), pa if a else None, pb if b else None,
                     (pa if overlap else po) if o else None)
        return call

    return [
        ("poly_mul", host_poly(L.psf_poly_mul_negacyclic), host_poly(L.psf_poly_mul_cyclic)),
        ("poly_mul_method0", host_poly(L.psf_poly_mul_negacyclic_method, 0), host_poly(L.psf_poly_mul_cyclic_method, 0)),
        ("poly_mul_method1", host_poly(L.psf_poly_mul_negacyclic_method, 1), host_poly(L.psf_poly_mul_cyclic_method, 1)),
        ("poly_mul_dev", poly_dev(L.psf_poly_mul_negacyclic_dev), poly_dev(L.psf_poly_mul_cyclic_dev)),
        ("ntt_forward_dev", fwd(L.psf_ntt_forward_dev), fwd(L.psf_ntt_forward_cyclic_dev)),
        ("poly_mul_hat_dev", hat(L.psf_poly_mul_hat_dev), hat(L.psf_poly_mul_hat_cyclic_dev)),
        ("matpoly_mul_dev", mat(L.psf_matpoly_mul_negacyclic_dev), mat(L.psf_matpoly_mul_cyclic_dev)),
        ("matpoly_mul_hat_dev", mat(L.psf_matpoly_mul_hat_dev), mat(L.psf_matpoly_mul_hat_cyclic_dev)),
        ("matpoly_mul", host_mat(L.psf_matpoly_mul_negacyclic), host_mat(L.psf_matpoly_mul_cyclic)),
    ]


CASES = [{}, {"count": 0}, {"a": 0}, {"b": 0}, {"o": 0}, {"a": 0, "count": 0}, {"q": 0}, {"q": 1}, {"q": 1 << 62}, {"q": (1 << 64) - 1}, {"n": 0},
         {"n": 8193}, {"n": 2048}, {"n": 255}, {"q": 1 << 30}, {"q": 17, "n": 8}, {"q": 2013265921}, {"q": (1 << 61) - 1}, {"q": 64, "n": 16},
         {"io": 16}, {"io": 32}, {"io": 0}, {"io": 16, "q": 1 << 30}, {"io": 16, "q": 2013265921}, {"io": 16, "n": 2048}, {"io": 16, "q": 17, "n": 8},
         {"rows": 0}, {"inner": 0}, {"cols": 0}, {"trans": 2}, {"trans": -1}, {"rows": 0, "count": 0}, {"rows": 1 << 40, "inner": 1 << 30},
         {"cols": 1 << 60}, {"count": 1 << 60}, {"count": 1 << 20, "a_stride": 1 << 50}, {"a": (1 << 64) - 1024}, {"o": 0x200000 + 6143},
         {"o": 0x100000}, {"o": 0x100000, "count": 0}, {"o": 0x100000 + 6144, "b": 0x800000}, {"inner": (1 << 20) + 1, "a": 1 << 40, "b": 2 << 40, "o": 3 << 40},
         {"device": 4096}, {"overlap": True}, {"q": 3329, "n": 256}, {"q": 12289, "n": 1024}]


def test_every_argument_error_has_the_code_of_the_negacyclic_twin():
    """every check returns before the first HIP call; calls that pass the checks meet device -1 / 4096 and return PSF_ERR_HIP in both rings"""
    L = _lib()
    seen = set()
    for name, neg, cyc in _pairs(L):
        for kw in CASES:
            want, got = neg(**kw), cyc(**kw)
            assert got == want, (name, kw, want, got)
            seen.add(got)
    assert {OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED} <= seen, seen


def test_argument_errors_are_the_documented_codes():
    L = _lib()
    p = {name: cyc for name, _, cyc in _pairs(L)}
    assert p["poly_mul_dev"](a=0) == ERR_PARAM and p["poly_mul_dev"](a=0, count=0) == OK
    assert p["poly_mul_dev"](io=32) == ERR_PARAM and p["poly_mul_dev"](n=8193) == ERR_PARAM and p["poly_mul_dev"](q=1) == ERR_PARAM
    assert p["matpoly_mul_dev"](a=0) == ERR_PARAM and p["matpoly_mul_dev"](a=0, count=0) == OK
    assert p["matpoly_mul_dev"](o=0x100000) == ERR_PARAM                                             # C on top of A
    assert p["matpoly_mul_hat_dev"](q=1 << 30) == ERR_UNSUPPORTED                                    # no NTT: no image form
    assert p["matpoly_mul_hat_dev"](q=3329, n=2048) == ERR_UNSUPPORTED                               # no wave kernel
    assert p["matpoly_mul_dev"](q=1 << 30, io=16) == ERR_UNSUPPORTED
    assert p["ntt_forward_dev"](q=1 << 30) == ERR_UNSUPPORTED and p["poly_mul_hat_dev"](q=17, n=8) == ERR_UNSUPPORTED
    assert p["poly_mul_method1"](q=1 << 30) == ERR_UNSUPPORTED and p["poly_mul_method1"](q=17, n=6) == ERR_UNSUPPORTED
    assert p["poly_mul"](q=1 << 30, a=0) == ERR_PARAM
    assert p["matpoly_mul"](overlap=True) == ERR_PARAM and p["matpoly_mul"](rows=0) == ERR_PARAM


def test_valid_call_without_a_device_is_a_hip_error():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 too on a host without a GPU)"""
    L = _lib()
    p = {name: cyc for name, _, cyc in _pairs(L)}
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        for q, n in [(17, 8), (3329, 256), (1 << 30, 64), (2013265921, 256)]:
            assert p["poly_mul"](q=q, n=8, device=dev) == ERR_HIP, (dev, q)
            assert p["matpoly_mul"](q=q, n=8, device=dev) == ERR_HIP, (dev, q)
            assert p["poly_mul_dev"](q=q, n=n, device=dev) == ERR_HIP, (dev, q, n)
            assert p["matpoly_mul_dev"](q=q, n=n, device=dev) == ERR_HIP, (dev, q, n)
        for name in ("ntt_forward_dev", "poly_mul_hat_dev", "matpoly_mul_hat_dev"):
            assert p[name](device=dev) == ERR_HIP, (dev, name)
    if not _have_device():
        import tools_amd as T
        with pytest.raises(T.PsfError) as ei:
            T.rq.matpoly_mul_cyclic(np.zeros((2, 3, 8), dtype=np.uint64), np.zeros((3, 1, 8), dtype=np.int64), 17)
        assert ei.value.status == ERR_HIP
        with pytest.raises(T.PsfError) as ei:
            T.rq.poly_mul_cyclic(np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.int64), 17)
        assert ei.value.status == ERR_HIP


def test_python_wrappers_reject_bad_shapes():
    import tools_amd as T
    for A, B in [((2, 3, 8), (2, 1, 8)), ((2, 3, 8), (3, 1, 4)), ((3, 8), (3, 1, 8)), ((2, 3, 8), (3, 8))]:
        with pytest.raises(ValueError):
            T.rq.matpoly_mul_cyclic(np.zeros(A, dtype=np.uint64), np.zeros(B, dtype=np.int64), 17)
    for a, b in [((2, 8), (2, 4)), ((2, 8), (3, 8)), ((8,), (2, 8)), ((2, 2, 8), (2, 2, 8)), ((2, 0), (2, 0))]:
        with pytest.raises(ValueError):
            T.rq.poly_mul_cyclic(np.zeros(a, dtype=np.uint64), np.zeros(b, dtype=np.int64), 17)
