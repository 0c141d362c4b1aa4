"""No-GPU checks of the fused R_q matrix products C = E + sign * op(A) B (psf_matpoly_mul_add_*, include/psf_mi355x.h): every new symbol in the header,
the built libraries and the three mirrors; every argument error through the ABI (checked before any HIP call, so a valid call on a host without a
device is PSF_ERR_HIP and an invalid one its own code); the big-integer model (tests/helpers/rq_fma_model.py) against a direct O(n^2) evaluation.
The device results are compared with the model in tests/test_gpu_matpoly_add.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.helpers import rq_fma_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
DEV_SYMBOLS = ["psf_matpoly_mul_add_negacyclic_dev", "psf_matpoly_mul_add_hat_dev", "psf_matpoly_mul_add_cyclic_dev", "psf_matpoly_mul_add_hat_cyclic_dev"]
HOST_SYMBOLS = ["psf_matpoly_mul_add_negacyclic", "psf_matpoly_mul_add_cyclic"]
SYMBOLS = DEV_SYMBOLS + HOST_SYMBOLS


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_every_symbol_is_declared_exported_and_mirrored():
    from tools_amd import _ffi, rq
    header, hpp, rs, ffi_py = _read("include", "psf_mi355x.h"), _read("include", "psf_mi355x.hpp"), _read("shim", "src", "ffi.rs"), _read("tools_amd", "_ffi.py")
    libs = [_ffi.lib(), _ffi.open_library(_ffi.EXP_LIB_PATH)]
    for name in SYMBOLS:
        proto = re.search(r"psf_status\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        assert re.search(r"const\s+\w+\s*\*\s*(d_)?e\s*,\s*int\s+sign\s*,", proto.group(1)), name          # E and sign in front of the output
        for L in libs:
            assert hasattr(L, name), name                                                               # the release and the experiments build
        assert re.search(r"\b" + name + r"\b", hpp), name
        assert re.search(r"pub fn " + name + r"\(", rs), name
        assert '"' + name + '"' in ffi_py, name
    assert set(_ffi.MATPOLY_MUL_ADD_DEV) == set(DEV_SYMBOLS) and set(_ffi.MATPOLY_MUL_ADD_HOST) == set(HOST_SYMBOLS)
    for fn in ("matpoly_mul_add", "matpoly_mul_add_dev", "matpoly_mul_add_hat_dev", "matpoly_mul_add_cyclic", "matpoly_mul_add_cyclic_dev", "matpoly_mul_add_hat_cyclic_dev"):
        assert callable(getattr(rq, fn)), fn


def _call(L, name):
    """the device form `name` with the defaults of one valid call: A 2 x 3, B 3 x 1, E and C 2 x 1 polynomials of 256 words"""
    vp = C.c_void_p

    def f(q=3329, n=256, count=1, rows=2, inner=3, cols=1, a=0x100000, a_stride=0, trans=0, b=0x200000, e=0x400000, sign=1, c=0x300000, io=64, device=0):
        return getattr(L, name)(device, q, n, count, rows, inner, cols, vp(a), a_stride, trans, vp(b), vp(e), sign, vp(c), io, None)
    return f


@pytest.mark.parametrize("name", DEV_SYMBOLS)
def test_argument_errors_through_the_abi(name):
    """every check returns before the first HIP call, so these codes hold on any host.  The pointers are never dereferenced: every call here fails a
    check, has count = 0, or names a device that does not exist."""
    f = _call(_lib(), name)
    hat = "hat" in name
    assert f(device=-1) == ERR_HIP                                              # the defaults are a valid call
    for sign in (0, 2, -2, 3):
        assert f(sign=sign) == ERR_PARAM, sign
        assert f(sign=sign, count=0) == ERR_PARAM, sign                         # like the shape, the sign is checked before count = 0
    assert f(sign=-1, device=-1) == ERR_HIP
    for kw in ({"a": 0}, {"b": 0}, {"c": 0}, {"e": 0}):
        assert f(**kw) == ERR_PARAM, kw                                         # NULL with count > 0
        assert f(count=0, **kw) == OK, kw
    # C and E: 2 x 1 x 256 x 8 = 4096 bytes.  The same buffer is the in-place form; any other common byte is an error
    assert f(e=0x300000, device=-1) == ERR_HIP
    for off in (1, 8, 2048, 4095, -1, -8, -4095):
        assert f(e=0x300000 + off) == ERR_PARAM, off
    assert f(e=0x300000 + 4096, device=-1) == ERR_HIP and f(e=0x300000 - 4096, device=-1) == ERR_HIP      # adjacent
    assert f(io=16, e=0x300000 + 1023) == ERR_PARAM and f(io=16, e=0x300000 + 1024, device=-1) == ERR_HIP  # 1024 bytes at 16-bit words
    assert f(count=2, a_stride=6 * (256 if hat else 1), e=0x300000 + 8191) == ERR_PARAM                 # two batches: 8192 bytes
    assert f(e=(1 << 64) - 1024) == ERR_PARAM                                   # the range of E wraps the address space
    # E may lie on A or B (both are only read); C may not
    assert f(e=0x100000, device=-1) == ERR_HIP and f(e=0x200000, device=-1) == ERR_HIP
    assert f(c=0x200000 + 6143) == ERR_PARAM and f(c=0x200000 - 4095) == ERR_PARAM                       # C on B (3 x 1 x 256 int64 = 6144 bytes)
    assert f(c=0x200000, e=0x200000) == ERR_PARAM                               # in place, but on top of B
    assert f(c=0x100000) == ERR_PARAM and f(c=0x100000 - 4095) == ERR_PARAM                              # C on A
    # the inherited checks
    for kw in ({"rows": 0}, {"inner": 0}, {"cols": 0}, {"trans": 2}, {"trans": -1}, {"io": 32}, {"io": 8}, {"io": 0}):
        assert f(**kw) == ERR_PARAM, kw
        assert f(count=0, **kw) == ERR_PARAM, kw
    for q in (0, 1, 1 << 62, (1 << 64) - 1):
        assert f(q=q) == ERR_PARAM, q
    for n in (0, 8193):
        assert f(n=n) == ERR_PARAM, n
    assert f(rows=1 << 40, inner=1 << 30) == ERR_PARAM and f(cols=1 << 60) == ERR_PARAM and f(count=1 << 60) == ERR_PARAM
    assert f(count=1 << 20, a_stride=1 << 50) == ERR_PARAM
    assert f(a=(1 << 64) - 1024) == ERR_PARAM
    # outside the kernels: nothing is launched
    far = {"a": 1 << 40, "b": 2 << 40, "c": 3 << 40, "e": 4 << 40}
    assert f(inner=(1 << 20) + 1, **far) == ERR_UNSUPPORTED
    assert f(q=1 << 30, io=16) == ERR_UNSUPPORTED and f(q=3329, n=2048, io=16) == ERR_UNSUPPORTED and f(q=2013265921, io=16) == ERR_UNSUPPORTED
    if hat:
        assert f(q=3329, n=2048) == ERR_UNSUPPORTED and f(q=1 << 30) == ERR_UNSUPPORTED
    else:
        assert f(q=1 << 30, device=-1) == ERR_HIP and f(q=3329, n=2048, device=-1) == ERR_HIP            # the schoolbook route
    # PSF_ERR_PARAM outranks PSF_ERR_UNSUPPORTED: each malformed argument on a call that is unsupported by itself
    for bad in ({"sign": 0}, {"e": 0}, {"e": 0x300000 + 8}, {"c": 0x200000}, {"trans": 2}):
        assert f(q=1 << 30, io=16, **bad) == ERR_PARAM, bad
    for bad in ({"sign": 2}, {"e": 0}, {"e": (3 << 40) + 8}, {"c": 2 << 40}, {"rows": 0}):
        assert f(inner=(1 << 20) + 1, **{**far, **bad}) == ERR_PARAM, bad


@pytest.mark.parametrize("name", HOST_SYMBOLS)
def test_host_form_errors_and_no_device(name):
    L = _lib()
    fn = getattr(L, name)
    a, b, e, c = np.zeros(2 * 3 * 8, dtype=np.uint64), np.zeros(3 * 8, dtype=np.int64), np.zeros(2 * 8, dtype=np.int64), np.zeros(2 * 8, dtype=np.uint64)
    pa, pb, pe, pc = (x.ctypes.data_as(C.POINTER(t)) for x, t in ((a, C.c_uint64), (b, C.c_int64), (e, C.c_int64), (c, C.c_uint64)))
    assert fn(0, 17, 8, 2, 3, 1, pa, pb, None, 1, pc) == ERR_PARAM                                       # NULL E
    assert fn(0, 17, 8, 2, 3, 1, None, pb, pe, 1, pc) == ERR_PARAM
    assert fn(0, 17, 8, 2, 3, 1, pa, pb, pe, 0, pc) == ERR_PARAM and fn(0, 17, 8, 2, 3, 1, pa, pb, pe, 2, pc) == ERR_PARAM
    assert fn(0, 17, 8, 0, 3, 1, pa, pb, pe, 1, pc) == ERR_PARAM and fn(0, 1, 8, 2, 3, 1, pa, pb, pe, 1, pc) == ERR_PARAM
    assert fn(0, 17, 8, 2, 3, 1, pa, pb, pe, 1, a.ctypes.data_as(C.POINTER(C.c_uint64))) == ERR_PARAM    # C on top of A
    e_in_c = C.cast(C.c_void_p(c.ctypes.data + 8), C.POINTER(C.c_int64))
    assert fn(0, 17, 8, 2, 3, 1, pa, pb, e_in_c, 1, pc) == ERR_PARAM                                     # E partly on C
    in_place = C.cast(C.c_void_p(c.ctypes.data), C.POINTER(C.c_int64))
    for dev in (-1, 4096):
        for q in (17, 3329):
            for sign in (1, -1):
                assert fn(dev, q, 8, 2, 3, 1, pa, pb, pe, sign, pc) == ERR_HIP, (dev, q, sign)
        assert fn(dev, 17, 8, 2, 3, 1, pa, pb, in_place, 1, pc) == ERR_HIP                               # c == e is allowed
    import tools_amd as T
    with pytest.raises(T.PsfError) as ei:
        getattr(T.rq, name[4:].replace("_negacyclic", ""))(np.zeros((2, 3, 8), dtype=np.uint64), np.zeros((3, 1, 8), dtype=np.int64),
                                                           np.zeros((2, 1, 8), dtype=np.int64), 17, sign=-1, device=4096)
    assert ei.value.status == ERR_HIP


def _direct(A, B, E, q, sign, ring):
    """C[i][j][c] = E + sign * sum_k sum_t A[i][k][t] B[k][j][(c - t) mod n], the wrapped terms negated in the negacyclic ring: O(n^2) Python integers"""
    rows, inner, n = A.shape
    cols = B.shape[1]
    out = np.zeros((rows, cols, n), dtype=np.uint64)
    for i in range(rows):
        for j in range(cols):
            for c in range(n):
                acc = 0
                for k in range(inner):
                    for t in range(n):
                        term = int(A[i, k, t]) * int(B[k, j, (c - t) % n])
                        acc += -term if (t > c and ring == "negacyclic") else term
                out[i, j, c] = (int(E[i, j, c]) + sign * acc) % q
    return out


def test_model_equals_a_direct_evaluation():
    rng = np.random.default_rng(11)
    for q, n, rows, inner, cols in [(17, 4, 2, 3, 2), (3329, 8, 3, 2, 1), ((1 << 61) - 1, 6, 1, 2, 2), (64, 5, 2, 1, 3), (2, 1, 1, 1, 1)]:
        A = rng.integers(0, q, size=(rows, inner, n), dtype=np.uint64)
        B = rng.integers(-(1 << 40), 1 << 40, size=(inner, cols, n), dtype=np.int64)
        E = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=(rows, cols, n), dtype=np.int64, endpoint=True)
        for ring in ("negacyclic", "cyclic"):
            for sign in (1, -1):
                got = F.matpoly_mul_add(A, B, E, q, sign, ring)
                assert got.dtype == np.uint64 and (got < q).all()
                assert (got == _direct(A, B, E, q, sign, ring)).all(), (q, n, ring, sign)
    with pytest.raises(ValueError):
        F.matpoly_mul_add(A, B, E, q, 0)
