"""No-GPU checks of the signing entry points of the SHA-2 sets of SLH-DSA in include/psf_mi355x.h (psf_slhdsa_sha2_sign_workspace_bytes,
psf_slhdsa_sha2_sign_dev, psf_slhdsa_sha2_sign): the symbols exported and mirrored, the workspace size equal to the SHAKE twin's, every argument error
in its stated order (all checked before the first HIP call, so the codes hold on any host) with the guard buffer unchanged, count = 0, and a valid call
without a device PSF_ERR_HIP.  The device results are compared with the model in tests/test_gpu_slhdsa_sha2_sign.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
SMAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
SYMBOLS = ("psf_slhdsa_sha2_sign_workspace_bytes", "psf_slhdsa_sha2_sign_dev", "psf_slhdsa_sha2_sign")
# param: (n, d, h', a, k, sig)
SETS = {0: (16, 7, 9, 12, 14, 7856), 1: (16, 22, 3, 6, 33, 17088), 2: (24, 7, 9, 14, 17, 16224), 3: (24, 22, 3, 8, 33, 35664), 4: (32, 8, 8, 14, 22, 29792),
        5: (32, 17, 4, 9, 35, 49856)}
NAMES = ["SLH-DSA-SHA2-128s", "SLH-DSA-SHA2-128f", "SLH-DSA-SHA2-192s", "SLH-DSA-SHA2-192f", "SLH-DSA-SHA2-256s", "SLH-DSA-SHA2-256f"]
TWINS = [n.replace("SHA2", "SHAKE") for n in NAMES]


def _lib():
    from tools_amd import slhdsa, slhdsa_sha2
    slhdsa._lib()
    return slhdsa_sha2._lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _ws(L, param, count):
    out = C.c_size_t(0)
    assert L.psf_slhdsa_sha2_sign_workspace_bytes(param, count, C.byref(out)) == OK
    return out.value


def test_every_symbol_is_exported_and_mirrored():
    L = _lib()
    for fn in SYMBOLS:
        assert hasattr(L, fn), fn
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"])
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "psf_mi355x.hpp")).read()
    for fn in SYMBOLS:
        assert f"pub fn {fn}(" in ffi, fn
        assert fn + "(" in hpp, fn
    for fn in ("slhdsa_sha2_sign_workspace_bytes(", "slhdsa_sha2_sign_dev(", "std::vector<uint8_t> slhdsa_sha2_sign("):
        assert "inline " in hpp and fn in hpp, fn
    import tools_amd as T
    for name in ("sign_workspace_bytes", "sign_dev", "sign_internal", "sign"):
        assert callable(getattr(T.slhdsa_sha2, name)), name
    assert "are not here" not in T.slhdsa_sha2.__doc__ and "HashSLH-DSA is not here" in T.slhdsa_sha2.__doc__


def test_workspace_bytes_equal_the_shake_twin():
    L = _lib()
    out = C.c_size_t(99)
    for param in (-1, 6, 45):
        assert L.psf_slhdsa_sha2_sign_workspace_bytes(param, 1, C.byref(out)) == ERR_PARAM
        assert L.psf_slhdsa_sha2_sign_workspace_bytes(param, 0, None) == ERR_PARAM
    assert L.psf_slhdsa_sha2_sign_workspace_bytes(1, 1, None) == ERR_PARAM
    assert L.psf_slhdsa_sha2_sign_workspace_bytes(1, SMAX // 1024, C.byref(out)) == ERR_PARAM      # does not fit size_t
    assert out.value == 99
    import tools_amd as T
    for param in SETS:
        for count in (0, 1, 3, 67, 1 << 20):
            twin = C.c_size_t(0)
            assert L.psf_slhdsa_sign_workspace_bytes(param, count, C.byref(twin)) == OK
            assert _ws(L, param, count) == twin.value and twin.value % 256 == 0, (param, count)
            assert T.slhdsa_sha2.sign_workspace_bytes(NAMES[param], count) == T.slhdsa.sign_workspace_bytes(TWINS[param], count)
        assert _ws(L, param, 0) == 0 and _ws(L, param, 1) > 0
    assert _ws(L, 2, (1 << 31) - 1) > 1 << 52                              # no 32-bit or 48-bit product on the way


def _sign_dev(L, param, sk_len, msg_len=33, sk_stride=None, msg_stride=None):
    ss = sk_len if sk_stride is None else sk_stride
    ms = msg_len if msg_stride is None else msg_stride
    return lambda c, sk, msg, rnd, sig, w, wb: L.psf_slhdsa_sha2_sign_dev(0, param, c, sk, ss, msg, msg_len, ms, rnd, sig, w, wb, None)


def _sign_host(L, param, sk_len, msg_len=33):
    return lambda c, sk, msg, rnd, sig, w=None, wb=0: L.psf_slhdsa_sha2_sign(0, param, c, sk, sk_len, msg, msg_len, msg_len, rnd, sig)


@pytest.mark.parametrize("param", [1, 2, 5])
def test_argument_errors_in_order_and_nothing_written(param):
    L = _lib()
    count = 2
    n, d, hp, a, k, sig_len = SETS[param]
    sk_len, msg_len = 4 * n, 33
    wsb = _ws(L, param, count)
    buf = np.full(wsb + (1 << 18), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256                              # the workspace first, 256-byte aligned
    lens = (sk_len, msg_len, n, sig_len)
    ptrs, at = [], WS + wsb
    for ln in lens:
        ptrs.append(at)
        at += count * ln + 64
    nul = [None] * 4
    for name, make, dev in (("sign_dev", lambda p: _sign_dev(L, p, sk_len, msg_len), True), ("sign", lambda p: _sign_host(L, p, sk_len, msg_len), False)):
        f = make(param)

        def call(cnt, p, w=WS, wb=wsb, g=f):
            return g(cnt, *p, w, wb)
        # 1. unknown param first of all, even with count = 0 and NULL pointers
        for bad in (-1, 6, 44, 768):
            assert call(count, ptrs, g=make(bad)) == ERR_PARAM, (name, bad)
            assert call(0, nul, w=None, wb=0, g=make(bad)) == ERR_PARAM, (name, bad)
        # count = 0: no work, no pointers, no workspace, no device
        assert call(0, nul, w=None, wb=0) == OK, name
        # 2. a NULL sk, msg or sig (addrnd may be NULL), before the strides, the byte counts, the workspace and the overlaps
        for i in (0, 1, 3):
            p = list(ptrs)
            p[i] = None
            assert call(count, p) == ERR_PARAM, (name, i)
            assert call(SMAX // 16, p) == ERR_PARAM, (name, i)
            if dev:
                assert call(count, p, w=None) == ERR_PARAM, (name, i)
        # 4. a byte count that overflows size_t
        assert call(SMAX // 16, ptrs) == ERR_PARAM, name
        assert call(SMAX // sig_len + 1, ptrs) == ERR_PARAM, name
        if dev:
            assert call(SMAX // (1 << 20), ptrs) == ERR_PARAM, name           # the buffers fit, the workspace does not
            # 5. the workspace: NULL, misaligned, too small
            assert call(count, ptrs, w=None) == ERR_PARAM, name
            for off in (1, 8, 64, 128):
                assert call(count, ptrs, w=WS + off) == ERR_PARAM, (name, off)
            assert call(count, ptrs, wb=wsb - 1) == ERR_PARAM, name
            assert call(count, ptrs, wb=0) == ERR_PARAM, name
            # ... before the overlaps
            p = list(ptrs)
            p[3] = p[0]
            assert call(count, p, wb=wsb - 1) == ERR_PARAM, name
        # 6. sig overlapping an input or the workspace
        for other in range(3):
            p = list(ptrs)
            p[3] = ptrs[other] + count * lens[other] - 1                      # its first byte is the other's last
            assert call(count, p) == ERR_PARAM, (name, other)
            p[3] = ptrs[other] - count * sig_len + 1                          # its last byte is the other's first
            assert call(count, p) == ERR_PARAM, (name, other)
        if dev:
            p = list(ptrs)
            p[3] = WS + wsb - 1
            assert call(count, p) == ERR_PARAM, name
            p[3] = WS - count * sig_len + 1
            assert call(count, p) == ERR_PARAM, name
        # a valid call (inputs may overlap each other; addrnd may be NULL) without a device is a HIP error
        if not _have_device():
            assert call(count, ptrs) == ERR_HIP, name
            assert call(count, [ptrs[0], ptrs[0], None, ptrs[3]]) == ERR_HIP, name
    # 3. the strides, each before the later classes
    args = (count, *ptrs, WS, wsb)
    assert _sign_dev(L, param, sk_len, 64, sk_stride=sk_len - 1)(*args) == ERR_PARAM
    assert _sign_dev(L, param, sk_len, 64, sk_stride=1)(*args) == ERR_PARAM
    assert _sign_dev(L, param, sk_len, 64, msg_stride=63)(*args) == ERR_PARAM
    assert _sign_dev(L, param, sk_len, 64, msg_stride=0)(*args) == ERR_PARAM
    assert _sign_dev(L, param, sk_len, 64, msg_stride=63)(SMAX // 16, *ptrs, None, 0) == ERR_PARAM         # the stride, before overflow and workspace
    assert _sign_dev(L, param, sk_len, SMAX - 8, msg_stride=SMAX)(1, *ptrs, WS, wsb) == ERR_PARAM           # 3 n + msg_len does not fit
    assert _sign_dev(L, param, sk_len, SMAX // 8, msg_stride=SMAX // 8)(1, *ptrs, WS, wsb) == ERR_PARAM     # nor does its bit count
    p = list(ptrs)
    p[3] = None                                                            # a NULL pointer comes before a bad stride
    assert _sign_dev(L, param, sk_len, 64, sk_stride=1)(count, *p, WS, wsb) == ERR_PARAM
    # more than 2^31 - 1 instances: unsupported, after every other check (a workspace of that size is only claimed, never touched)
    big = 1 << 31
    need = _ws(L, param, big)
    far = [1 << 40, 1 << 50, (1 << 50) + (1 << 45), 1 << 51]
    assert _sign_dev(L, param, sk_len, 64)(big, *far, 1 << 62, need) == ERR_UNSUPPORTED
    assert _sign_dev(L, param, sk_len, 64)(big, *far, 1 << 62, need - 1) == ERR_PARAM
    if not _have_device():
        # valid forms: one key for all, wider strides, an empty message without a pointer
        assert _sign_dev(L, param, sk_len, 64, sk_stride=0)(*args) == ERR_HIP
        assert _sign_dev(L, param, sk_len, 64, sk_stride=sk_len + 5, msg_stride=70)(*args) == ERR_HIP
        assert _sign_dev(L, param, sk_len, 0)(count, ptrs[0], None, *ptrs[2:], WS, wsb) == ERR_HIP
    assert (buf == 7).all()


def test_valid_calls_without_a_device_are_hip_errors():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    param, count = 3, 2
    n, d, hp, a, k, sig_len = SETS[param]
    wsb = _ws(L, param, count)
    buf = np.full(wsb + (1 << 18), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256
    A = WS + wsb
    B, R, S = A + 1000, A + 2000, A + 4000
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        assert L.psf_slhdsa_sha2_sign_dev(dev, param, count, A, 4 * n, B, 20, 20, R, S, WS, wsb, None) == ERR_HIP, dev
        assert L.psf_slhdsa_sha2_sign_dev(dev, param, count, A, 0, None, 0, 0, None, S, WS, wsb, None) == ERR_HIP, dev
        assert L.psf_slhdsa_sha2_sign(dev, param, count, A, 4 * n, B, 64, 64, None, S) == ERR_HIP, dev
    assert (buf == 7).all()
    import tools_amd as T
    D = T.slhdsa_sha2
    if not _have_device():
        for call in (lambda: D.sign_internal(NAMES[1], bytes(64), [b"m", b"n"]), lambda: D.sign_internal(NAMES[2], [bytes(96)], [b"m"], [bytes(24)]),
                     lambda: D.sign(NAMES[5], bytes(128), b"msg", ctx=b"c"), lambda: D.sign(NAMES[1], bytes(64), b"msg", deterministic=True)):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP
    with pytest.raises(ValueError):
        D.sign(NAMES[1], bytes(64), b"msg", ctx=bytes(256))
    with pytest.raises(ValueError):
        D.sign(TWINS[1], bytes(64), b"msg")                               # a SHAKE name is not a set of this module
    with pytest.raises(ValueError):
        D.sign_workspace_bytes(TWINS[0], 1)
    with pytest.raises(ValueError):
        D.sign_internal(NAMES[2], bytes(95), [b"m"])
    with pytest.raises(ValueError):
        D.sign_internal(NAMES[2], bytes(96), [b"m", b"mm"])
    with pytest.raises(ValueError):
        D.sign_internal(NAMES[2], bytes(96), [b"m"], [bytes(23)])
