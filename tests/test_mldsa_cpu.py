"""No-GPU checks of the ML-DSA entry points of include/psf_mi355x.h (psf_mldsa_*, psf_*_fips204*): every symbol exported and mirrored, the sizes and
workspace sizes, every argument error in its stated order (all checked before the first HIP call, so the codes hold on any host) with the guard
buffer unchanged, count = 0, and a valid call without a device PSF_ERR_HIP.  The device results are compared with the model in
tests/test_gpu_mldsa.py and tests/test_gpu_fips204.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
SMAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
STAGES = ("psf_sample_ntt_fips204", "psf_sample_bounded_fips204", "psf_sample_in_ball_fips204", "psf_ntt_image_from_fips204")
SYMBOLS = ("psf_mldsa_sizes", "psf_mldsa_workspace_bytes", "psf_mldsa_keygen_dev", "psf_mldsa_verify_dev", "psf_mldsa_keygen", "psf_mldsa_verify") + STAGES + \
    tuple(s + "_dev" for s in STAGES)
SIZES = {44: (1312, 2560, 2420), 65: (1952, 4032, 3309), 87: (2592, 4896, 4627)}
KL = {44: (4, 4), 65: (6, 5), 87: (8, 7)}
KEYGEN, VERIFY = 0, 1
BYTES, MU = 0, 1


def _lib():
    from tools_amd import fips204, mldsa
    fips204._lib()
    return mldsa._lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _ws(L, param, count, op):
    out = C.c_size_t(0)
    assert L.psf_mldsa_workspace_bytes(param, count, op, C.byref(out)) == OK
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
    for const in ("PSF_MLDSA_44: psf_status = 44", "PSF_MLDSA_65: psf_status = 65", "PSF_MLDSA_87: psf_status = 87", "PSF_MLDSA_OP_VERIFY: psf_status = 1",
                  "PSF_MLDSA_MSG_MU: psf_status = 1", "PSF_MLDSA_WHY_HINT: psf_status = 1", "PSF_MLDSA_WHY_NORM: psf_status = 2", "PSF_MLDSA_WHY_HASH: psf_status = 4"):
        assert const in ffi, const
    import tools_amd as T
    for name in ("sizes", "workspace_bytes", "keygen_dev", "verify_dev", "keygen_internal", "verify_internal", "keygen", "verify"):
        assert callable(getattr(T.mldsa, name)), name
    for name in ("sample_ntt_dev", "sample_ntt", "sample_bounded_dev", "sample_bounded", "sample_in_ball_dev", "sample_in_ball", "image_from_fips204_dev",
                 "image_from_fips204"):
        assert callable(getattr(T.fips204, name)), name
    assert (T.mldsa.WHY_HINT, T.mldsa.WHY_NORM, T.mldsa.WHY_HASH, T.mldsa.MSG_BYTES, T.mldsa.MSG_MU) == (1, 2, 4, 0, 1)


def test_sizes():
    L = _lib()
    import tools_amd as T
    for param, want in SIZES.items():
        v = [C.c_size_t(0) for _ in range(3)]
        assert L.psf_mldsa_sizes(param, *[C.byref(x) for x in v]) == OK
        assert tuple(x.value for x in v) == want
        assert L.psf_mldsa_sizes(param, None, None, None) == OK
        assert T.mldsa.sizes(f"ML-DSA-{param}") == dict(zip(("pk", "sk", "sig"), want))
    for param in (-1, 0, 2, 3, 4, 43, 66, 88, 1024):
        assert L.psf_mldsa_sizes(param, None, None, None) == ERR_PARAM


def test_workspace_bytes_values_and_monotonicity():
    L = _lib()
    out = C.c_size_t(99)
    for param in (-1, 0, 2, 45):
        assert L.psf_mldsa_workspace_bytes(param, 1, KEYGEN, C.byref(out)) == ERR_PARAM
    for op in (-1, 2, 100):
        assert L.psf_mldsa_workspace_bytes(65, 1, op, C.byref(out)) == ERR_PARAM
    assert L.psf_mldsa_workspace_bytes(65, 1, KEYGEN, None) == ERR_PARAM
    assert L.psf_mldsa_workspace_bytes(65, SMAX // 1024, VERIFY, C.byref(out)) == ERR_PARAM       # does not fit size_t
    assert out.value == 99
    for param, (k, l) in KL.items():
        for op in (KEYGEN, VERIFY):
            last = 0
            for count in (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 67, 255, 256, 259, 4096, 65536):
                w = _ws(L, param, count, op)
                assert w % 256 == 0 and w >= last, (param, op, count)
                last = w
            assert _ws(L, param, 0, op) == 0
        # the images of A_hat are k l 1024 bytes per instance; every other polynomial is 2048 bytes of 64-bit words
        assert _ws(L, param, 65536, KEYGEN) >= 65536 * (k * l * 1024 + (2 * k + l) * 2048 + 64)
        assert _ws(L, param, 65536, VERIFY) >= 65536 * (k * l * 1024 + (2 * k + l + 1) * 2048 + 128 + 4 + 32 * k)
        assert _ws(L, param, 65536, VERIFY) < 65536 * 256 * 1024
    assert _ws(L, 87, 65536, KEYGEN) > 1 << 32 and _ws(L, 87, 65536, VERIFY) > 1 << 32      # offsets past 32 bits at ML-DSA-87


def _keygen_dev(L, param):
    return lambda c, xi, pk, sk, w, wb: L.psf_mldsa_keygen_dev(0, param, c, xi, pk, sk, w, wb, None, None)


def _verify_dev(L, param, pk_len, sig_len, msg_len=33, kind=BYTES, pk_stride=None, msg_stride=None):
    ps = pk_len if pk_stride is None else pk_stride
    ms = msg_len if msg_stride is None else msg_stride
    return lambda c, pk, msg, sig, ok, why, w, wb: L.psf_mldsa_verify_dev(0, param, c, pk, ps, msg, msg_len, ms, kind, sig, ok, why, w, wb, None, None)


@pytest.mark.parametrize("param", [44, 65, 87])
def test_argument_errors_in_order_and_nothing_written(param):
    L = _lib()
    count = 2
    pk_len, sk_len, sig_len = SIZES[param]
    wsb = max(_ws(L, param, count, op) for op in (KEYGEN, VERIFY))
    buf = np.full(wsb + (1 << 16), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256                              # the workspace first, 256-byte aligned
    P = WS + wsb
    msg_len = 33
    calls = {
        "keygen_dev": (_keygen_dev, (32, pk_len, sk_len), 1, KEYGEN, True),
        "verify_dev": (lambda L_, p: _verify_dev(L_, p, pk_len, sig_len, msg_len), (pk_len, msg_len, sig_len, 1, 1), 3, VERIFY, True),
        "keygen": (lambda L_, p: (lambda c, xi, pk, sk, w=None, wb=0: L_.psf_mldsa_keygen(0, p, c, xi, pk, sk)), (32, pk_len, sk_len), 1, KEYGEN, False),
        "verify": (lambda L_, p: (lambda c, pk, msg, sig, ok, why, w=None, wb=0: L_.psf_mldsa_verify(0, p, c, pk, pk_len, msg, msg_len, msg_len, BYTES, sig, ok, why)),
                   (pk_len, msg_len, sig_len, 1, 1), 3, VERIFY, False),
    }
    for name, (make, lens, n_in, op, dev) in calls.items():
        f = make(L, param)
        ptrs, at = [], P
        for ln in lens:
            ptrs.append(at)
            at += count * ln + 64
        nul = [None] * len(ptrs)

        def call(cnt, p, w=WS, wb=wsb, g=f):
            return g(cnt, *p, w, wb)
        # 1. unknown param first of all, even with count = 0 and NULL pointers
        for bad in (-1, 0, 2, 3, 45, 768):
            g = make(L, bad)
            assert call(count, ptrs, g=g) == ERR_PARAM, (name, bad)
            assert call(0, nul, w=None, wb=0, g=g) == ERR_PARAM, (name, bad)
        # count = 0: no work, no pointers, no workspace, no device
        assert call(0, nul, w=None, wb=0) == OK, name
        # 2. a NULL data pointer, before the strides, the byte counts, the workspace and the overlaps (d_why may be NULL)
        for i in range(len(ptrs)):
            if name.startswith("verify") and i == 4:
                continue
            p = list(ptrs)
            p[i] = None
            assert call(count, p) == ERR_PARAM, (name, i)
            assert call(SMAX // 16, p) == ERR_PARAM, (name, i)
            if dev:
                assert call(count, p, w=None) == ERR_PARAM, (name, i)
        # 4. a byte count that overflows size_t
        assert call(SMAX // 16, ptrs) == ERR_PARAM, name
        assert call(SMAX // max(lens) + 1, ptrs) == ERR_PARAM, name
        if dev:
            assert call(SMAX // (1 << 18), ptrs) == ERR_PARAM, name           # the buffers fit, the workspace does not
            # 5. the workspace: NULL, misaligned, too small
            need = _ws(L, param, count, op)
            assert call(count, ptrs, w=None) == ERR_PARAM, name
            for off in (1, 8, 64, 128):
                assert call(count, ptrs, w=WS + off) == ERR_PARAM, (name, off)
            assert call(count, ptrs, wb=need - 1) == ERR_PARAM, name
            assert call(count, ptrs, wb=0) == ERR_PARAM, name
            # ... before the overlaps
            p = list(ptrs)
            p[-1] = p[0]
            assert call(count, p, wb=need - 1) == ERR_PARAM, name
        # 6. an output that overlaps an input, another output, the workspace
        for o in range(n_in, len(ptrs)):
            for other in range(len(ptrs)):
                if other == o:
                    continue
                p = list(ptrs)
                p[o] = ptrs[other] + count * lens[other] - 1                  # its first byte is the other's last
                assert call(count, p) == ERR_PARAM, (name, o, other)
                p[o] = ptrs[other] - count * lens[o] + 1                      # its last byte is the other's first
                assert call(count, p) == ERR_PARAM, (name, o, other)
            if dev:
                p = list(ptrs)
                p[o] = WS + need - 1
                assert call(count, p) == ERR_PARAM, (name, o)
                p[o] = WS - count * lens[o] + 1
                assert call(count, p) == ERR_PARAM, (name, o)
        # a valid call (inputs may overlap each other) without a device is a HIP error
        if not _have_device():
            assert call(count, ptrs) == ERR_HIP, name
            if name.startswith("verify"):
                p = list(ptrs)
                p[1] = p[0]
                assert call(count, p) == ERR_HIP, name
                p = list(ptrs)
                p[4] = None
                assert call(count, p) == ERR_HIP, name
    # verify: msg_kind, then the strides and MSG_MU's length (3.), each before the later classes
    ptrs, at = [], P
    for ln in (pk_len, 64, sig_len, 1, 1):
        ptrs.append(at)
        at += count * ln + 64
    for kind in (-1, 2, 7):
        assert _verify_dev(L, param, pk_len, sig_len, 64, kind)(count, *ptrs, WS, wsb) == ERR_PARAM
        assert _verify_dev(L, param, pk_len, sig_len, 64, kind)(0, None, None, None, None, None, None, 0) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, pk_stride=pk_len - 1)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, pk_stride=1)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, msg_stride=63)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, msg_stride=0)(count, *ptrs, WS, wsb) == ERR_PARAM
    for bad_len in (0, 32, 63, 65):
        assert _verify_dev(L, param, pk_len, sig_len, bad_len, MU, msg_stride=128)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, sig_len, 64, MU, msg_stride=63)(SMAX // 16, *ptrs, None, 0) == ERR_PARAM      # the stride, before overflow and workspace
    # a NULL pointer comes before a bad stride
    p = list(ptrs)
    p[2] = None
    assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, pk_stride=1)(count, *p, WS, wsb) == ERR_PARAM
    # more than 2^31 - 1 instances: unsupported, after every other check (a workspace of that size is only claimed, never touched)
    big = 1 << 31
    need = _ws(L, param, big, VERIFY)
    far = [1 << 60, 1 << 61, (1 << 61) + (1 << 59), 1 << 62, (1 << 62) + (1 << 40)]
    assert _verify_dev(L, param, pk_len, sig_len, 64, MU)(big, *far, 256, need) == ERR_UNSUPPORTED
    assert _verify_dev(L, param, pk_len, sig_len, 64, MU)(big, *far, 256, need - 1) == ERR_PARAM
    assert L.psf_mldsa_keygen_dev(0, param, big, far[0], far[1], far[3], 256, _ws(L, param, big, KEYGEN), None, None) == ERR_UNSUPPORTED
    if not _have_device():
        # valid forms: one key for all, an empty message without a pointer, mu as the message
        assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, pk_stride=0)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _verify_dev(L, param, pk_len, sig_len, 64, BYTES, pk_stride=pk_len + 5, msg_stride=70)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _verify_dev(L, param, pk_len, sig_len, 0, BYTES)(count, ptrs[0], None, *ptrs[2:], WS, wsb) == ERR_HIP
        assert _verify_dev(L, param, pk_len, sig_len, 64, MU)(count, *ptrs, WS, wsb) == ERR_HIP
    assert (buf == 7).all()


def test_stage_argument_errors():
    L = _lib()
    buf = np.full(1 << 16, 7, dtype=np.uint8)
    S = buf.ctypes.data
    O = (S + 4096 + 7) // 8 * 8
    dev = not _have_device()
    # sample_ntt: k, l; stride; NULL; overflow; overlap
    for k, l in ((256, 1), (1, 256), (0, 1), (1, 0)):
        assert L.psf_sample_ntt_fips204_dev(0, 1, k, l, S, 34, O, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, 2, 0, 0, S, 33, O, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, 2, 4, 4, S, 31, O, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, 2, 0, 0, None, 34, O, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, 2, 0, 0, S, 34, None, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, SMAX // 64, 0, 0, S, 34, O, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, 2, 0, 0, S, 34, S + 60, None, None) == ERR_PARAM
    assert L.psf_sample_ntt_fips204_dev(0, 0, 0, 0, None, 34, None, None, None) == OK
    assert L.psf_sample_ntt_fips204(0, 2, 0, 0, S, 33, O) == ERR_PARAM
    # sample_bounded: eta = 0; nonces; stride ...; then unsupported eta
    assert L.psf_sample_bounded_fips204_dev(0, 1, 0, S, 64, 0, 1, O, None, None) == ERR_PARAM
    assert L.psf_sample_bounded_fips204_dev(0, 1, 2, S, 64, 65536, 1, O, None, None) == ERR_PARAM
    assert L.psf_sample_bounded_fips204_dev(0, 1, 2, S, 64, 65537, 0, O, None, None) == ERR_PARAM
    assert L.psf_sample_bounded_fips204_dev(0, 1, 2, S, 63, 0, 1, O, None, None) == ERR_PARAM
    assert L.psf_sample_bounded_fips204_dev(0, 1, 3, S, 63, 0, 1, O, None, None) == ERR_PARAM       # the stride comes before the unsupported eta
    assert L.psf_sample_bounded_fips204_dev(0, 1, 2, None, 64, 0, 1, O, None, None) == ERR_PARAM
    assert L.psf_sample_bounded_fips204_dev(0, 1, 2, S, 64, 0, 1, S + 8, None, None) == ERR_PARAM
    for eta in (1, 3, 5, 8):
        assert L.psf_sample_bounded_fips204_dev(0, 1, eta, S, 64, 0, 1, O, None, None) == ERR_UNSUPPORTED
        assert L.psf_sample_bounded_fips204(0, 1, eta, S, 64, 0, 1, O) == ERR_UNSUPPORTED
    assert L.psf_sample_bounded_fips204_dev(0, 3, 2, S, 64, 5, 0, O, None, None) == OK             # per_seed = 0
    # sample_in_ball: tau
    for tau in (0, 65, 256):
        assert L.psf_sample_in_ball_fips204_dev(0, 1, tau, S, 32, 32, O, None, None) == ERR_PARAM
    assert L.psf_sample_in_ball_fips204_dev(0, 2, 39, S, 32, 31, O, None, None) == ERR_PARAM
    assert L.psf_sample_in_ball_fips204_dev(0, 2, 39, S, 32, 32, None, None, None) == ERR_PARAM
    assert L.psf_sample_in_ball_fips204_dev(0, 2, 39, S, 32, 32, S + 63, None, None) == ERR_PARAM
    # image_from
    assert L.psf_ntt_image_from_fips204_dev(0, 1, None, O, None) == ERR_PARAM
    assert L.psf_ntt_image_from_fips204_dev(0, 1, O, None, None) == ERR_PARAM
    assert L.psf_ntt_image_from_fips204_dev(0, SMAX // 1024, O, O + (1 << 40), None) == ERR_PARAM
    assert L.psf_ntt_image_from_fips204_dev(0, 2, O, O + 4095, None) == ERR_PARAM
    assert L.psf_ntt_image_from_fips204_dev(0, 0, None, None, None) == OK
    if dev:
        assert L.psf_sample_ntt_fips204_dev(0, 2, 4, 4, S, 32, O, None, None) == ERR_HIP
        assert L.psf_sample_ntt_fips204(0, 2, 0, 0, S, 34, O) == ERR_HIP
        assert L.psf_sample_bounded_fips204_dev(0, 2, 4, S, 64, 3, 2, O, None, None) == ERR_HIP
        assert L.psf_sample_bounded_fips204(0, 2, 2, S, 64, 0, 2, O) == ERR_HIP
        assert L.psf_sample_in_ball_fips204_dev(0, 2, 60, S, 64, 64, O, None, None) == ERR_HIP
        assert L.psf_sample_in_ball_fips204(0, 2, 1, S, 32, 32, O) == ERR_HIP
        assert L.psf_ntt_image_from_fips204_dev(0, 2, O, O + 8192, None) == ERR_HIP
        assert L.psf_ntt_image_from_fips204(0, 2, O, O + 8192) == ERR_HIP
    assert (buf == 7).all()


def test_valid_calls_without_a_device_are_hip_errors():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    param, count = 65, 2
    pk_len, sk_len, sig_len = SIZES[param]
    wsb = max(_ws(L, param, count, op) for op in (KEYGEN, VERIFY))
    buf = np.full(wsb + (1 << 16), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256
    A = WS + wsb
    B, Cc, O1, O2 = A + 5000, A + 12000, A + 20000, A + 30000
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        assert L.psf_mldsa_keygen_dev(dev, param, count, A, O1, O2, WS, wsb, None, None) == ERR_HIP, dev
        assert L.psf_mldsa_verify_dev(dev, param, count, A, pk_len, B, 20, 20, BYTES, Cc, O1, O2, WS, wsb, None, None) == ERR_HIP, dev
        assert L.psf_mldsa_keygen(dev, param, count, A, O1, O2) == ERR_HIP, dev
        assert L.psf_mldsa_verify(dev, param, count, A, 0, B, 64, 64, MU, Cc, O1, None) == ERR_HIP, dev
    assert (buf == 7).all()
    if not _have_device():
        import tools_amd as T
        D = T.mldsa
        for call in (lambda: D.keygen_internal("ML-DSA-44", [bytes(32)]), lambda: D.keygen("ML-DSA-87", 2),
                     lambda: D.verify_internal("ML-DSA-65", bytes(1952), [b"m"], [bytes(3309)]), lambda: D.verify("ML-DSA-44", bytes(1312), b"msg", bytes(2420), ctx=b"c"),
                     lambda: T.fips204.sample_in_ball(np.zeros((2, 32), np.uint8), 39)):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP
        assert D.verify("ML-DSA-44", bytes(1312), b"msg", bytes(2420), ctx=bytes(256)) is False
        with pytest.raises(ValueError):
            D.verify_internal("ML-DSA-65", bytes(1951), [b"m"], [bytes(3309)])
        with pytest.raises(ValueError):
            D.sizes("ML-DSA-128")
