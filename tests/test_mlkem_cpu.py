"""No-GPU checks of the ML-KEM entry points of include/psf_mi355x.h (psf_mlkem_*): every symbol exported and mirrored, the sizes and workspace
sizes, every argument error in its stated order (all checked before the first HIP call, so the codes hold on any host) with the guard buffer
unchanged, count = 0, and a valid call without a device PSF_ERR_HIP.  The device results are compared with the model in tests/test_gpu_mlkem.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP = 0, 1, 7
SMAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
DEV = ("psf_mlkem_keygen_dev", "psf_mlkem_encaps_dev", "psf_mlkem_decaps_dev", "psf_mlkem_check_ek_dev", "psf_mlkem_check_dk_dev")
HOST = ("psf_mlkem_keygen", "psf_mlkem_encaps", "psf_mlkem_decaps", "psf_mlkem_check_ek", "psf_mlkem_check_dk")
SYMBOLS = ("psf_mlkem_sizes", "psf_mlkem_workspace_bytes") + DEV + HOST
SIZES = {2: (800, 1632, 768, 32), 3: (1184, 2400, 1088, 32), 4: (1568, 3168, 1568, 32)}
KEYGEN, ENCAPS, DECAPS, CHECK = range(4)


def _lib():
    from tools_amd import mlkem
    return mlkem._lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _ws(L, param, count, op):
    out = C.c_size_t(0)
    assert L.psf_mlkem_workspace_bytes(param, count, op, C.byref(out)) == OK
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
    for const in ("PSF_MLKEM_512: psf_status = 2", "PSF_MLKEM_768: psf_status = 3", "PSF_MLKEM_1024: psf_status = 4", "PSF_MLKEM_OP_CHECK: psf_status = 3"):
        assert const in ffi, const
    import tools_amd as T
    for name in ("sizes", "workspace_bytes", "keygen_dev", "encaps_dev", "decaps_dev", "check_ek_dev", "check_dk_dev", "keygen_internal", "encaps_internal",
                 "decaps", "check_ek", "check_dk", "keygen", "encaps"):
        assert callable(getattr(T.mlkem, name)), name


def test_sizes():
    L = _lib()
    import tools_amd as T
    for param, want in SIZES.items():
        v = [C.c_size_t(0) for _ in range(4)]
        assert L.psf_mlkem_sizes(param, *[C.byref(x) for x in v]) == OK
        assert tuple(x.value for x in v) == want
        assert L.psf_mlkem_sizes(param, None, None, None, None) == OK
        name = {2: "ML-KEM-512", 3: "ML-KEM-768", 4: "ML-KEM-1024"}[param]
        assert T.mlkem.sizes(name) == dict(zip(("ek", "dk", "ct", "ss"), want))
    for param in (-1, 0, 1, 5, 512):
        assert L.psf_mlkem_sizes(param, None, None, None, None) == ERR_PARAM


def test_workspace_bytes_values_and_monotonicity():
    L = _lib()
    out = C.c_size_t(99)
    for param in (-1, 0, 1, 5):
        assert L.psf_mlkem_workspace_bytes(param, 1, KEYGEN, C.byref(out)) == ERR_PARAM
    for op in (-1, 4, 100):
        assert L.psf_mlkem_workspace_bytes(3, 1, op, C.byref(out)) == ERR_PARAM
    assert L.psf_mlkem_workspace_bytes(3, 1, KEYGEN, None) == ERR_PARAM
    assert L.psf_mlkem_workspace_bytes(3, SMAX // 1024, DECAPS, C.byref(out)) == ERR_PARAM       # does not fit size_t
    assert out.value == 99
    for param, (ek, dk, ct, ss) in SIZES.items():
        k = param
        for op in (KEYGEN, ENCAPS, DECAPS, CHECK):
            last = 0
            for count in (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 67, 255, 256, 259, 4096, 65536):
                w = _ws(L, param, count, op)
                assert w % 256 == 0 and w >= last, (param, op, count)
                last = w
            assert _ws(L, param, 0, op) == 0
            assert _ws(L, param, 1, CHECK) == 0
        # the images of A_hat alone are k * k * 1024 bytes per instance; every secret polynomial has a place as well
        assert _ws(L, param, 65536, KEYGEN) >= 65536 * (k * k * 1024 + k * k * 512 + 3 * k * 512)
        assert _ws(L, param, 65536, ENCAPS) >= 65536 * (k * k + k) * 1536
        assert _ws(L, param, 65536, DECAPS) >= 65536 * ((k * k + 2 * k) * 1536 + ct)
        assert _ws(L, param, 65536, DECAPS) < 65536 * 64 * 1024
    assert _ws(L, 4, 65536, DECAPS) >= 1 << 30                            # about 1 GiB of matrix images at ML-KEM-1024


def _calls(L, param, ws, ws_bytes, like=None):
    """every entry point as name: (f(count, pointers...), the item sizes of its buffers, how many are inputs, its workspace op); `like`: the set
    whose sizes lay the buffers out when `param` is not one"""
    ek, dk, ct, _ = SIZES[like or param]
    return {
        "psf_mlkem_keygen_dev": (lambda c, a, b, o1, o2, w=ws, wb=ws_bytes: L.psf_mlkem_keygen_dev(0, param, c, a, b, o1, o2, w, wb, None, None), (32, 32, ek, dk), 2, KEYGEN),
        "psf_mlkem_encaps_dev": (lambda c, a, b, o1, o2, w=ws, wb=ws_bytes: L.psf_mlkem_encaps_dev(0, param, c, a, b, o1, o2, w, wb, None, None), (ek, 32, 32, ct), 2, ENCAPS),
        "psf_mlkem_decaps_dev": (lambda c, a, b, o1, w=ws, wb=ws_bytes: L.psf_mlkem_decaps_dev(0, param, c, a, b, o1, w, wb, None, None), (dk, ct, 32), 2, DECAPS),
        "psf_mlkem_check_ek_dev": (lambda c, a, o1, w=None, wb=0: L.psf_mlkem_check_ek_dev(0, param, c, a, o1, None), (ek, 1), 1, None),
        "psf_mlkem_check_dk_dev": (lambda c, a, o1, w=None, wb=0: L.psf_mlkem_check_dk_dev(0, param, c, a, o1, None), (dk, 1), 1, None),
        "psf_mlkem_keygen": (lambda c, a, b, o1, o2, w=None, wb=0: L.psf_mlkem_keygen(0, param, c, a, b, o1, o2), (32, 32, ek, dk), 2, None),
        "psf_mlkem_encaps": (lambda c, a, b, o1, o2, w=None, wb=0: L.psf_mlkem_encaps(0, param, c, a, b, o1, o2), (ek, 32, 32, ct), 2, None),
        "psf_mlkem_decaps": (lambda c, a, b, o1, w=None, wb=0: L.psf_mlkem_decaps(0, param, c, a, b, o1), (dk, ct, 32), 2, None),
        "psf_mlkem_check_ek": (lambda c, a, o1, w=None, wb=0: L.psf_mlkem_check_ek(0, param, c, a, o1), (ek, 1), 1, None),
        "psf_mlkem_check_dk": (lambda c, a, o1, w=None, wb=0: L.psf_mlkem_check_dk(0, param, c, a, o1), (dk, 1), 1, None),
    }


@pytest.mark.parametrize("param", [2, 3, 4])
def test_argument_errors_in_order_and_nothing_written(param):
    L = _lib()
    count = 2
    wsb = max(_ws(L, param, count, op) for op in (KEYGEN, ENCAPS, DECAPS))
    buf = np.full(wsb + (1 << 16), 7, dtype=np.uint8)
    base = buf.ctypes.data
    WS = (base + 255) // 256 * 256                                           # the workspace first, 256-byte aligned
    P = WS + wsb
    for name, (f, lens, n_in, op) in _calls(L, param, WS, wsb).items():
        ptrs, at = [], P
        for ln in lens:
            ptrs.append(at)
            at += count * ln + 64
        dev3 = op is not None

        def call(cnt, p, w=WS, wb=wsb):
            return f(cnt, *p, w=w, wb=wb) if dev3 else f(cnt, *p)
        # 1. unknown param first of all: checked through a sibling with the same pointers (even with count = 0 and NULL pointers)
        for bad in (-1, 0, 1, 5, 768):
            g = _calls(L, bad, WS, wsb, like=param)[name][0]
            assert (g(count, *ptrs) if not dev3 else g(count, *ptrs, w=WS, wb=wsb)) == ERR_PARAM, (name, bad)
            assert (g(0, *[None] * len(ptrs)) if not dev3 else g(0, *[None] * len(ptrs), w=None, wb=0)) == ERR_PARAM, (name, bad)
        # count = 0: no work, no pointers, no workspace, no device
        assert (f(0, *[None] * len(ptrs)) if not dev3 else f(0, *[None] * len(ptrs), w=None, wb=0)) == OK, name
        # 2. a NULL data pointer, before the byte counts, the workspace and the overlaps
        for i in range(len(ptrs)):
            p = list(ptrs)
            p[i] = None
            assert call(count, p) == ERR_PARAM, (name, i)
            assert call(SMAX // 16, p) == ERR_PARAM, (name, i)
            if dev3:
                assert call(count, p, w=None) == ERR_PARAM, (name, i)
        # 3. a byte count that overflows size_t
        assert call(SMAX // 16, ptrs) == ERR_PARAM, name
        assert call(SMAX // max(lens) + 1, ptrs) == ERR_PARAM, name
        if dev3:
            assert call(SMAX // (1 << 16), ptrs) == ERR_PARAM, name           # the buffers fit, the workspace does not
            # 4. the workspace: NULL, misaligned, too small
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
        # 5. an output that overlaps an input, another output, the workspace
        for o in range(n_in, len(ptrs)):
            for other in range(len(ptrs)):
                if other == o:
                    continue
                p = list(ptrs)
                p[o] = ptrs[other] + count * lens[other] - 1                  # its first byte is the other's last
                assert call(count, p) == ERR_PARAM, (name, o, other)
                p[o] = ptrs[other] - count * lens[o] + 1                      # its last byte is the other's first
                assert call(count, p) == ERR_PARAM, (name, o, other)
            if dev3:
                p = list(ptrs)
                p[o] = WS + need - 1
                assert call(count, p) == ERR_PARAM, (name, o)
                p[o] = WS - count * lens[o] + 1
                assert call(count, p) == ERR_PARAM, (name, o)
        # two inputs may overlap: the call is valid, and without a device it is a HIP error
        if n_in == 2 and not _have_device():
            p = list(ptrs)
            p[1] = p[0]
            assert call(count, p) == ERR_HIP, name
    assert (buf == 7).all()


def test_valid_calls_without_a_device_are_hip_errors():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    param, count = 3, 2
    ek, dk, ct, _ = SIZES[param]
    wsb = max(_ws(L, param, count, op) for op in (KEYGEN, ENCAPS, DECAPS))
    buf = np.full(wsb + (1 << 15), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256
    A = WS + wsb
    B, O1, O2 = A + 5000, A + 10000, A + 15000
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        assert L.psf_mlkem_keygen_dev(dev, param, count, A, B, O1, O2, WS, wsb, None, None) == ERR_HIP, dev
        assert L.psf_mlkem_encaps_dev(dev, param, count, A, B, O1, O2, WS, wsb, None, None) == ERR_HIP, dev
        assert L.psf_mlkem_decaps_dev(dev, param, count, A, B, O1, WS, wsb, None, None) == ERR_HIP, dev
        assert L.psf_mlkem_check_ek_dev(dev, param, count, A, O1, None) == ERR_HIP, dev
        assert L.psf_mlkem_check_dk_dev(dev, param, count, A, O1, None) == ERR_HIP, dev
        assert L.psf_mlkem_keygen(dev, param, count, A, B, O1, O2) == ERR_HIP, dev
        assert L.psf_mlkem_encaps(dev, param, count, A, B, O1, O2) == ERR_HIP, dev
        assert L.psf_mlkem_decaps(dev, param, count, A, B, O1) == ERR_HIP, dev
        assert L.psf_mlkem_check_ek(dev, param, count, A, O1) == ERR_HIP, dev
        assert L.psf_mlkem_check_dk(dev, param, count, A, O1) == ERR_HIP, dev
    assert (buf == 7).all()
    if not _have_device():
        import tools_amd as T
        K = T.mlkem
        for call in (lambda: K.keygen_internal("ML-KEM-512", [bytes(32)], [bytes(32)]), lambda: K.encaps_internal("ML-KEM-768", [bytes(1184)], [bytes(32)]),
                     lambda: K.decaps("ML-KEM-1024", [bytes(3168)], [bytes(1568)]), lambda: K.check_ek("ML-KEM-512", [bytes(800)]),
                     lambda: K.check_dk("ML-KEM-512", [bytes(1632)]), lambda: K.keygen("ML-KEM-512", 2), lambda: K.encaps("ML-KEM-512", [bytes(800)])):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP
        with pytest.raises(ValueError):
            K.encaps_internal("ML-KEM-768", [bytes(1183)], [bytes(32)])
        with pytest.raises(ValueError):
            K.sizes("ML-KEM-2048")
