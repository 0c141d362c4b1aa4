"""No-GPU checks of the FIPS 203 entry points of include/psf_mi355x.h (psf_keccak*, psf_sample_*_fips203*, psf_ntt_image_*_fips203*): every symbol
exported, every argument error in its stated order (all checked before the first HIP call, so the codes hold on any host), a valid call without a
device PSF_ERR_HIP, and the regenerated FFI.  The device results are compared with hashlib and the model in tests/test_gpu_fips203.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
SMAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
SYMBOLS = ("psf_keccak_dev", "psf_keccak", "psf_sample_ntt_fips203_dev", "psf_sample_ntt_fips203", "psf_sample_cbd_fips203_dev",
           "psf_sample_cbd_fips203", "psf_ntt_image_from_fips203_dev", "psf_ntt_image_to_fips203_dev", "psf_ntt_image_from_fips203",
           "psf_ntt_image_to_fips203")


def _lib():
    from tools_amd import _ffi
    return _ffi.lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def test_every_symbol_is_exported_and_mirrored():
    L = _lib()
    for fn in SYMBOLS:
        assert hasattr(L, fn), fn
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"])
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "psf_mi355x.hpp")).read()
    for fn in SYMBOLS:
        assert f"pub fn {fn}(" in ffi, fn
    for fn in SYMBOLS:
        if fn.endswith("_dev") or fn == "psf_keccak":
            assert fn + "(" in hpp, fn
    import tools_amd as T
    for name in ("keccak", "sample_ntt", "sample_cbd", "image_from_fips203", "image_to_fips203"):
        assert callable(getattr(T.fips203, name)) and callable(getattr(T.fips203, name + "_dev")), name


def test_keccak_argument_errors():
    L = _lib()
    buf = np.full(4096, 7, dtype=np.uint8)
    P = buf.ctypes.data
    IN, OUT = P, P + 2048

    for name in ("psf_keccak_dev", "psf_keccak"):
        def f(func, count, i, il, ist, o, ol, ost, name=name):
            args = [0, func, count, i, il, ist, o, ol, ost] + ([None] if name.endswith("_dev") else [])
            return getattr(L, name)(*args)
        for func in (-1, 4, 100):                                            # unknown function first of all
            assert f(func, 2, IN, 8, 8, OUT, 32, 32) == ERR_PARAM
            assert f(func, 0, None, 8, 4, None, 0, 0) == ERR_PARAM
        for func, good in ((0, 32), (1, 64)):                                # SHA3: the one digest length
            for ol in (0, 1, 31, 33, 64 if func == 0 else 32, 136):
                assert f(func, 2, IN, 8, 8, OUT, ol, max(ol, 1)) == ERR_PARAM, (func, ol)
                assert f(func, 0, IN, 8, 8, OUT, ol, max(ol, 1)) == ERR_PARAM, (func, ol)      # ... checked before count = 0
            assert f(func, 0, IN, 8, 8, OUT, good, good) == OK
        for func in (2, 3):
            assert f(func, 2, IN, 8, 8, OUT, 0, 0) == ERR_PARAM              # out_len = 0
            assert f(func, 0, None, 0, 0, None, 1, 1) == OK                  # count = 0: no work, no device, no pointers
            assert f(func, 0, None, 1600, 1600, None, 1000, 1000) == OK
            assert f(func, 2, IN, 8, 7, OUT, 32, 32) == ERR_PARAM            # a stride smaller than its length
            assert f(func, 2, IN, 8, 8, OUT, 32, 31) == ERR_PARAM
            assert f(func, 0, IN, 8, 7, OUT, 32, 32) == ERR_PARAM
            assert f(func, 2, IN, 8, 8, None, 32, 32) == ERR_PARAM           # NULL with count > 0
            assert f(func, 2, None, 8, 8, OUT, 32, 32) == ERR_PARAM
            assert f(func, 2, None, 8, 7, OUT, 32, 32) == ERR_PARAM
            assert f(func, 3, IN, 8, SMAX // 2, OUT, 32, 32) == ERR_PARAM    # (count - 1) stride + len overflows size_t
            assert f(func, SMAX // 16, IN, 8, 8, OUT, 32, 32) == ERR_PARAM
            assert f(func, 2, IN, 8, 8, OUT, 32, SMAX) == ERR_PARAM
            assert f(func, 2, IN, 64, 64, IN + 127, 32, 32) == ERR_PARAM     # the last input byte is the first output byte
            assert f(func, 2, IN, 64, 64, IN, 32, 32) == ERR_PARAM
            assert f(func, 2, IN + 63, 64, 64, IN, 32, 32) == ERR_PARAM
            assert f(func, 2, IN, 8, 1024, IN + 16, 8, 1024) == ERR_PARAM    # interleaved rows count as overlapping ranges
    assert (buf == 7).all()


def _ntt_forms(L):
    def dev(count, k, seed, stride, out, io=64):
        return L.psf_sample_ntt_fips203_dev(0, count, k, seed, stride, out, None, io, None)

    def host(count, k, seed, stride, out, io=64):
        return L.psf_sample_ntt_fips203(0, count, k, seed, stride, out)
    return {"dev": dev, "host": host}


def test_sample_ntt_argument_errors():
    L = _lib()
    buf = np.full(1 << 16, 7, dtype=np.uint8)
    SEED, OUT = buf.ctypes.data, buf.ctypes.data + 4096
    for name, f in _ntt_forms(L).items():
        for k in (17, 255, 0xFFFFFFFF):
            assert f(1, k, SEED, 32, OUT) == ERR_PARAM, (name, k)
            assert f(0, k, None, 0, None) == ERR_PARAM, (name, k)
        if name == "dev":
            for io in (0, 8, 32, -16, 63):
                assert f(1, 0, SEED, 34, OUT, io) == ERR_PARAM, io
                assert f(0, 0, SEED, 34, OUT, io) == ERR_PARAM, io
            assert f(0, 3, None, 32, None, 16) == OK
        assert f(1, 0, SEED, 33, OUT) == ERR_PARAM, name                     # the raw form reads 34 bytes
        assert f(1, 1, SEED, 31, OUT) == ERR_PARAM, name                     # the matrix form 32
        assert f(0, 1, SEED, 31, OUT) == ERR_PARAM, name
        assert f(0, 16, None, 32, None) == OK, name
        assert f(0, 0, None, 34, None) == OK, name
        assert f(1, 0, None, 34, OUT) == ERR_PARAM, name                     # NULL with count > 0
        assert f(1, 0, SEED, 34, None) == ERR_PARAM, name
        assert f(SMAX // 2048 + 1, 0, SEED, 34, OUT) == ERR_PARAM, name      # count * 256 * 8 overflows
        assert f(SMAX // (2048 * 256) + 1, 16, SEED, 32, OUT) == ERR_PARAM, name
        assert f(2, 0, SEED, SMAX // 2 + 1, OUT) == ERR_PARAM, name
        assert f(1, 0, OUT + 2047, 34, OUT) == ERR_PARAM, name               # the seed inside the output
        assert f(2, 2, OUT - 33, 32, OUT) == ERR_PARAM, name
    assert (buf == 7).all()


def _cbd_forms(L):
    def dev(count, eta, sigma, stride, first, per, out, io=64):
        return L.psf_sample_cbd_fips203_dev(0, count, eta, sigma, stride, first, per, out, io, None)

    def host(count, eta, sigma, stride, first, per, out, io=64):
        return L.psf_sample_cbd_fips203(0, count, eta, sigma, stride, first, per, out)
    return {"dev": dev, "host": host}


def test_sample_cbd_argument_errors_param_before_unsupported():
    L = _lib()
    buf = np.full(1 << 16, 7, dtype=np.uint8)
    SIG, OUT = buf.ctypes.data, buf.ctypes.data + 4096
    for name, f in _cbd_forms(L).items():
        assert f(1, 0, SIG, 32, 0, 1, OUT) == ERR_PARAM, name                # eta = 0
        assert f(0, 0, None, 32, 0, 1, None) == ERR_PARAM, name
        for first, per in ((0, 257), (256, 1), (1, 256), (255, 2), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF), (257, 0)):
            assert f(1, 2, SIG, 32, first, per, OUT) == ERR_PARAM, (name, first, per)
            assert f(1, 5, SIG, 32, first, per, OUT) == ERR_PARAM, (name, first, per)        # ... outranks the unsupported eta
        for eta in (1, 4, 5, 16, 0xFFFFFFFF):
            assert f(1, eta, SIG, 32, 0, 1, OUT) == ERR_UNSUPPORTED, (name, eta)
            assert f(0, eta, None, 32, 0, 1, None) == ERR_UNSUPPORTED, (name, eta)
            assert f(1, eta, None, 32, 0, 1, OUT) == ERR_PARAM, (name, eta)  # every PARAM check outranks it
            assert f(1, eta, SIG, 31, 0, 1, OUT) == ERR_PARAM, (name, eta)
        if name == "dev":
            for io in (0, 8, 32, -16):
                assert f(1, 2, SIG, 32, 0, 1, OUT, io) == ERR_PARAM, io
                assert f(1, 7, SIG, 32, 0, 1, OUT, io) == ERR_PARAM, io
            assert f(0, 3, None, 32, 0, 8, None, 16) == OK
        for eta in (2, 3):
            assert f(0, eta, None, 32, 0, 256, None) == OK, name
            assert f(0, eta, None, 32, 248, 8, None) == OK, name
            assert f(3, eta, SIG, 32, 7, 0, OUT) == OK, name                 # per_seed = 0: nothing to write
            assert f(1, eta, SIG, 31, 0, 1, OUT) == ERR_PARAM, name
            assert f(1, eta, None, 32, 0, 1, OUT) == ERR_PARAM, name
            assert f(1, eta, SIG, 32, 0, 1, None) == ERR_PARAM, name
            assert f(SMAX // 2048 + 1, eta, SIG, 32, 0, 1, OUT) == ERR_PARAM, name
            assert f(SMAX // 4096, eta, SIG, 32, 0, 4, OUT) == ERR_PARAM, name
            assert f(1, eta, OUT + 100, 32, 0, 1, OUT) == ERR_PARAM, name    # sigma inside the output
    assert (buf == 7).all()


def test_image_argument_errors():
    L = _lib()
    buf = np.full(1 << 14, 7, dtype=np.uint8)
    A, B = buf.ctypes.data, buf.ctypes.data + 8192
    for fn in (L.psf_ntt_image_from_fips203_dev, L.psf_ntt_image_to_fips203_dev):
        frm = fn is L.psf_ntt_image_from_fips203_dev

        def f(count, fhat, io, hat, fn=fn, frm=frm):
            return fn(0, count, fhat, io, hat, None) if frm else fn(0, count, hat, fhat, io, None)
        for io in (0, 8, 32, -64):
            assert f(1, A, io, B) == ERR_PARAM
            assert f(0, None, io, None) == ERR_PARAM
        for io in (16, 64):
            assert f(0, None, io, None) == OK
            assert f(1, None, io, B) == ERR_PARAM
            assert f(1, A, io, None) == ERR_PARAM
            assert f(SMAX // 2048 + 1, A, io, B) == ERR_PARAM
            assert f(1, A, io, A) == ERR_PARAM
            assert f(1, A, io, A + 256 * (io // 8) - 1) == ERR_PARAM
    assert L.psf_ntt_image_from_fips203(0, 1, None, B) == ERR_PARAM
    assert L.psf_ntt_image_to_fips203(0, 1, None, B) == ERR_PARAM
    assert L.psf_ntt_image_from_fips203(0, 0, None, None) == OK
    assert L.psf_ntt_image_to_fips203(0, 1, A, A + 1023) == ERR_PARAM
    assert (buf == 7).all()


def test_valid_calls_without_a_device_are_hip_errors():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    buf = np.full(1 << 14, 7, dtype=np.uint8)
    A, B = buf.ctypes.data, buf.ctypes.data + 8192
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        assert L.psf_keccak(dev, 3, 2, A, 33, 33, B, 128, 128) == ERR_HIP, dev
        assert L.psf_sample_ntt_fips203(dev, 1, 0, A, 34, B) == ERR_HIP, dev
        assert L.psf_sample_cbd_fips203(dev, 1, 2, A, 32, 0, 1, B) == ERR_HIP, dev
        assert L.psf_ntt_image_from_fips203(dev, 1, A, B) == ERR_HIP, dev
        assert L.psf_ntt_image_to_fips203(dev, 1, A, B) == ERR_HIP, dev
    assert (buf == 7).all()
    if not _have_device():
        import tools_amd as T
        F = T.fips203
        for call in (lambda: F.keccak(F.SHAKE256, [b"abc"], 16), lambda: F.sample_ntt(np.zeros((1, 34), np.uint8)),
                     lambda: F.sample_cbd(np.zeros((2, 32), np.uint8), 3, per_seed=2), lambda: F.image_from_fips203(np.zeros((2, 256), np.uint64)),
                     lambda: F.image_to_fips203(np.zeros(256, np.uint32))):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP
        for dcall in (lambda: F.keccak_dev(F.SHA3_256, 1, A, 5, B, 32), lambda: F.sample_ntt_dev(B, 1, A, k=2),
                      lambda: F.sample_cbd_dev(B, 1, A, 2), lambda: F.image_from_fips203_dev(B, 1, A), lambda: F.image_to_fips203_dev(B, 1, A)):
            with pytest.raises(T.PsfError) as ei:
                dcall()
            assert ei.value.status == ERR_HIP
