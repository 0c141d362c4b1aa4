"""No-GPU checks of the entry points of include/psf_mi355x.h for the SHA-2 parameter sets of SLH-DSA (psf_slhdsa_sha2_*) and for the batched hashes under
them (psf_sha2_dev, psf_sha2): every symbol exported and mirrored, the sizes against FIPS 205 Table 2, the workspace sizes, every argument error in its
stated order (all checked before the first HIP call, so the codes hold on any host) with the guard buffer unchanged, count = 0, and a valid call
without a device PSF_ERR_HIP.  The parameter numbering is these entry points' own: tools_amd.slhdsa_sha2.PARAM holds the six SHA-2 names, and a SHAKE
name is a ValueError.  The device results are compared with the model in tests/test_gpu_slhdsa_sha2.py and with hashlib in tests/test_gpu_sha2.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
SMAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
SYMBOLS = ("psf_slhdsa_sha2_sizes", "psf_slhdsa_sha2_workspace_bytes", "psf_slhdsa_sha2_keygen_dev", "psf_slhdsa_sha2_verify_dev", "psf_slhdsa_sha2_keygen",
           "psf_slhdsa_sha2_verify", "psf_sha2_dev", "psf_sha2")
# param: (n, h', k, pk, sk, sig)
SETS = {0: (16, 9, 14, 32, 64, 7856), 1: (16, 3, 33, 32, 64, 17088), 2: (24, 9, 17, 48, 96, 16224), 3: (24, 3, 33, 48, 96, 35664), 4: (32, 8, 22, 64, 128, 29792),
        5: (32, 4, 35, 64, 128, 49856)}
NAMES = ["SLH-DSA-SHA2-128s", "SLH-DSA-SHA2-128f", "SLH-DSA-SHA2-192s", "SLH-DSA-SHA2-192f", "SLH-DSA-SHA2-256s", "SLH-DSA-SHA2-256f"]
KEYGEN, VERIFY = 0, 1


def _lib():
    from tools_amd import slhdsa_sha2
    return slhdsa_sha2._lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _ws(L, param, count, op):
    out = C.c_size_t(0)
    assert L.psf_slhdsa_sha2_workspace_bytes(param, count, op, C.byref(out)) == OK
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
    for const in ("PSF_SLHDSA_SHA2_128S: psf_status = 0", "PSF_SLHDSA_SHA2_128F: psf_status = 1", "PSF_SLHDSA_SHA2_192S: psf_status = 2",
                  "PSF_SLHDSA_SHA2_192F: psf_status = 3", "PSF_SLHDSA_SHA2_256S: psf_status = 4", "PSF_SLHDSA_SHA2_256F: psf_status = 5",
                  "PSF_SLHDSA_OP_KEYGEN: psf_status = 0", "PSF_SLHDSA_OP_VERIFY: psf_status = 1", "PSF_SHA2_256: psf_status = 0", "PSF_SHA2_512: psf_status = 1"):
        assert const in ffi, const
    import tools_amd as T
    for name in ("sizes", "workspace_bytes", "keygen_dev", "verify_dev", "keygen_internal", "verify_internal", "keygen", "verify"):
        assert callable(getattr(T.slhdsa, name)), name
    assert T.slhdsa_sha2.PARAM == {n: i for i, n in enumerate(NAMES)}
    assert callable(T.sha2.sha2_dev) and callable(T.sha2.sha2)
    assert "SLH-DSA-SHA2-128s" not in T.slhdsa.PARAM and len(T.slhdsa.PARAM) == 6       # the SHAKE module keeps its own six


def test_sizes_against_the_table():
    L = _lib()
    import tools_amd as T
    for param, (n, hp, k, pk, sk, sig) in SETS.items():
        v = [C.c_size_t(0) for _ in range(3)]
        assert L.psf_slhdsa_sha2_sizes(param, *[C.byref(x) for x in v]) == OK
        assert tuple(x.value for x in v) == (pk, sk, sig)
        assert L.psf_slhdsa_sha2_sizes(param, None, None, None) == OK
        assert T.slhdsa_sha2.sizes(NAMES[param]) == {"pk": pk, "sk": sk, "sig": sig}
    for param in (-1, 6, 7, 44, 128, 1024):
        assert L.psf_slhdsa_sha2_sizes(param, None, None, None) == ERR_PARAM
    with pytest.raises(ValueError):
        T.slhdsa_sha2.sizes("SLH-DSA-SHAKE-128s")


def test_workspace_bytes_values_and_monotonicity():
    L = _lib()
    out = C.c_size_t(99)
    for param in (-1, 6, 45):
        assert L.psf_slhdsa_sha2_workspace_bytes(param, 1, KEYGEN, C.byref(out)) == ERR_PARAM
    for op in (-1, 2, 100):
        assert L.psf_slhdsa_sha2_workspace_bytes(1, 1, op, C.byref(out)) == ERR_PARAM
    assert L.psf_slhdsa_sha2_workspace_bytes(1, 1, KEYGEN, None) == ERR_PARAM
    assert L.psf_slhdsa_sha2_workspace_bytes(1, SMAX // 1024, VERIFY, C.byref(out)) == ERR_PARAM        # does not fit size_t
    assert L.psf_slhdsa_sha2_workspace_bytes(0, SMAX // 1024, KEYGEN, C.byref(out)) == ERR_PARAM
    assert out.value == 99
    for param, (n, hp, k, pk, sk, sig) in SETS.items():
        ln = 2 * n + 3
        for op in (KEYGEN, VERIFY):
            last = 0
            for count in (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 67, 255, 256, 259, 4096, 65536, (1 << 31) - 1):
                w = _ws(L, param, count, op)
                assert w % 256 == 0 and w >= last, (param, op, count)
                last = w
            assert _ws(L, param, 0, op) == 0
        # keygen: the chain ends and the leaves of the top tree; verify: 64 bytes of H_msg, the FORS roots, the node, the chain ends of one layer
        big = (1 << 31) - 1
        assert _ws(L, param, big, KEYGEN) >= big * ((ln + 1) * n << hp)
        assert _ws(L, param, big, KEYGEN) < (big + 1) * ((ln + 1) * n << hp) + 512
        assert _ws(L, param, big, VERIFY) >= big * (64 + k * n + 32 + ln * n)
        assert _ws(L, param, 1, KEYGEN) >= ((ln + 1) * n << hp) and _ws(L, param, 1, VERIFY) >= 64 + k * n + 32 + ln * n
    assert _ws(L, 4, (1 << 31) - 1, KEYGEN) > 1 << 50                      # no 32-bit or 48-bit product on the way


def _keygen_dev(L, param):
    return lambda c, a, b, s, pk, sk, w, wb: L.psf_slhdsa_sha2_keygen_dev(0, param, c, a, b, s, pk, sk, w, wb, None)


def _verify_dev(L, param, pk_len, msg_len=33, pk_stride=None, msg_stride=None):
    ps = pk_len if pk_stride is None else pk_stride
    ms = msg_len if msg_stride is None else msg_stride
    return lambda c, pk, msg, sig, ok, w, wb: L.psf_slhdsa_sha2_verify_dev(0, param, c, pk, ps, msg, msg_len, ms, sig, ok, w, wb, None)


@pytest.mark.parametrize("param", [1, 2, 5])
def test_argument_errors_in_order_and_nothing_written(param):
    L = _lib()
    count = 2
    n, hp, k, pk_len, sk_len, sig_len = SETS[param]
    wsb = max(_ws(L, param, count, op) for op in (KEYGEN, VERIFY))
    buf = np.full(wsb + (1 << 18), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256                              # the workspace first, 256-byte aligned
    P = WS + wsb
    msg_len = 33
    calls = {
        "keygen_dev": (_keygen_dev, (n, n, n, pk_len, sk_len), 3, KEYGEN, True),
        "verify_dev": (lambda L_, p: _verify_dev(L_, p, pk_len, msg_len), (pk_len, msg_len, sig_len, 1), 3, VERIFY, True),
        "keygen": (lambda L_, p: (lambda c, a, b, s, pk, sk, w=None, wb=0: L_.psf_slhdsa_sha2_keygen(0, p, c, a, b, s, pk, sk)), (n, n, n, pk_len, sk_len), 3, KEYGEN, False),
        "verify": (lambda L_, p: (lambda c, pk, msg, sig, ok, w=None, wb=0: L_.psf_slhdsa_sha2_verify(0, p, c, pk, pk_len, msg, msg_len, msg_len, sig, ok)),
                   (pk_len, msg_len, sig_len, 1), 3, VERIFY, False),
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
        for bad in (-1, 6, 44, 768):
            g = make(L, bad)
            assert call(count, ptrs, g=g) == ERR_PARAM, (name, bad)
            assert call(0, nul, w=None, wb=0, g=g) == ERR_PARAM, (name, bad)
        # count = 0: no work, no pointers, no workspace, no device
        assert call(0, nul, w=None, wb=0) == OK, name
        # 2. a NULL data pointer, before the strides, the byte counts, the workspace and the overlaps
        for i in range(len(ptrs)):
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
            assert call(SMAX // (1 << 17), ptrs) == ERR_PARAM, name           # the buffers fit, the workspace does not
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
            p = list(ptrs)
            p[1] = p[0]
            assert call(count, p) == ERR_HIP, name
    # verify: the strides (3.), each before the later classes
    ptrs, at = [], P
    for ln in (pk_len, 64, sig_len, 1):
        ptrs.append(at)
        at += count * ln + 64
    assert _verify_dev(L, param, pk_len, 64, pk_stride=pk_len - 1)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, 64, pk_stride=1)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, 64, msg_stride=63)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, 64, msg_stride=0)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _verify_dev(L, param, pk_len, 64, msg_stride=63)(SMAX // 16, *ptrs, None, 0) == ERR_PARAM      # the stride, before overflow and workspace
    assert _verify_dev(L, param, pk_len, SMAX - 8, msg_stride=SMAX)(1, *ptrs, WS, wsb) == ERR_PARAM        # 3 n + msg_len does not fit
    # a NULL pointer comes before a bad stride
    p = list(ptrs)
    p[2] = None
    assert _verify_dev(L, param, pk_len, 64, pk_stride=1)(count, *p, WS, wsb) == ERR_PARAM
    # more than 2^31 - 1 instances: unsupported, after every other check (a workspace of that size is only claimed, never touched)
    big = 1 << 31
    need = _ws(L, param, big, VERIFY)
    far = [1 << 60, 1 << 61, (1 << 61) + (1 << 59), 1 << 62]
    assert _verify_dev(L, param, pk_len, 64)(big, *far, 256, need) == ERR_UNSUPPORTED
    assert _verify_dev(L, param, pk_len, 64)(big, *far, 256, need - 1) == ERR_PARAM
    kfar = [1 << 60, (1 << 60) + (1 << 40), (1 << 60) + (1 << 41), 1 << 61, 1 << 62]
    assert L.psf_slhdsa_sha2_keygen_dev(0, param, big, *kfar, 256, _ws(L, param, big, KEYGEN), None) == ERR_UNSUPPORTED
    if not _have_device():
        # valid forms: one key for all, wider strides, an empty message without a pointer
        assert _verify_dev(L, param, pk_len, 64, pk_stride=0)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _verify_dev(L, param, pk_len, 64, pk_stride=pk_len + 5, msg_stride=70)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _verify_dev(L, param, pk_len, 0)(count, ptrs[0], None, *ptrs[2:], WS, wsb) == ERR_HIP
    assert (buf == 7).all()


def test_valid_calls_without_a_device_are_hip_errors():
    """no CPU fallback: a valid call on a device that does not exist returns PSF_ERR_HIP (device 0 on a host without a GPU)"""
    L = _lib()
    param, count = 3, 2
    n, hp, k, pk_len, sk_len, sig_len = SETS[param]
    wsb = max(_ws(L, param, count, op) for op in (KEYGEN, VERIFY))
    buf = np.full(wsb + (1 << 18), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256
    A = WS + wsb
    B, Cc, S, O1, O2 = A + 1000, A + 2000, A + 4000, A + 100000, A + 110000
    for dev in [-1, 4096] + ([] if _have_device() else [0]):
        assert L.psf_slhdsa_sha2_keygen_dev(dev, param, count, A, B, Cc, O1, O2, WS, wsb, None) == ERR_HIP, dev
        assert L.psf_slhdsa_sha2_verify_dev(dev, param, count, A, pk_len, B, 20, 20, S, O1, WS, wsb, None) == ERR_HIP, dev
        assert L.psf_slhdsa_sha2_keygen(dev, param, count, A, B, Cc, O1, O2) == ERR_HIP, dev
        assert L.psf_slhdsa_sha2_verify(dev, param, count, A, 0, B, 64, 64, S, O1) == ERR_HIP, dev
    assert (buf == 7).all()
    if not _have_device():
        import tools_amd as T
        D = T.slhdsa_sha2
        for call in (lambda: D.keygen_internal(NAMES[1], [bytes(16)], [bytes(16)], [bytes(16)]), lambda: D.keygen(NAMES[5], 2),
                     lambda: D.verify_internal(NAMES[2], bytes(48), [b"m"], [bytes(16224)]), lambda: D.verify(NAMES[1], bytes(32), b"msg", bytes(17088), ctx=b"c")):
            with pytest.raises(T.PsfError) as ei:
                call()
            assert ei.value.status == ERR_HIP
    import tools_amd as T
    with pytest.raises(ValueError):
        T.slhdsa_sha2.verify(NAMES[1], bytes(32), b"msg", bytes(17088), ctx=bytes(256))
    with pytest.raises(ValueError):
        T.slhdsa_sha2.verify_internal(NAMES[2], bytes(47), [b"m"], [bytes(16224)])


# ---- psf_sha2_dev / psf_sha2 ------------------------------------------------------------------------------------------------------------------------------

def _sha2_calls(L):
    return {"sha2_dev": lambda f, c, i, il, is_, o, ol, os_: L.psf_sha2_dev(0, f, c, i, il, is_, o, ol, os_, None),
            "sha2": lambda f, c, i, il, is_, o, ol, os_: L.psf_sha2(0, f, c, i, il, is_, o, ol, os_)}


def test_sha2_argument_errors_in_order_and_nothing_written():
    import tools_amd as T
    L = T.sha2._lib()
    buf = np.full(1 << 16, 7, dtype=np.uint8)
    IN, OUT = buf.ctypes.data + 64, buf.ctypes.data + 32768
    count = 3
    for name, f in _sha2_calls(L).items():
        # 1. unknown func first of all, even with count = 0 and NULL pointers
        for func in (-1, 2, 3, 44):
            assert f(func, count, IN, 64, 64, OUT, 32, 32) == ERR_PARAM, (name, func)
            assert f(func, 0, None, 0, 0, None, 32, 32) == ERR_PARAM, (name, func)
        # 2. the wrong out_len: 0, or above the digest size
        for func, size in ((0, 32), (1, 64)):
            for out_len in (0, size + 1, 65, 1000):
                assert f(func, count, IN, 64, 64, OUT, out_len, out_len) == ERR_PARAM, (name, func, out_len)
                assert f(func, 0, None, 0, 0, None, out_len, out_len) == ERR_PARAM, (name, func, out_len)
            # 3. a stride smaller than its length, before the NULL pointers
            assert f(func, count, IN, 64, 63, OUT, size, size) == ERR_PARAM, (name, func)
            assert f(func, count, IN, 64, 64, OUT, size, size - 1) == ERR_PARAM, (name, func)
            assert f(func, 0, None, 64, 63, None, size, size) == ERR_PARAM, (name, func)
            # count = 0: no work, no pointers, no device
            assert f(func, 0, None, 64, 64, None, size, size) == OK, (name, func)
            # 4. a NULL pointer with count > 0; the input may be NULL only when in_len = 0
            assert f(func, count, None, 64, 64, OUT, size, size) == ERR_PARAM, (name, func)
            assert f(func, count, IN, 64, 64, None, size, size) == ERR_PARAM, (name, func)
            assert f(func, count, None, 0, 0, None, size, size) == ERR_PARAM, (name, func)
            # 5. a byte count that overflows size_t
            assert f(func, SMAX // 32, IN, 64, 64, OUT, size, size) == ERR_PARAM, (name, func)
            assert f(func, 2, IN, SMAX - 4, SMAX - 4, OUT, size, size) == ERR_PARAM, (name, func)
            # 6. an output range that overlaps the input range
            assert f(func, count, IN, 64, 64, IN + 3 * 64 - 1, size, size) == ERR_PARAM, (name, func)
            assert f(func, count, IN, 64, 64, IN - 3 * size + 1, size, size) == ERR_PARAM, (name, func)
            assert f(func, count, IN, 64, 100, IN + 64, 16, 100) == ERR_PARAM, (name, func)                # interleaved rows still overlap as ranges
            # valid calls without a device: HIP errors, for every out_len 1 ... size, padded strides and the empty message without a pointer
            if not _have_device():
                for out_len in (1, 16, 24, size):
                    assert f(func, count, IN, 64, 64, OUT, out_len, out_len) == ERR_HIP, (name, func, out_len)
                assert f(func, count, IN, 65, 71, OUT, size, size + 5) == ERR_HIP, (name, func)
                assert f(func, count, None, 0, 0, OUT, size, size) == ERR_HIP, (name, func)
    for dev in (-1, 4096):
        assert L.psf_sha2_dev(dev, 0, count, IN, 64, 64, OUT, 32, 32, None) == ERR_HIP
        assert L.psf_sha2(dev, 1, count, IN, 64, 64, OUT, 64, 64) == ERR_HIP
    assert (buf == 7).all()
    with pytest.raises(ValueError):
        T.sha2.sha2(0, [b"ab", b"abc"])
