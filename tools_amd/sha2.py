"""SHA-256 and SHA-512 (FIPS 180-4) on the device, batched, through the C ABI (psf_sha2_dev / psf_sha2, include/psf_mi355x.h): one hash state per lane,
equally long messages, the leading out_len bytes of every digest -- the twin of fips203.keccak_dev / keccak for the hashes the SHA-2 parameter sets of
SLH-DSA (tools_amd.slhdsa_sha2) are built on."""
import ctypes as C

import numpy as np

from ._ffi import _vp, check, lib

SHA2_256, SHA2_512 = range(2)
DIGEST_BYTES = {SHA2_256: 32, SHA2_512: 64}

_typed = False


def _lib():
    global _typed
    L = lib()
    if not _typed:
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        L.psf_sha2_dev.argtypes = [i, i, sz, vp, sz, sz, vp, sz, sz, vp]
        L.psf_sha2.argtypes = [i, i, sz, vp, sz, sz, vp, sz, sz]
        _typed = True
    return L


def sha2_dev(func, count, d_in, in_len, d_out, out_len, in_stride=None, out_stride=None, device=0, stream=None):
    """psf_sha2_dev: message c at d_in + c * in_stride (in_len bytes), the first out_len bytes of digest c at d_out + c * out_stride; strides default
    to the lengths."""
    check(_lib().psf_sha2_dev(device, func, count, d_in or 0, in_len, in_len if in_stride is None else in_stride, d_out or 0, out_len,
                              out_len if out_stride is None else out_stride, stream or 0), "sha2_dev")


def sha2(func, messages, out_len=None, device=0):
    """digests of a batch of equally long messages: `messages` is a uint8 array (count, in_len) or a list of bytes; returns uint8 (count, out_len),
    out_len defaulting to the whole digest"""
    if not isinstance(messages, np.ndarray):
        lens = {len(m) for m in messages}
        if len(lens) > 1:
            raise ValueError("sha2: the messages of one batch have one length")
        messages = np.frombuffer(b"".join(bytes(m) for m in messages), dtype=np.uint8).reshape(len(messages), lens.pop() if lens else 0)
    msg = np.ascontiguousarray(messages, dtype=np.uint8)
    count, in_len = msg.shape
    if out_len is None:
        out_len = DIGEST_BYTES.get(func, 0)
    out = np.empty((count, out_len), dtype=np.uint8)
    check(_lib().psf_sha2(device, func, count, _vp(msg), in_len, in_len, _vp(out), out_len, out_len), "sha2")
    return out
