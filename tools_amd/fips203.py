"""What an ML-KEM implementation needs beyond the ring arithmetic, byte for byte as FIPS 203 defines it, through the C ABI (psf_keccak*,
psf_sample_*_fips203*, psf_ntt_image_*_fips203*, include/psf_mi355x.h):

  keccak       SHA3-256 (H), SHA3-512 (G), SHAKE128 (XOF), SHAKE256 (J, PRF) over a batch of messages of one length, one Keccak state per lane
  sample_ntt   SampleNTT (Algorithm 7): raw 34-byte inputs, or the k x k matrix A_hat of a 32-byte rho
  sample_cbd   SamplePolyCBD_eta(PRF_eta(sigma, N)) (Algorithm 8) for a run of nonces N per seed
  image_from / image_to   FIPS 203's NTT-domain representation <-> the images of gadget.ntt_forward_dev at q = 3329, n = 256, so that A_hat,
               t_hat and s_hat cross the boundary in both directions

The *_dev forms take raw device pointers (e.g. torch `data_ptr()`), run in `stream` and allocate nothing; the host forms take numpy arrays and
bytes and run on the device too.  Everything computes on the GPU."""
import ctypes as C

import numpy as np

from ._ffi import _vp, check, lib

SHA3_256, SHA3_512, SHAKE128, SHAKE256 = range(4)
Q, N = 3329, 256


def keccak_dev(func, count, d_in, in_len, d_out, out_len, in_stride=None, out_stride=None, device=0, stream=None):
    """psf_keccak_dev: message c at d_in + c * in_stride (in_len bytes), digest c at d_out + c * out_stride (out_len bytes); strides default to
    the lengths."""
    check(lib().psf_keccak_dev(device, func, count, d_in or 0, in_len, in_len if in_stride is None else in_stride, d_out or 0, out_len,
                               out_len if out_stride is None else out_stride, stream or 0), "keccak_dev")


def keccak(func, messages, out_len, device=0):
    """digests of a batch of equally long messages: `messages` is a uint8 array (count, in_len) or a list of bytes; returns uint8 (count, out_len)"""
    if not isinstance(messages, np.ndarray):
        lens = {len(m) for m in messages}
        if len(lens) > 1:
            raise ValueError("keccak: the messages of one batch have one length")
        messages = np.frombuffer(b"".join(bytes(m) for m in messages), dtype=np.uint8).reshape(len(messages), lens.pop() if lens else 0)
    msg = np.ascontiguousarray(messages, dtype=np.uint8)
    count, in_len = msg.shape
    out = np.empty((count, out_len), dtype=np.uint8)
    check(lib().psf_keccak(device, func, count, _vp(msg), in_len, in_len, _vp(out), out_len, out_len), "keccak")
    return out


def sample_ntt_dev(d_out, count, d_seed, k=0, seed_stride=None, d_fail=None, io_bits=64, device=0, stream=None):
    """psf_sample_ntt_fips203_dev.  k = 0: `count` inputs of 34 bytes, one polynomial each.  1 <= k <= 16: `count` seeds rho of 32 bytes, count k k
    polynomials, (c, i, j) = SampleNTT(rho_c || j || i) = A_hat[i][j].  uint64 or uint16 (io_bits 16) words in [0, q).  d_fail: a device int
    (or None) OR-ed with 1 if a polynomial reached the cap of 8 SHAKE128 blocks."""
    if seed_stride is None:
        seed_stride = 32 if k else 34
    check(lib().psf_sample_ntt_fips203_dev(device, count, k, d_seed or 0, seed_stride, d_out or 0, d_fail or 0, io_bits, stream or 0), "sample_ntt_dev")


def sample_ntt(seeds, k=0, device=0):
    """host form: `seeds` uint8 (count, 34) for k = 0 or (count, 32) for the matrix form; returns uint64 (count, 256) or (count, k, k, 256)"""
    sd = np.ascontiguousarray(seeds, dtype=np.uint8)
    if sd.ndim != 2 or sd.shape[1] != (32 if k else 34):
        raise ValueError(f"sample_ntt: seeds of shape {sd.shape}")
    count = sd.shape[0]
    out = np.empty((count, k, k, N) if k else (count, N), dtype=np.uint64)
    check(lib().psf_sample_ntt_fips203(device, count, k, _vp(sd), sd.shape[1], _vp(out)), "sample_ntt")
    return out


def sample_cbd_dev(d_out, count, d_sigma, eta, first_nonce=0, per_seed=1, sigma_stride=32, io_bits=64, device=0, stream=None):
    """psf_sample_cbd_fips203_dev: polynomial (c, t) = SamplePolyCBD_eta(PRF_eta(sigma_c, first_nonce + t)) for t < per_seed; int64 or int16
    (io_bits 16) words in [-eta, eta]; eta = 2 or 3."""
    check(lib().psf_sample_cbd_fips203_dev(device, count, eta, d_sigma or 0, sigma_stride, first_nonce, per_seed, d_out or 0, io_bits, stream or 0),
          "sample_cbd_dev")


def sample_cbd(sigmas, eta, first_nonce=0, per_seed=1, device=0):
    """host form: `sigmas` uint8 (count, 32); returns int64 (count, per_seed, 256)"""
    sg = np.ascontiguousarray(sigmas, dtype=np.uint8)
    if sg.ndim != 2 or sg.shape[1] != 32:
        raise ValueError(f"sample_cbd: seeds of shape {sg.shape}")
    out = np.empty((sg.shape[0], per_seed, N), dtype=np.int64)
    check(lib().psf_sample_cbd_fips203(device, sg.shape[0], eta, _vp(sg), 32, first_nonce, per_seed, _vp(out)), "sample_cbd")
    return out


def image_from_fips203_dev(d_hat, count, d_fhat, io_bits=64, device=0, stream=None):
    """psf_ntt_image_from_fips203_dev: `count` polynomials in FIPS 203's NTT representation (uint64 of any value, or uint16 in [0, q)) -> images
    (count * 256 uint32) for poly_mul_hat_dev / matpoly_mul_hat_dev / matpoly_mul_add_hat_dev at (3329, 256)"""
    check(lib().psf_ntt_image_from_fips203_dev(device, count, d_fhat or 0, io_bits, d_hat or 0, stream or 0), "image_from_fips203_dev")


def image_to_fips203_dev(d_fhat, count, d_hat, io_bits=64, device=0, stream=None):
    """psf_ntt_image_to_fips203_dev: images (of ntt_forward_dev or image_from_fips203_dev) -> canonical residues in FIPS 203's NTT representation"""
    check(lib().psf_ntt_image_to_fips203_dev(device, count, d_hat or 0, d_fhat or 0, io_bits, stream or 0), "image_to_fips203_dev")


def image_from_fips203(fhat, device=0):
    """host form: uint64 (..., 256) -> uint32 images of the same shape"""
    f = np.ascontiguousarray(fhat, dtype=np.uint64)
    if f.ndim < 1 or f.shape[-1] != N:
        raise ValueError(f"image_from_fips203: shape {f.shape}")
    hat = np.empty(f.shape, dtype=np.uint32)
    check(lib().psf_ntt_image_from_fips203(device, f.size // N, _vp(f), _vp(hat)), "image_from_fips203")
    return hat


def image_to_fips203(hat, device=0):
    """host form: uint32 images (..., 256) -> uint64 residues in [0, q) of the same shape"""
    h = np.ascontiguousarray(hat, dtype=np.uint32)
    if h.ndim < 1 or h.shape[-1] != N:
        raise ValueError(f"image_to_fips203: shape {h.shape}")
    f = np.empty(h.shape, dtype=np.uint64)
    check(lib().psf_ntt_image_to_fips203(device, h.size // N, _vp(h), _vp(f)), "image_to_fips203")
    return f
