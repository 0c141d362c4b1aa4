"""The stages of ML-DSA, byte for byte as FIPS 204 defines them, through the C ABI (psf_sample_*_fips204*, psf_ntt_image_from_fips204*,
include/psf_mi355x.h):

  sample_ntt      RejNTTPoly (Algorithm 30): raw 34-byte inputs, or the k x l matrix A_hat of a 32-byte rho (ExpandA)
  sample_bounded  RejBoundedPoly (Algorithm 31) for a run of nonces per 64-byte seed (ExpandS)
  sample_in_ball  SampleInBall (Algorithm 29)
  image_from      FIPS 204's NTT-domain order -> the images of the *_hat_dev products at q = 8380417, n = 256

64-bit words throughout.  The *_dev forms take raw device pointers (e.g. torch `data_ptr()`), run in `stream` and allocate nothing; the host forms
take numpy arrays and run on the device too."""
import ctypes as C

import numpy as np

from ._ffi import _vp, check, lib

Q, N = 8380417, 256
_typed = False


def _lib():
    global _typed
    L = lib()
    if not _typed:
        vp, sz, u32, i = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
        L.psf_sample_ntt_fips204_dev.argtypes = [i, sz, u32, u32, vp, sz, vp, vp, vp]
        L.psf_sample_ntt_fips204.argtypes = [i, sz, u32, u32, vp, sz, vp]
        L.psf_sample_bounded_fips204_dev.argtypes = [i, sz, u32, vp, sz, u32, u32, vp, vp, vp]
        L.psf_sample_bounded_fips204.argtypes = [i, sz, u32, vp, sz, u32, u32, vp]
        L.psf_sample_in_ball_fips204_dev.argtypes = [i, sz, u32, vp, sz, sz, vp, vp, vp]
        L.psf_sample_in_ball_fips204.argtypes = [i, sz, u32, vp, sz, sz, vp]
        L.psf_ntt_image_from_fips204_dev.argtypes = [i, sz, vp, vp, vp]
        L.psf_ntt_image_from_fips204.argtypes = [i, sz, vp, vp]
        _typed = True
    return L


def sample_ntt_dev(d_out, count, d_seed, k=0, l=0, seed_stride=None, d_fail=None, device=0, stream=None):
    """psf_sample_ntt_fips204_dev.  k = l = 0: `count` inputs of 34 bytes, one polynomial each.  Otherwise `count` seeds rho of 32 bytes and count k l
    polynomials, (c, r, s) = RejNTTPoly(rho_c || s || r) = A_hat[r][s].  uint64 words in [0, q)."""
    if seed_stride is None:
        seed_stride = 32 if k else 34
    check(_lib().psf_sample_ntt_fips204_dev(device, count, k, l, d_seed or 0, seed_stride, d_out or 0, d_fail or 0, stream or 0), "fips204.sample_ntt_dev")


def sample_ntt(seeds, k=0, l=0, device=0):
    """host form: `seeds` uint8 (count, 34) for k = 0 or (count, 32) for the matrix form; returns uint64 (count, 256) or (count, k, l, 256)"""
    sd = np.ascontiguousarray(seeds, dtype=np.uint8)
    if sd.ndim != 2 or sd.shape[1] != (32 if k else 34):
        raise ValueError(f"fips204.sample_ntt: seeds of shape {sd.shape}")
    out = np.empty((sd.shape[0], k, l, N) if k else (sd.shape[0], N), dtype=np.uint64)
    check(_lib().psf_sample_ntt_fips204(device, sd.shape[0], k, l, _vp(sd), sd.shape[1], _vp(out)), "fips204.sample_ntt")
    return out


def sample_bounded_dev(d_out, count, d_seed, eta, first_nonce=0, per_seed=1, seed_stride=64, d_fail=None, device=0, stream=None):
    """psf_sample_bounded_fips204_dev: polynomial (c, t) = RejBoundedPoly(seed_c || le16(first_nonce + t)) for t < per_seed; int64 words in
    [-eta, eta]; eta = 2 or 4."""
    check(_lib().psf_sample_bounded_fips204_dev(device, count, eta, d_seed or 0, seed_stride, first_nonce, per_seed, d_out or 0, d_fail or 0, stream or 0),
          "fips204.sample_bounded_dev")


def sample_bounded(seeds, eta, first_nonce=0, per_seed=1, device=0):
    """host form: `seeds` uint8 (count, 64); returns int64 (count, per_seed, 256)"""
    sd = np.ascontiguousarray(seeds, dtype=np.uint8)
    if sd.ndim != 2 or sd.shape[1] != 64:
        raise ValueError(f"fips204.sample_bounded: seeds of shape {sd.shape}")
    out = np.empty((sd.shape[0], per_seed, N), dtype=np.int64)
    check(_lib().psf_sample_bounded_fips204(device, sd.shape[0], eta, _vp(sd), 64, first_nonce, per_seed, _vp(out)), "fips204.sample_bounded")
    return out


def sample_in_ball_dev(d_out, count, d_ctilde, tau, ctilde_len, ctilde_stride=None, d_fail=None, device=0, stream=None):
    """psf_sample_in_ball_fips204_dev: polynomial c = SampleInBall(the ctilde_len bytes of instance c); int64 words in {-1, 0, 1}, tau of them non-zero"""
    check(_lib().psf_sample_in_ball_fips204_dev(device, count, tau, d_ctilde or 0, ctilde_len, ctilde_len if ctilde_stride is None else ctilde_stride, d_out or 0,
                                                d_fail or 0, stream or 0), "fips204.sample_in_ball_dev")


def sample_in_ball(ctildes, tau, device=0):
    """host form: `ctildes` uint8 (count, len); returns int64 (count, 256)"""
    ct = np.ascontiguousarray(ctildes, dtype=np.uint8)
    if ct.ndim != 2:
        raise ValueError(f"fips204.sample_in_ball: inputs of shape {ct.shape}")
    out = np.empty((ct.shape[0], N), dtype=np.int64)
    check(_lib().psf_sample_in_ball_fips204(device, ct.shape[0], tau, _vp(ct), ct.shape[1], ct.shape[1], _vp(out)), "fips204.sample_in_ball")
    return out


def image_from_fips204_dev(d_hat, count, d_fhat, device=0, stream=None):
    """psf_ntt_image_from_fips204_dev: `count` polynomials as Algorithm 41 leaves them (uint64 of any value) -> images (count * 256 uint32) for
    poly_mul_hat_dev / matpoly_mul_hat_dev / matpoly_mul_add_hat_dev at (8380417, 256)"""
    check(_lib().psf_ntt_image_from_fips204_dev(device, count, d_fhat or 0, d_hat or 0, stream or 0), "fips204.image_from_fips204_dev")


def image_from_fips204(fhat, device=0):
    """host form: uint64 (..., 256) -> uint32 images of the same shape"""
    f = np.ascontiguousarray(fhat, dtype=np.uint64)
    if f.ndim < 1 or f.shape[-1] != N:
        raise ValueError(f"fips204.image_from_fips204: shape {f.shape}")
    hat = np.empty(f.shape, dtype=np.uint32)
    check(_lib().psf_ntt_image_from_fips204(device, f.size // N, _vp(f), _vp(hat)), "fips204.image_from_fips204")
    return hat
