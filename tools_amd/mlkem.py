"""ML-KEM (FIPS 203) on the device, batched, through the C ABI (psf_mlkem_*, include/psf_mi355x.h): bytes in, bytes out.

  sizes / workspace_bytes   the byte sizes of a parameter set and of the workspace of an operation
  keygen_dev / encaps_dev / decaps_dev   ML-KEM.KeyGen_internal, Encaps_internal and Decaps_internal (Algorithms 16 to 18) over raw device
               pointers (e.g. torch `data_ptr()`), ordered on `stream`, nothing allocated; the caller supplies d, z and m and the workspace
  check_ek_dev / check_dk_dev   the modulus check of section 7.2 and the hash check of section 7.3, one byte per instance
  keygen_internal / encaps_internal / decaps / check_ek / check_dk   the host forms over lists of bytes (they run on the device too)
  keygen / encaps   ML-KEM.KeyGen and ML-KEM.Encaps (Algorithms 19 and 20): the two that draw randomness, here from os.urandom.  They exist in
               Python only; the library itself draws none.

Instance c of every buffer is at base + c * size; a parameter set is named "ML-KEM-512", "ML-KEM-768" or "ML-KEM-1024"."""
import ctypes as C
import os

import numpy as np

from ._ffi import _rows, _vp, check, lib

PARAM = {"ML-KEM-512": 2, "ML-KEM-768": 3, "ML-KEM-1024": 4}
OP_KEYGEN, OP_ENCAPS, OP_DECAPS, OP_CHECK = range(4)
OPS = {"keygen": OP_KEYGEN, "encaps": OP_ENCAPS, "decaps": OP_DECAPS, "check": OP_CHECK}

_typed = False


def _lib():
    global _typed
    L = lib()
    if not _typed:
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        L.psf_mlkem_sizes.argtypes = [i] + [C.POINTER(sz)] * 4
        L.psf_mlkem_workspace_bytes.argtypes = [i, sz, i, C.POINTER(sz)]
        L.psf_mlkem_keygen_dev.argtypes = [i, i, sz, vp, vp, vp, vp, vp, sz, vp, vp]
        L.psf_mlkem_encaps_dev.argtypes = [i, i, sz, vp, vp, vp, vp, vp, sz, vp, vp]
        L.psf_mlkem_decaps_dev.argtypes = [i, i, sz, vp, vp, vp, vp, sz, vp, vp]
        L.psf_mlkem_check_ek_dev.argtypes = [i, i, sz, vp, vp, vp]
        L.psf_mlkem_check_dk_dev.argtypes = [i, i, sz, vp, vp, vp]
        L.psf_mlkem_keygen.argtypes = [i, i, sz, vp, vp, vp, vp]
        L.psf_mlkem_encaps.argtypes = [i, i, sz, vp, vp, vp, vp]
        L.psf_mlkem_decaps.argtypes = [i, i, sz, vp, vp, vp]
        L.psf_mlkem_check_ek.argtypes = [i, i, sz, vp, vp]
        L.psf_mlkem_check_dk.argtypes = [i, i, sz, vp, vp]
        _typed = True
    return L


def _param(name):
    if name in PARAM:
        return PARAM[name]
    if name in PARAM.values():
        return name
    raise ValueError(f"unknown ML-KEM parameter set {name!r}")


def sizes(name):
    """{"ek": ..., "dk": ..., "ct": ..., "ss": 32} in bytes"""
    v = [C.c_size_t(0) for _ in range(4)]
    check(_lib().psf_mlkem_sizes(_param(name), *[C.byref(x) for x in v]), "mlkem.sizes")
    return dict(zip(("ek", "dk", "ct", "ss"), (int(x.value) for x in v)))


def workspace_bytes(name, count, op):
    """bytes of the 256-byte aligned device workspace that `op` ("keygen", "encaps", "decaps", "check") needs for `count` instances"""
    out = C.c_size_t(0)
    check(_lib().psf_mlkem_workspace_bytes(_param(name), count, OPS[op] if op in OPS else op, C.byref(out)), "mlkem.workspace_bytes")
    return int(out.value)


def keygen_dev(name, count, d_d, d_z, d_ek, d_dk, d_ws, ws_bytes, d_fail=None, device=0, stream=None):
    """psf_mlkem_keygen_dev: (ek_c, dk_c) = ML-KEM.KeyGen_internal(d_c, z_c)"""
    check(_lib().psf_mlkem_keygen_dev(device, _param(name), count, d_d or 0, d_z or 0, d_ek or 0, d_dk or 0, d_ws or 0, ws_bytes, d_fail or 0, stream or 0),
          "mlkem.keygen_dev")


def encaps_dev(name, count, d_ek, d_m, d_ss, d_ct, d_ws, ws_bytes, d_fail=None, device=0, stream=None):
    """psf_mlkem_encaps_dev: (K_c, c_c) = ML-KEM.Encaps_internal(ek_c, m_c)"""
    check(_lib().psf_mlkem_encaps_dev(device, _param(name), count, d_ek or 0, d_m or 0, d_ss or 0, d_ct or 0, d_ws or 0, ws_bytes, d_fail or 0, stream or 0),
          "mlkem.encaps_dev")


def decaps_dev(name, count, d_dk, d_ct, d_ss, d_ws, ws_bytes, d_fail=None, device=0, stream=None):
    """psf_mlkem_decaps_dev: K_c = ML-KEM.Decaps_internal(dk_c, c_c)"""
    check(_lib().psf_mlkem_decaps_dev(device, _param(name), count, d_dk or 0, d_ct or 0, d_ss or 0, d_ws or 0, ws_bytes, d_fail or 0, stream or 0),
          "mlkem.decaps_dev")


def check_ek_dev(name, count, d_ek, d_ok, device=0, stream=None):
    """psf_mlkem_check_ek_dev: ok[c] = 1 when every 12-bit field of ek_c is below q, else 0"""
    check(_lib().psf_mlkem_check_ek_dev(device, _param(name), count, d_ek or 0, d_ok or 0, stream or 0), "mlkem.check_ek_dev")


def check_dk_dev(name, count, d_dk, d_ok, device=0, stream=None):
    """psf_mlkem_check_dk_dev: ok[c] = 1 when H of the embedded ek equals the embedded hash, else 0"""
    check(_lib().psf_mlkem_check_dk_dev(device, _param(name), count, d_dk or 0, d_ok or 0, stream or 0), "mlkem.check_dk_dev")


# ---- host forms ------------------------------------------------------------------------------------------------------------------------------------

def _split(a):
    return [bytes(r) for r in a]


def keygen_internal(name, ds, zs, device=0):
    """[(ek, dk)] for the 32-byte seeds d and z of each instance"""
    sz = sizes(name)
    d, z = _rows(ds, 32, "d", "mlkem"), _rows(zs, 32, "z", "mlkem")
    if len(d) != len(z):
        raise ValueError("mlkem.keygen_internal: as many d as z")
    ek, dk = np.empty((len(d), sz["ek"]), np.uint8), np.empty((len(d), sz["dk"]), np.uint8)
    check(_lib().psf_mlkem_keygen(device, _param(name), len(d), _vp(d), _vp(z), _vp(ek), _vp(dk)), "mlkem.keygen_internal")
    return list(zip(_split(ek), _split(dk)))


def encaps_internal(name, eks, ms, device=0):
    """[(K, c)] for each encapsulation key and 32-byte m.  No input check: see encaps."""
    sz = sizes(name)
    ek, m = _rows(eks, sz["ek"], "ek", "mlkem"), _rows(ms, 32, "m", "mlkem")
    if len(ek) != len(m):
        raise ValueError("mlkem.encaps_internal: as many ek as m")
    ss, ct = np.empty((len(ek), 32), np.uint8), np.empty((len(ek), sz["ct"]), np.uint8)
    check(_lib().psf_mlkem_encaps(device, _param(name), len(ek), _vp(ek), _vp(m), _vp(ss), _vp(ct)), "mlkem.encaps_internal")
    return list(zip(_split(ss), _split(ct)))


def decaps(name, dks, cts, device=0):
    """[K] = ML-KEM.Decaps_internal for each decapsulation key and ciphertext.  check_dk is the caller's to run once per key."""
    sz = sizes(name)
    dk, ct = _rows(dks, sz["dk"], "dk", "mlkem"), _rows(cts, sz["ct"], "ciphertext", "mlkem")
    if len(dk) != len(ct):
        raise ValueError("mlkem.decaps: as many dk as ciphertexts")
    ss = np.empty((len(dk), 32), np.uint8)
    check(_lib().psf_mlkem_decaps(device, _param(name), len(dk), _vp(dk), _vp(ct), _vp(ss)), "mlkem.decaps")
    return _split(ss)


def check_ek(name, eks, device=0):
    """[bool]: the modulus check of section 7.2"""
    ek = _rows(eks, sizes(name)["ek"], "ek", "mlkem")
    ok = np.zeros(len(ek), np.uint8)
    check(_lib().psf_mlkem_check_ek(device, _param(name), len(ek), _vp(ek), _vp(ok)), "mlkem.check_ek")
    return [bool(v) for v in ok]


def check_dk(name, dks, device=0):
    """[bool]: the hash check of section 7.3"""
    dk = _rows(dks, sizes(name)["dk"], "dk", "mlkem")
    ok = np.zeros(len(dk), np.uint8)
    check(_lib().psf_mlkem_check_dk(device, _param(name), len(dk), _vp(dk), _vp(ok)), "mlkem.check_dk")
    return [bool(v) for v in ok]


# ---- Algorithms 19 and 20: the randomised forms, in Python only ------------------------------------------------------------------------------------

def keygen(name, count, device=0, random=os.urandom):
    """ML-KEM.KeyGen for `count` fresh key pairs: d and z from `random` (os.urandom), then keygen_internal"""
    return keygen_internal(name, [random(32) for _ in range(count)], [random(32) for _ in range(count)], device=device)


def encaps(name, eks, device=0, random=os.urandom):
    """ML-KEM.Encaps: the modulus check on every key (ValueError if one fails), m from `random` (os.urandom), then encaps_internal"""
    eks = list(eks)
    bad = [c for c, ok in enumerate(check_ek(name, eks, device=device)) if not ok]
    if bad:
        raise ValueError(f"mlkem.encaps: encapsulation keys {bad} fail the modulus check")
    return encaps_internal(name, eks, [random(32) for _ in range(len(eks))], device=device)
