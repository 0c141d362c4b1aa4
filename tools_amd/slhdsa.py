"""SLH-DSA (FIPS 205, August 2024) on the device, batched, through the C ABI (psf_slhdsa_*, include/psf_mi355x.h): bytes in, bytes out, the six SHAKE
parameter sets.

  sizes / workspace_bytes   the byte sizes of a parameter set and of the workspace of an operation
  keygen_dev / verify_dev   slh_keygen_internal and slh_verify_internal (Algorithms 18 and 20) over raw device pointers (e.g. torch `data_ptr()`),
               ordered on `stream`, nothing allocated; the caller supplies the seeds and the workspace
  sign_workspace_bytes / sign_dev   slh_sign_internal (Algorithm 19) over raw device pointers, under the same rules; the workspace is all zero afterwards
  keygen_internal / verify_internal / sign_internal   the host forms over lists of bytes (they run on the device too)
  keygen / sign / verify   slh_keygen (Algorithm 21: the three seeds from os.urandom), slh_sign(M, ctx, SK) (Algorithm 22: addrnd from os.urandom
               unless deterministic) and slh_verify(M, SIG, ctx, PK) (Algorithm 24), with M' = 0 || |ctx| || ctx || M.  They exist in Python only; the
               library itself draws no randomness and formats no message.

A parameter set is named "SLH-DSA-SHAKE-128s", "-128f", "-192s", "-192f", "-256s" or "-256f".  The SHA-2 sets are tools_amd.slhdsa_sha2;
HashSLH-DSA is not here."""
import ctypes as C
import os

import numpy as np

from ._ffi import _rows, _vp, check, lib

PARAM = {"SLH-DSA-SHAKE-128s": 0, "SLH-DSA-SHAKE-128f": 1, "SLH-DSA-SHAKE-192s": 2, "SLH-DSA-SHAKE-192f": 3, "SLH-DSA-SHAKE-256s": 4, "SLH-DSA-SHAKE-256f": 5}
OP_KEYGEN, OP_VERIFY = range(2)
OPS = {"keygen": OP_KEYGEN, "verify": OP_VERIFY}

_typed = False


def _lib():
    global _typed
    L = lib()
    if not _typed:
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        L.psf_slhdsa_sizes.argtypes = [i] + [C.POINTER(sz)] * 3
        L.psf_slhdsa_workspace_bytes.argtypes = [i, sz, i, C.POINTER(sz)]
        L.psf_slhdsa_keygen_dev.argtypes = [i, i, sz, vp, vp, vp, vp, vp, vp, sz, vp]
        L.psf_slhdsa_verify_dev.argtypes = [i, i, sz, vp, sz, vp, sz, sz, vp, vp, vp, sz, vp]
        L.psf_slhdsa_keygen.argtypes = [i, i, sz, vp, vp, vp, vp, vp]
        L.psf_slhdsa_verify.argtypes = [i, i, sz, vp, sz, vp, sz, sz, vp, vp]
        L.psf_slhdsa_sign_workspace_bytes.argtypes = [i, sz, C.POINTER(sz)]
        L.psf_slhdsa_sign_dev.argtypes = [i, i, sz, vp, sz, vp, sz, sz, vp, vp, vp, sz, vp]
        L.psf_slhdsa_sign.argtypes = [i, i, sz, vp, sz, vp, sz, sz, vp, vp]
        _typed = True
    return L


def _param(name):
    if name in PARAM:
        return PARAM[name]
    if not isinstance(name, str) and name in PARAM.values():
        return name
    raise ValueError(f"unknown SLH-DSA parameter set {name!r}")


def sizes(name):
    """{"pk": ..., "sk": ..., "sig": ...} in bytes; n is pk / 2"""
    v = [C.c_size_t(0) for _ in range(3)]
    check(_lib().psf_slhdsa_sizes(_param(name), *[C.byref(x) for x in v]), "slhdsa.sizes")
    return dict(zip(("pk", "sk", "sig"), (int(x.value) for x in v)))


def workspace_bytes(name, count, op):
    """bytes of the 256-byte aligned device workspace that `op` ("keygen", "verify") needs for `count` instances"""
    out = C.c_size_t(0)
    check(_lib().psf_slhdsa_workspace_bytes(_param(name), count, OPS[op] if op in OPS else op, C.byref(out)), "slhdsa.workspace_bytes")
    return int(out.value)


def keygen_dev(name, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, d_ws, ws_bytes, device=0, stream=None):
    """psf_slhdsa_keygen_dev: (pk_c, sk_c) = slh_keygen_internal(SK.seed_c, SK.prf_c, PK.seed_c); the workspace is all zero afterwards"""
    check(_lib().psf_slhdsa_keygen_dev(device, _param(name), count, d_sk_seed or 0, d_sk_prf or 0, d_pk_seed or 0, d_pk or 0, d_sk or 0, d_ws or 0, ws_bytes, stream or 0),
          "slhdsa.keygen_dev")


def verify_dev(name, count, d_pk, d_msg, msg_len, d_sig, d_ok, d_ws, ws_bytes, pk_stride=None, msg_stride=None, device=0, stream=None):
    """psf_slhdsa_verify_dev: ok[c] = slh_verify_internal(M_c, SIG_c, PK_c).  pk_stride defaults to the pk size (0: one key for all), msg_stride to
    msg_len."""
    if pk_stride is None:
        pk_stride = sizes(name)["pk"]
    check(_lib().psf_slhdsa_verify_dev(device, _param(name), count, d_pk or 0, pk_stride, d_msg or 0, msg_len, msg_len if msg_stride is None else msg_stride,
                                       d_sig or 0, d_ok or 0, d_ws or 0, ws_bytes, stream or 0), "slhdsa.verify_dev")


def sign_workspace_bytes(name, count):
    """bytes of the 256-byte aligned device workspace that signing needs for `count` instances (the same for every sk_stride)"""
    out = C.c_size_t(0)
    check(_lib().psf_slhdsa_sign_workspace_bytes(_param(name), count, C.byref(out)), "slhdsa.sign_workspace_bytes")
    return int(out.value)


def sign_dev(name, count, d_sk, d_msg, msg_len, d_addrnd, d_sig, d_ws, ws_bytes, sk_stride=None, msg_stride=None, device=0, stream=None):
    """psf_slhdsa_sign_dev: SIG_c = slh_sign_internal(M_c, SK_c, addrnd_c); d_addrnd None: the deterministic variant.  sk_stride defaults to the sk size
    (0: one key for all), msg_stride to msg_len.  The workspace is all zero afterwards."""
    if sk_stride is None:
        sk_stride = sizes(name)["sk"]
    check(_lib().psf_slhdsa_sign_dev(device, _param(name), count, d_sk or 0, sk_stride, d_msg or 0, msg_len, msg_len if msg_stride is None else msg_stride,
                                     d_addrnd or 0, d_sig or 0, d_ws or 0, ws_bytes, stream or 0), "slhdsa.sign_dev")


# ---- host forms ------------------------------------------------------------------------------------------------------------------------------------

def keygen_internal(name, sk_seeds, sk_prfs, pk_seeds, device=0):
    """[(pk, sk)] for the n-byte (SK.seed, SK.prf, PK.seed) of each instance"""
    sz = sizes(name)
    n = sz["pk"] // 2
    a, b, c = _rows(sk_seeds, n, "SK.seed", "slhdsa"), _rows(sk_prfs, n, "SK.prf", "slhdsa"), _rows(pk_seeds, n, "PK.seed", "slhdsa")
    if not len(a) == len(b) == len(c):
        raise ValueError("slhdsa.keygen_internal: as many SK.prf and PK.seed strings as SK.seed strings")
    pk, sk = np.empty((len(a), sz["pk"]), np.uint8), np.empty((len(a), sz["sk"]), np.uint8)
    check(_lib().psf_slhdsa_keygen(device, _param(name), len(a), _vp(a), _vp(b), _vp(c), _vp(pk), _vp(sk)), "slhdsa.keygen_internal")
    return [(bytes(x), bytes(y)) for x, y in zip(pk, sk)]


def verify_internal(name, pks, msgs, sigs, device=0):
    """[bool] for each (PK, M, SIG); `pks` is one key (bytes) for all or a list with one key per instance; the messages of one call have one length"""
    sz = sizes(name)
    sig = _rows(sigs, sz["sig"], "signature", "slhdsa")
    msgs = [bytes(m) for m in msgs]
    lens = {len(m) for m in msgs}
    if len(lens) > 1:
        raise ValueError("slhdsa.verify_internal: the messages of one call have one length")
    msg_len = lens.pop() if lens else 0
    msg = _rows(msgs, msg_len, "message", "slhdsa")
    one = isinstance(pks, (bytes, bytearray))
    pk = _rows([pks] if one else pks, sz["pk"], "pk", "slhdsa")
    if len(msg) != len(sig) or (not one and len(pk) != len(sig)):
        raise ValueError("slhdsa.verify_internal: as many keys and messages as signatures")
    ok = np.zeros(len(sig), np.uint8)
    check(_lib().psf_slhdsa_verify(device, _param(name), len(sig), _vp(pk), 0 if one else sz["pk"], _vp(msg), msg_len, msg_len, _vp(sig), _vp(ok)),
          "slhdsa.verify_internal")
    return [bool(a) for a in ok]


def sign_internal(name, sks, msgs, addrnds=None, device=0):
    """[SIG] for each (SK, M, addrnd); `sks` is one key (bytes) for all or a list with one key per instance; the messages of one call have one length;
    addrnds None: the deterministic variant, else one n-byte string per instance"""
    sz = sizes(name)
    n = sz["pk"] // 2
    msgs = [bytes(m) for m in msgs]
    lens = {len(m) for m in msgs}
    if len(lens) > 1:
        raise ValueError("slhdsa.sign_internal: the messages of one call have one length")
    msg_len = lens.pop() if lens else 0
    msg = _rows(msgs, msg_len, "message", "slhdsa")
    one = isinstance(sks, (bytes, bytearray))
    sk = _rows([sks] if one else sks, sz["sk"], "sk", "slhdsa")
    rnd = None if addrnds is None else _rows(addrnds, n, "addrnd", "slhdsa")
    if (not one and len(sk) != len(msg)) or (rnd is not None and len(rnd) != len(msg)):
        raise ValueError("slhdsa.sign_internal: as many keys and addrnd strings as messages")
    sig = np.zeros((len(msg), sz["sig"]), np.uint8)
    check(_lib().psf_slhdsa_sign(device, _param(name), len(msg), _vp(sk), 0 if one else sz["sk"], _vp(msg), msg_len, msg_len, None if rnd is None else _vp(rnd),
                                 _vp(sig)), "slhdsa.sign_internal")
    return [bytes(x) for x in sig]


# ---- Algorithms 21, 22 and 24: the external forms, in Python only ------------------------------------------------------------------------------------------

def keygen(name, count=1, device=0, random=os.urandom):
    """slh_keygen for `count` fresh key pairs: SK.seed, SK.prf and PK.seed from `random` (os.urandom), then keygen_internal; [(pk, sk)]"""
    n = sizes(name)["pk"] // 2
    seeds = [[random(n) for _ in range(count)] for _ in range(3)]
    return keygen_internal(name, *seeds, device=device)


def sign(name, sk, M, ctx=b"", deterministic=False, device=0, random=os.urandom):
    """slh_sign (Algorithm 22) of one message: ValueError when ctx is longer than 255 bytes, else slh_sign_internal(0 || |ctx| || ctx || M, SK, addrnd)
    with addrnd n bytes from `random` (os.urandom), or none when `deterministic`"""
    if len(ctx) > 255:
        raise ValueError("slhdsa.sign: ctx longer than 255 bytes")
    addrnd = None if deterministic else [random(sizes(name)["pk"] // 2)]
    return sign_internal(name, bytes(sk), [bytes([0, len(ctx)]) + bytes(ctx) + bytes(M)], addrnd, device=device)[0]


def verify(name, pk, M, sig, ctx=b"", device=0):
    """slh_verify (Algorithm 24) of one signature: ValueError when ctx is longer than 255 bytes, else slh_verify_internal(0 || |ctx| || ctx || M, SIG, PK)"""
    if len(ctx) > 255:
        raise ValueError("slhdsa.verify: ctx longer than 255 bytes")
    return verify_internal(name, bytes(pk), [bytes([0, len(ctx)]) + bytes(ctx) + bytes(M)], [sig], device=device)[0]
