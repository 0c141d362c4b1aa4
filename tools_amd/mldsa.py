"""ML-DSA (FIPS 204, August 2024) on the device, batched, through the C ABI (psf_mldsa_*, include/psf_mi355x.h): bytes in, bytes out.

  sizes / workspace_bytes   the byte sizes of a parameter set and of the workspace of an operation
  keygen_dev / verify_dev   ML-DSA.KeyGen_internal and ML-DSA.Verify_internal (Algorithms 6 and 8) over raw device pointers (e.g. torch
               `data_ptr()`), ordered on `stream`, nothing allocated; the caller supplies xi and the workspace
  keygen_internal / verify_internal   the host forms over lists of bytes (they run on the device too)
  sign_workspace_bytes / sign_begin_dev / sign_round_dev / sign_end_dev   ML-DSA.Sign_internal (Algorithm 7) over raw device pointers: begin, then
               rounds with `active` = the value last read from the device word d_live until it is 0, then end
  sign_internal   the host form of signing over lists of bytes: signatures and the number of attempts of each
  keygen / sign / verify   ML-DSA.KeyGen (xi from os.urandom), ML-DSA.Sign(sk, M, ctx) (Algorithm 2: rnd from os.urandom, or 32 zero bytes with
               deterministic=True) and ML-DSA.Verify(pk, M, sigma, ctx) (Algorithm 3), with M' = 0 || |ctx| || ctx || M.  They exist in Python only; the
               library itself draws no randomness and formats no message.

A parameter set is named "ML-DSA-44", "ML-DSA-65" or "ML-DSA-87"; `why` is an OR of WHY_HINT, WHY_NORM and WHY_HASH."""
import ctypes as C
import os

import numpy as np

from ._ffi import _rows, _vp, check, lib

PARAM = {"ML-DSA-44": 44, "ML-DSA-65": 65, "ML-DSA-87": 87}
OP_KEYGEN, OP_VERIFY = range(2)
OPS = {"keygen": OP_KEYGEN, "verify": OP_VERIFY}
MSG_BYTES, MSG_MU = range(2)
WHY_HINT, WHY_NORM, WHY_HASH = 1, 2, 4

_typed = False


def _lib():
    global _typed
    L = lib()
    if not _typed:
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        L.psf_mldsa_sizes.argtypes = [i] + [C.POINTER(sz)] * 3
        L.psf_mldsa_workspace_bytes.argtypes = [i, sz, i, C.POINTER(sz)]
        L.psf_mldsa_keygen_dev.argtypes = [i, i, sz, vp, vp, vp, vp, sz, vp, vp]
        L.psf_mldsa_verify_dev.argtypes = [i, i, sz, vp, sz, vp, sz, sz, i, vp, vp, vp, vp, sz, vp, vp]
        L.psf_mldsa_keygen.argtypes = [i, i, sz, vp, vp, vp]
        L.psf_mldsa_verify.argtypes = [i, i, sz, vp, sz, vp, sz, sz, i, vp, vp, vp]
        L.psf_mldsa_sign_workspace_bytes.argtypes = [i, sz, sz, C.POINTER(sz)]
        L.psf_mldsa_sign_begin_dev.argtypes = [i, i, sz, vp, sz, vp, sz, sz, i, vp, vp, sz, vp, vp, vp]
        L.psf_mldsa_sign_round_dev.argtypes = [i, i, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp]
        L.psf_mldsa_sign_end_dev.argtypes = [i, i, sz, sz, vp, sz, vp]
        L.psf_mldsa_sign.argtypes = [i, i, sz, vp, sz, vp, sz, sz, i, vp, vp, C.c_uint32, vp]
        _typed = True
    return L


def _param(name):
    if name in PARAM:
        return PARAM[name]
    if name in PARAM.values():
        return name
    raise ValueError(f"unknown ML-DSA parameter set {name!r}")


def sizes(name):
    """{"pk": ..., "sk": ..., "sig": ...} in bytes"""
    v = [C.c_size_t(0) for _ in range(3)]
    check(_lib().psf_mldsa_sizes(_param(name), *[C.byref(x) for x in v]), "mldsa.sizes")
    return dict(zip(("pk", "sk", "sig"), (int(x.value) for x in v)))


def workspace_bytes(name, count, op):
    """bytes of the 256-byte aligned device workspace that `op` ("keygen", "verify") needs for `count` instances"""
    out = C.c_size_t(0)
    check(_lib().psf_mldsa_workspace_bytes(_param(name), count, OPS[op] if op in OPS else op, C.byref(out)), "mldsa.workspace_bytes")
    return int(out.value)


def keygen_dev(name, count, d_xi, d_pk, d_sk, d_ws, ws_bytes, d_fail=None, device=0, stream=None):
    """psf_mldsa_keygen_dev: (pk_c, sk_c) = ML-DSA.KeyGen_internal(xi_c)"""
    check(_lib().psf_mldsa_keygen_dev(device, _param(name), count, d_xi or 0, d_pk or 0, d_sk or 0, d_ws or 0, ws_bytes, d_fail or 0, stream or 0),
          "mldsa.keygen_dev")


def verify_dev(name, count, d_pk, d_msg, msg_len, d_sig, d_ok, d_ws, ws_bytes, d_why=None, pk_stride=None, msg_stride=None, msg_kind=MSG_BYTES, d_fail=None,
               device=0, stream=None):
    """psf_mldsa_verify_dev: ok[c] = ML-DSA.Verify_internal(pk_c, M'_c, sigma_c).  pk_stride defaults to the pk size (0: one key for all), msg_stride
    to msg_len; msg_kind MSG_MU: the 64 message bytes are mu."""
    if pk_stride is None:
        pk_stride = sizes(name)["pk"]
    check(_lib().psf_mldsa_verify_dev(device, _param(name), count, d_pk or 0, pk_stride, d_msg or 0, msg_len, msg_len if msg_stride is None else msg_stride, msg_kind,
                                      d_sig or 0, d_ok or 0, d_why or 0, d_ws or 0, ws_bytes, d_fail or 0, stream or 0), "mldsa.verify_dev")


def sign_workspace_bytes(name, count, sk_stride=None):
    """bytes of the 256-byte aligned device workspace of one signing of `count` instances; sk_stride 0: one key for all (the smaller layout),
    None: the sk size (one key per instance)"""
    out = C.c_size_t(0)
    check(_lib().psf_mldsa_sign_workspace_bytes(_param(name), count, sizes(name)["sk"] if sk_stride is None else sk_stride, C.byref(out)), "mldsa.sign_workspace_bytes")
    return int(out.value)


def sign_begin_dev(name, count, d_sk, d_msg, msg_len, d_ws, ws_bytes, d_live, d_rnd=None, sk_stride=None, msg_stride=None, msg_kind=MSG_BYTES, d_fail=None, device=0,
                   stream=None):
    """psf_mldsa_sign_begin_dev: slot j of the workspace gets instance j, *d_live = count.  d_rnd None: the deterministic variant"""
    if sk_stride is None:
        sk_stride = sizes(name)["sk"]
    check(_lib().psf_mldsa_sign_begin_dev(device, _param(name), count, d_sk or 0, sk_stride, d_msg or 0, msg_len, msg_len if msg_stride is None else msg_stride, msg_kind,
                                          d_rnd or 0, d_ws or 0, ws_bytes, d_live or 0, d_fail or 0, stream or 0), "mldsa.sign_begin_dev")


def sign_round_dev(name, count, active, d_sig, d_ws, ws_bytes, d_live, d_rounds=None, sk_stride=None, d_fail=None, device=0, stream=None):
    """psf_mldsa_sign_round_dev: one attempt for the first min(active, *d_live) slots; accepted instances get their signature and leave"""
    if sk_stride is None:
        sk_stride = sizes(name)["sk"]
    check(_lib().psf_mldsa_sign_round_dev(device, _param(name), count, sk_stride, active, d_sig or 0, d_rounds or 0, d_ws or 0, ws_bytes, d_live or 0, d_fail or 0,
                                          stream or 0), "mldsa.sign_round_dev")


def sign_end_dev(name, count, d_ws, ws_bytes, sk_stride=None, device=0, stream=None):
    """psf_mldsa_sign_end_dev: every byte of the workspace to zero"""
    if sk_stride is None:
        sk_stride = sizes(name)["sk"]
    check(_lib().psf_mldsa_sign_end_dev(device, _param(name), count, sk_stride, d_ws or 0, ws_bytes, stream or 0), "mldsa.sign_end_dev")


# ---- host forms ------------------------------------------------------------------------------------------------------------------------------------

def keygen_internal(name, xis, device=0):
    """[(pk, sk)] for the 32-byte seed xi of each instance"""
    sz = sizes(name)
    xi = _rows(xis, 32, "xi", "mldsa")
    pk, sk = np.empty((len(xi), sz["pk"]), np.uint8), np.empty((len(xi), sz["sk"]), np.uint8)
    check(_lib().psf_mldsa_keygen(device, _param(name), len(xi), _vp(xi), _vp(pk), _vp(sk)), "mldsa.keygen_internal")
    return [(bytes(a), bytes(b)) for a, b in zip(pk, sk)]


def verify_internal(name, pks, msgs, sigs, msg_kind=MSG_BYTES, device=0, why=False):
    """[bool] (why=True: [(bool, why)]) for each (pk, M', sigma); `pks` is one key (bytes) for all or a list with one key per instance; the messages
    of one call have one length"""
    sz = sizes(name)
    sig = _rows(sigs, sz["sig"], "signature", "mldsa")
    msgs = [bytes(m) for m in msgs]
    lens = {len(m) for m in msgs}
    if len(lens) > 1:
        raise ValueError("mldsa.verify_internal: the messages of one call have one length")
    msg_len = lens.pop() if lens else 0
    msg = _rows(msgs, msg_len, "message", "mldsa")
    one = isinstance(pks, (bytes, bytearray))
    pk = _rows([pks] if one else pks, sz["pk"], "pk", "mldsa")
    if len(msg) != len(sig) or (not one and len(pk) != len(sig)):
        raise ValueError("mldsa.verify_internal: as many keys and messages as signatures")
    ok, wh = np.zeros(len(sig), np.uint8), np.zeros(len(sig), np.uint8)
    check(_lib().psf_mldsa_verify(device, _param(name), len(sig), _vp(pk), 0 if one else sz["pk"], _vp(msg), msg_len, msg_len, msg_kind, _vp(sig), _vp(ok), _vp(wh)),
          "mldsa.verify_internal")
    return [(bool(a), int(b)) for a, b in zip(ok, wh)] if why else [bool(a) for a in ok]


def sign_internal(name, sks, msgs, rnds=None, msg_kind=MSG_BYTES, max_rounds=1024, device=0):
    """([signature], [attempts]) for each (sk, M', rnd); `sks` is one key (bytes) for all or a list with one key per instance; the messages of one
    call have one length; rnds None: the deterministic variant.  Raises PsfError(PSF_ERR_SAMPLER) when instances are unsigned after max_rounds."""
    sz = sizes(name)
    msgs = [bytes(m) for m in msgs]
    lens = {len(m) for m in msgs}
    if len(lens) > 1:
        raise ValueError("mldsa.sign_internal: the messages of one call have one length")
    msg_len = lens.pop() if lens else 0
    msg = _rows(msgs, msg_len, "message", "mldsa")
    one = isinstance(sks, (bytes, bytearray))
    sk = _rows([sks] if one else sks, sz["sk"], "sk", "mldsa")
    rnd = None if rnds is None else _rows(rnds, 32, "rnd", "mldsa")
    if (not one and len(sk) != len(msg)) or (rnd is not None and len(rnd) != len(msg)):
        raise ValueError("mldsa.sign_internal: as many keys and rnd strings as messages")
    sig, rounds = np.zeros((len(msg), sz["sig"]), np.uint8), np.zeros(len(msg), np.uint32)
    check(_lib().psf_mldsa_sign(device, _param(name), len(msg), _vp(sk), 0 if one else sz["sk"], _vp(msg), msg_len, msg_len, msg_kind, None if rnd is None else _vp(rnd),
                                _vp(sig), max_rounds, _vp(rounds)), "mldsa.sign_internal")
    return [bytes(a) for a in sig], [int(r) for r in rounds]


# ---- Algorithms 1, 2 and 3: the external forms, in Python only ------------------------------------------------------------------------------------------

def keygen(name, count, device=0, random=os.urandom):
    """ML-DSA.KeyGen for `count` fresh key pairs: xi from `random` (os.urandom), then keygen_internal"""
    return keygen_internal(name, [random(32) for _ in range(count)], device=device)


def sign(name, sk, M, ctx=b"", random=os.urandom, deterministic=False, device=0):
    """ML-DSA.Sign (Algorithm 2) of one message: rnd from `random` (os.urandom), or 32 zero bytes when deterministic; ValueError when ctx is longer
    than 255 bytes"""
    if len(ctx) > 255:
        raise ValueError("mldsa.sign: ctx longer than 255 bytes")
    rnd = None if deterministic else [random(32)]
    return sign_internal(name, bytes(sk), [bytes([0, len(ctx)]) + bytes(ctx) + bytes(M)], rnd, device=device)[0][0]


def verify(name, pk, M, sig, ctx=b"", device=0):
    """ML-DSA.Verify (Algorithm 3) of one signature: False when ctx is longer than 255 bytes, else Verify_internal(pk, 0 || |ctx| || ctx || M, sigma)"""
    if len(ctx) > 255:
        return False
    return verify_internal(name, bytes(pk), [bytes([0, len(ctx)]) + bytes(ctx) + bytes(M)], [sig], device=device)[0]
