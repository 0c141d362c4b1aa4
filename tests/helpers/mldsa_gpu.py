"""The harness of the ML-DSA device tests (tests/test_gpu_mldsa*.py, tests/test_gpu_fips204.py): buffers at chosen byte offsets from a 16-byte
boundary with guard bytes around every output (the pieces of tests/helpers/mlkem_gpu.py), the workspace and sampler flag of a call with their
checks, one function per device entry point that runs it and applies all of them, and the cached runs of the pure-Python model that the tests
compare with.  The model's signer is slow, so its outputs are cached per (name, ...) and large batches are made by tiling a few distinct (key,
message, signature) triples.  Nothing here imports the library or torch: both are arguments.

Offsets.  Every `dev_*` function (dev_sign of tests/helpers/mldsa_sign_gpu.py too) takes `offs`: None (every buffer one byte past a 16-byte
boundary, the default of the suite), an int (that offset for every buffer) or a dict from `offsets()` with one entry per buffer: the inputs
"in_xi", "in_pk", "in_sk", "in_msg", "in_sig", "in_rnd" and the outputs "out_pk", "out_sk", "out_sig", "out_ok", "out_why".

Strides.  `pk_stride`, `sk_stride` and `msg_stride` lay the items of that input out at that pitch (`_put_pitched`); the bytes between two items
are a non-zero pattern that starts at `gap`.  Outputs are packed: they have no gap bytes."""
import functools
import random

import numpy as np

from tests.helpers import mldsa_model as M
from tests.helpers.mlkem_gpu import _off, _out, _put, _take

INPUTS = ("xi", "pk", "sk", "msg", "sig", "rnd")
OUTPUTS = ("pk", "sk", "sig", "ok", "why")


def offsets(inputs=1, outputs=1, **named):
    """the `offs` dict with every input at `inputs`, every output at `outputs`, and the buffers in `named` (in_sk=0, out_sig=4, ...) at their own"""
    offs = {"in_" + k: inputs for k in INPUTS}
    offs.update({"out_" + k: outputs for k in OUTPUTS})
    for key, value in named.items():
        assert key in offs, key
        offs[key] = value
    return offs


def pitched(items, stride, gap):
    """the items of one size at a pitch of `stride` bytes as one bytes object; the bytes after each item (the last too) are gap, gap + 1, ... without zeros"""
    size = len(items[0])
    assert stride > size and all(len(x) == size for x in items) and 0 < gap < 256
    rows = np.empty((len(items), stride), dtype=np.uint8)
    rows[:, :size] = np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), size)
    fill = (gap + np.arange(len(items) * (stride - size), dtype=np.int64)) % 255 + 1
    rows[:, size:] = fill.astype(np.uint8).reshape(len(items), stride - size)
    return rows.tobytes()


def _put_pitched(torch, items, off=1, stride=None, gap=0xC3):
    """_put with the items `stride` bytes apart (None or their size: packed)"""
    if stride is None or stride == len(items[0]):
        return _put(torch, items, off)
    return _put(torch, [pitched(items, stride, gap)], off)

NAMES = sorted(M.PARAMS)
DISTINCT = 3


@functools.lru_cache(maxsize=None)
def keys(name, count):
    """the model's KeyGen_internal of `count` fixed seeds: {"xi", "pk", "sk"} (never modified by a test)"""
    rng = random.Random(2003 * NAMES.index(name) + count)
    xi = [rng.randbytes(32) for _ in range(count)]
    pairs = [M.keygen_internal(x, name) for x in xi]
    return {"xi": xi, "pk": [p for p, _ in pairs], "sk": [s for _, s in pairs]}


@functools.lru_cache(maxsize=None)
def triples(name, msg_len, one_key=False):
    """DISTINCT honest (pk, M', sigma) of the model with messages of msg_len bytes, under DISTINCT keys or all under the first"""
    ks = keys(name, DISTINCT)
    rng = random.Random(7001 * NAMES.index(name) + 13 * msg_len + one_key)
    out = []
    for i in range(DISTINCT):
        j = 0 if one_key else i
        msg = rng.randbytes(msg_len)
        out.append((ks["pk"][j], msg, M.sign_internal(ks["sk"][j], msg, rng.randbytes(32), name)))
    return out


def tiled(name, count, msg_len, one_key=False):
    """`count` instances: instance i is triple i mod DISTINCT; returns (pks, msgs, sigs)"""
    t = triples(name, msg_len, one_key)
    return tuple([t[i % DISTINCT][f] for i in range(count)] for f in range(3))


@functools.lru_cache(maxsize=None)
def why_of(name, pk, msg, sig):
    """the model's verdict, cached by content: tiled batches repeat a few distinct instances"""
    return M.verify_why(pk, msg, sig, name)


def mu_of(pk, msg):
    return M.H(M.H(pk, 64) + msg, 64)


def flip(data, pos, bit=0):
    b = bytearray(data)
    b[pos] ^= 1 << bit
    return bytes(b)


def layout(name):
    """byte offsets inside a signature: {"z": first byte of z, "hint": first hint byte, "zb": bytes per polynomial of z}"""
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    zb = 32 * (1 + (g1 - 1).bit_length())
    return {"z": cb, "hint": cb + zb * l, "zb": zb}


def with_z_coefficient(name, sig, poly, index, value):
    """the signature with coefficient `index` of polynomial `poly` of z set to `value`"""
    g1 = M.PARAMS[name][5]
    lay = layout(name)
    at = lay["z"] + lay["zb"] * poly
    z = M.bit_unpack(sig[at:at + lay["zb"]], g1 - 1, g1)
    z[index] = value
    return sig[:at] + M.bit_pack(z, g1 - 1, g1) + sig[at + lay["zb"]:]


def with_hint(name, sig, y):
    return sig[:layout(name)["hint"]] + bytes(y)


class Scratch:
    """the workspace of one call, filled with a non-zero byte, and a sampler flag that starts at `flag`"""

    def __init__(self, torch, D, name, count, op, flag=0):
        self.torch, self.bytes = torch, D.workspace_bytes(name, count, op)
        assert self.bytes % 256 == 0 and self.bytes > 0
        self.ws = torch.full((self.bytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        self.ptr = (self.ws.data_ptr() + 255) // 256 * 256
        self.start = flag
        self.flag = torch.full((1,), flag, dtype=torch.int32, device="cuda")

    def check(self, what, cleared):
        """nothing written outside the workspace, the flag as it was, and (keygen) every byte of the workspace zero"""
        self.torch.cuda.synchronize()
        lo = self.ptr - self.ws.data_ptr()
        if cleared:
            assert not bool(self.ws[lo:lo + self.bytes].any().item()), (what, "the workspace is not all zero after the call")
        assert bool((self.ws[:lo] == 0x5A).all().item()) and bool((self.ws[lo + self.bytes:] == 0x5A).all().item()), (what, "wrote outside the workspace")
        assert int(self.flag.item()) == self.start, (what, "the sampler flag changed")


def dev_keygen(torch, D, name, xi, flag=0, offs=None):
    count, sz = len(xi), M.sizes(name)
    o_pk, o_sk = _off(offs, "out_pk"), _off(offs, "out_sk")
    bxi, pxi = _put(torch, xi, _off(offs, "in_xi"))
    bpk, ppk = _out(torch, count * sz["pk"], o_pk)
    bsk, psk = _out(torch, count * sz["sk"], o_sk)
    sc = Scratch(torch, D, name, count, "keygen", flag)
    torch.cuda.synchronize()
    D.keygen_dev(name, count, pxi, ppk, psk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
    pk = _take(torch, bpk, count * sz["pk"], sz["pk"], (name, count, "pk"), o_pk)
    sk = _take(torch, bsk, count * sz["sk"], sz["sk"], (name, count, "sk"), o_sk)
    sc.check((name, count, "keygen"), cleared=True)
    del bxi
    return pk, sk, (bpk, ppk)


def dev_verify(torch, D, name, pks, msgs, sigs, msg_kind=0, flag=0, pk_ptr=None, with_why=True, offs=None, pk_stride=None, msg_stride=None, gap=0xC3):
    """verify_dev over the instances; `pks`: a list with one key per instance, or bytes (one key for all: pk_stride = 0); `pk_stride` / `msg_stride`:
    the pitch of the keys (of a list) / the messages, None: packed; returns (ok, why) as lists"""
    count, sz = len(sigs), M.sizes(name)
    one = isinstance(pks, bytes)
    o_ok, o_why = _off(offs, "out_ok"), _off(offs, "out_why")
    assert not (one and pk_stride) and not (pk_ptr is not None and pk_stride)
    keep = None
    if pk_ptr is None:
        keep, pk_ptr = _put_pitched(torch, [pks] if one else pks, _off(offs, "in_pk"), pk_stride, gap)
    msg_len = len(msgs[0])
    assert all(len(m) == msg_len for m in msgs)
    bm, pm = _put_pitched(torch, msgs, _off(offs, "in_msg"), msg_stride, gap ^ 0x5F) if msg_len else (None, None)
    bs, ps = _put(torch, sigs, _off(offs, "in_sig"))
    bok, pok = _out(torch, count, o_ok)
    bwhy, pwhy = _out(torch, count, o_why)
    sc = Scratch(torch, D, name, count, "verify", flag)
    torch.cuda.synchronize()
    D.verify_dev(name, count, pk_ptr, pm, msg_len, ps, pok, sc.ptr, sc.bytes, d_why=pwhy if with_why else None,
                 pk_stride=0 if one else (pk_stride or sz["pk"]), msg_stride=msg_stride, msg_kind=msg_kind, d_fail=sc.flag.data_ptr())
    ok = [b[0] for b in _take(torch, bok, count, 1, (name, count, "ok"), o_ok)]
    why = [b[0] for b in _take(torch, bwhy, count, 1, (name, count, "why"), o_why)] if with_why else None
    if not with_why:
        _take(torch, bwhy, 0, 1, (name, count, "why"), o_why)              # untouched when d_why is NULL
    sc.check((name, count, "verify"), cleared=False)
    del keep, bm, bs
    return ok, why
