"""The harness of the ML-DSA device tests (tests/test_gpu_mldsa.py, tests/test_gpu_fips204.py): buffers one byte past a 16-byte boundary with guard
bytes around every output (the pieces of tests/helpers/mlkem_gpu.py), the workspace and sampler flag of a call with their checks, one function per
device entry point that runs it and applies all of them, and the cached runs of the pure-Python model that the tests compare with.  The model's
signer is slow, so its outputs are cached per (name, ...) and large batches are made by tiling a few distinct (key, message, signature) triples.
Nothing here imports the library or torch: both are arguments."""
import functools
import random

from tests.helpers import mldsa_model as M
from tests.helpers.mlkem_gpu import _out, _put, _take

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


def dev_keygen(torch, D, name, xi, flag=0):
    count, sz = len(xi), M.sizes(name)
    bxi, pxi = _put(torch, xi)
    bpk, ppk = _out(torch, count * sz["pk"])
    bsk, psk = _out(torch, count * sz["sk"])
    sc = Scratch(torch, D, name, count, "keygen", flag)
    torch.cuda.synchronize()
    D.keygen_dev(name, count, pxi, ppk, psk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
    pk = _take(torch, bpk, count * sz["pk"], sz["pk"], (name, count, "pk"))
    sk = _take(torch, bsk, count * sz["sk"], sz["sk"], (name, count, "sk"))
    sc.check((name, count, "keygen"), cleared=True)
    del bxi
    return pk, sk, (bpk, ppk)


def dev_verify(torch, D, name, pks, msgs, sigs, msg_kind=0, flag=0, pk_ptr=None, with_why=True):
    """verify_dev over the instances; `pks`: a list with one key per instance, or bytes (one key for all: pk_stride = 0); returns (ok, why) as lists"""
    count, sz = len(sigs), M.sizes(name)
    one = isinstance(pks, bytes)
    keep = None
    if pk_ptr is None:
        keep, pk_ptr = _put(torch, [pks] if one else pks)
    msg_len = len(msgs[0])
    assert all(len(m) == msg_len for m in msgs)
    bm, pm = _put(torch, msgs) if msg_len else (None, None)
    bs, ps = _put(torch, sigs)
    bok, pok = _out(torch, count)
    bwhy, pwhy = _out(torch, count)
    sc = Scratch(torch, D, name, count, "verify", flag)
    torch.cuda.synchronize()
    D.verify_dev(name, count, pk_ptr, pm, msg_len, ps, pok, sc.ptr, sc.bytes, d_why=pwhy if with_why else None, pk_stride=0 if one else sz["pk"],
                 msg_kind=msg_kind, d_fail=sc.flag.data_ptr())
    ok = [b[0] for b in _take(torch, bok, count, 1, (name, count, "ok"))]
    why = [b[0] for b in _take(torch, bwhy, count if with_why else 0, 1, (name, count, "why"))] if with_why else None
    if not with_why:
        _take(torch, bwhy, 0, 1, (name, count, "why"))                     # untouched when d_why is NULL
    sc.check((name, count, "verify"), cleared=False)
    del keep, bm, bs
    return ok, why
