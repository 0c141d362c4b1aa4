"""The harness of the SLH-DSA device tests (tests/test_gpu_slhdsa.py): one function per device entry point that places every buffer one byte past a
16-byte boundary with guard bytes around every output (the pieces of tests/helpers/mlkem_gpu.py), gives the call a workspace filled with a non-zero
byte, runs it and checks the guards, and that the workspace is all zero after KeyGen.  Nothing here imports the library or torch: both are arguments.

Offsets.  Every `dev_*` function (those of tests/helpers/slhdsa_sha2_gpu.py and dev_sign of tests/helpers/slhdsa_sign_gpu.py too) takes `offs`: None
(every buffer one byte past a 16-byte boundary, the default of the suite), an int (that offset for every buffer) or a dict from `offsets()` with one
entry per buffer: the inputs "in_sk_seed", "in_sk_prf", "in_pk_seed", "in_pk", "in_sk", "in_msg", "in_sig", "in_rnd" and the outputs "out_pk",
"out_sk", "out_sig", "out_ok".

Strides.  `pk_stride`, `sk_stride` and `msg_stride` lay the items of that input out at that pitch (tests/helpers/mldsa_gpu.py's `pitched`); the bytes
between two items are a non-zero pattern that starts at `gap`.  Outputs are packed: they have no gap bytes."""
from tests.helpers import slhdsa_model as M
from tests.helpers.mldsa_gpu import _put_pitched
from tests.helpers.mlkem_gpu import _off, _out, _put, _put_dev, _take, _take_dev

INPUTS = ("sk_seed", "sk_prf", "pk_seed", "pk", "sk", "msg", "sig", "rnd")
OUTPUTS = ("pk", "sk", "sig", "ok")


def offsets(inputs=1, outputs=1, **named):
    """the `offs` dict with every input at `inputs`, every output at `outputs`, and the buffers in `named` (in_pk=0, out_ok=4, ...) at their own"""
    offs = {"in_" + k: inputs for k in INPUTS}
    offs.update({"out_" + k: outputs for k in OUTPUTS})
    for key, value in named.items():
        assert key in offs, key
        offs[key] = value
    return offs


class Scratch:
    """the workspace of one call, filled with a non-zero byte"""

    def __init__(self, torch, D, name, count, op):
        self.torch, self.bytes = torch, D.workspace_bytes(name, count, op)
        assert self.bytes % 256 == 0 and self.bytes > 0
        self.ws = torch.full((self.bytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        self.ptr = (self.ws.data_ptr() + 255) // 256 * 256

    def check(self, what, cleared):
        """nothing written outside the workspace, and (keygen) every byte of the workspace zero"""
        self.torch.cuda.synchronize()
        lo = self.ptr - self.ws.data_ptr()
        if cleared:
            assert not bool(self.ws[lo:lo + self.bytes].any().item()), (what, "the workspace is not all zero after the call")
        assert bool((self.ws[:lo] == 0x5A).all().item()) and bool((self.ws[lo + self.bytes:] == 0x5A).all().item()), (what, "wrote outside the workspace")


def dev_keygen(torch, D, name, sk_seeds, sk_prfs, pk_seeds, offs=None, model=M):
    """keygen_dev over the instances; returns (pks, sks) as lists of bytes; `model`: the module whose sizes() knows `name`"""
    count, sz = len(sk_seeds), model.sizes(name)
    o_pk, o_sk = _off(offs, "out_pk"), _off(offs, "out_sk")
    (ba, pa), (bb, pb), (bc, pc) = (_put(torch, x, _off(offs, "in_" + k)) for k, x in (("sk_seed", sk_seeds), ("sk_prf", sk_prfs), ("pk_seed", pk_seeds)))
    bpk, ppk = _out(torch, count * sz["pk"], o_pk)
    bsk, psk = _out(torch, count * sz["sk"], o_sk)
    sc = Scratch(torch, D, name, count, "keygen")
    torch.cuda.synchronize()
    D.keygen_dev(name, count, pa, pb, pc, ppk, psk, sc.ptr, sc.bytes)
    pk = _take(torch, bpk, count * sz["pk"], sz["pk"], (name, count, "pk"), o_pk)
    sk = _take(torch, bsk, count * sz["sk"], sz["sk"], (name, count, "sk"), o_sk)
    sc.check((name, count, "keygen"), cleared=True)
    del ba, bb, bc
    return pk, sk


def dev_verify(torch, D, name, pks, msgs, sigs, offs=None, pk_stride=None, msg_stride=None, gap=0xC3, model=M):
    """verify_dev over the instances; `pks`: a list with one key per instance, or bytes (one key for all: pk_stride = 0); `pk_stride` / `msg_stride`:
    the pitch of the keys (of a list) / the messages, None: packed; returns ok as a list"""
    count, sz = len(sigs), model.sizes(name)
    one = isinstance(pks, bytes)
    assert not (one and pk_stride)
    o_ok = _off(offs, "out_ok")
    bp, pp = _put_pitched(torch, [pks] if one else pks, _off(offs, "in_pk"), pk_stride, gap)
    msg_len = len(msgs[0])
    assert all(len(m) == msg_len for m in msgs) and len(msgs) == count
    bm, pm = _put_pitched(torch, msgs, _off(offs, "in_msg"), msg_stride, gap ^ 0x5F) if msg_len else (None, None)
    bs, ps = _put(torch, sigs, _off(offs, "in_sig"))
    bok, pok = _out(torch, count, o_ok)
    sc = Scratch(torch, D, name, count, "verify")
    torch.cuda.synchronize()
    D.verify_dev(name, count, pp, pm, msg_len, ps, pok, sc.ptr, sc.bytes, pk_stride=0 if one else (pk_stride or sz["pk"]), msg_stride=msg_stride)
    ok = [b[0] for b in _take(torch, bok, count, 1, (name, count, "ok"), o_ok)]
    sc.check((name, count, "verify"), cleared=False)
    del bp, bm, bs
    return ok


# ---- batches that live on the device: nothing of the batch's size crosses to the host --------------------------------------------------------------------
def rows(torch, items):
    """items of one size as a (len(items), size) uint8 tensor on the device"""
    import numpy as np
    return torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), len(items[0])).copy()).cuda()


def tile(torch, period_rows, count):
    """row i is row i mod period of `period_rows`"""
    p = period_rows.shape[0]
    return period_rows.repeat((count + p - 1) // p, 1)[:count].contiguous()


def same_rows(torch, got, period_rows, what):
    """got[i] == period_rows[i mod period] for every i, compared on the device a slab of periods at a time; names the first instances that differ"""
    count, step = got.shape[0], period_rows.shape[0] * 2048
    want = tile(torch, period_rows, min(step, count))
    bad = []
    for lo in range(0, count, step):
        part = got[lo:lo + step]
        ne = (part != want[:part.shape[0]]).any(dim=1)
        if bool(ne.any().item()):
            bad += [lo + int(i) for i in ne.nonzero().flatten()[:8].tolist()]
            if len(bad) >= 8:
                break
    assert not bad, (what, "first differing instances:", bad[:8], "of", count)


def release(torch):
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def dev_verify_rows(torch, D, name, pk_rows, msg_rows, sig_rows, off=0):
    """verify_dev over (count, size) device tensors: `pk_rows` with one row is one key for all (pk_stride = 0); the guards and the workspace are checked
    on the device; returns ok as a (count,) device tensor"""
    count = sig_rows.shape[0]
    one = pk_rows.shape[0] == 1
    assert (one or pk_rows.shape[0] == count) and msg_rows.shape[0] == count
    bp, pp = _put_dev(torch, pk_rows, off)
    bm, pm = _put_dev(torch, msg_rows, off)
    if sig_rows.is_contiguous() and sig_rows.data_ptr() % 16 == 0 and off == 0:
        bs, ps = sig_rows, sig_rows.data_ptr()                             # as it stands: no second copy of a batch of gigabytes
    else:
        bs, ps = _put_dev(torch, sig_rows, off)
    bok, pok = _out(torch, count, off)
    sc = Scratch(torch, D, name, count, "verify")
    torch.cuda.synchronize()
    D.verify_dev(name, count, pp, pm, msg_rows.shape[1], ps, pok, sc.ptr, sc.bytes, pk_stride=0 if one else pk_rows.shape[1])
    ok = _take_dev(torch, bok, count, 1, (name, count, "ok"), off).reshape(count)
    sc.check((name, count, "verify"), cleared=False)
    del bp, bm, bs
    return ok
