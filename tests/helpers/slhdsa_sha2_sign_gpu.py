"""The harness of the signing device tests of SLH-DSA's SHA-2 sets (tests/test_gpu_slhdsa_sha2_sign*.py): tests/helpers/slhdsa_sign_gpu.py's dev_sign over the
sizes of tests/helpers/slhdsa_sha2_model.py -- every buffer one byte past a 16-byte boundary, guard bytes around the signatures, a workspace filled with a
non-zero byte that is all zero after the call, nothing written outside the workspace; `offs`, `sk_stride`, `msg_stride` and `gap` as described there
(addrnd is always packed: the library takes no stride for it).  Nothing here imports the library or torch: both are arguments."""
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers.mldsa_gpu import _put_pitched
from tests.helpers.mlkem_gpu import _off, _out, _put, _take
from tests.helpers.slhdsa_sign_gpu import SignScratch  # noqa: F401


def dev_sign(torch, D, name, sks, msgs, addrnds=None, offs=None, sk_stride=None, msg_stride=None, gap=0xC3):
    """sign_dev over the instances; `sks`: a list with one key per instance, or bytes (one key for all: sk_stride = 0); addrnds None: the deterministic
    variant (no pointer); an empty message has no pointer either; `sk_stride` / `msg_stride`: the pitch of the keys (of a list) / the messages, None:
    packed; returns the signatures as a list of bytes"""
    count, sz = len(msgs), M.sizes(name)
    one = isinstance(sks, bytes)
    assert (one or len(sks) == count) and not (one and sk_stride)
    o_sig = _off(offs, "out_sig")
    bk, pk = _put_pitched(torch, [sks] if one else sks, _off(offs, "in_sk"), sk_stride, gap)
    msg_len = len(msgs[0])
    assert all(len(m) == msg_len for m in msgs)
    bm, pm = _put_pitched(torch, msgs, _off(offs, "in_msg"), msg_stride, gap ^ 0x5F) if msg_len else (None, None)
    br, pr = (None, None) if addrnds is None else _put(torch, addrnds, _off(offs, "in_rnd"))
    assert addrnds is None or (len(addrnds) == count and all(len(r) == sz["pk"] // 2 for r in addrnds))
    bs, ps = _out(torch, count * sz["sig"], o_sig)
    sc = SignScratch(torch, D, name, count)
    torch.cuda.synchronize()
    D.sign_dev(name, count, pk, pm, msg_len, pr, ps, sc.ptr, sc.bytes, sk_stride=0 if one else (sk_stride or sz["sk"]), msg_stride=msg_stride)
    sigs = _take(torch, bs, count * sz["sig"], sz["sig"], (name, count, "sig"), o_sig)
    sc.check((name, count, "sign"))
    del bk, bm, br
    return sigs
