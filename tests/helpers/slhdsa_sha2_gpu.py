"""The harness of the device tests of SLH-DSA's SHA-2 sets (tests/test_gpu_slhdsa_sha2.py): tests/helpers/slhdsa_gpu.py's two functions over the sizes
of tests/helpers/slhdsa_sha2_model.py -- every buffer one byte past a 16-byte boundary with guard bytes around every output, a workspace filled with a
non-zero byte, the guards checked, and the workspace all zero after KeyGen.  Nothing here imports the library or torch: both are arguments."""
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers.mlkem_gpu import _out, _put, _take
from tests.helpers.slhdsa_gpu import Scratch


def dev_keygen(torch, D, name, sk_seeds, sk_prfs, pk_seeds):
    """keygen_dev over the instances; returns (pks, sks) as lists of bytes"""
    count, sz = len(sk_seeds), M.sizes(name)
    (ba, pa), (bb, pb), (bc, pc) = _put(torch, sk_seeds), _put(torch, sk_prfs), _put(torch, pk_seeds)
    bpk, ppk = _out(torch, count * sz["pk"])
    bsk, psk = _out(torch, count * sz["sk"])
    sc = Scratch(torch, D, name, count, "keygen")
    torch.cuda.synchronize()
    D.keygen_dev(name, count, pa, pb, pc, ppk, psk, sc.ptr, sc.bytes)
    pk = _take(torch, bpk, count * sz["pk"], sz["pk"], (name, count, "pk"))
    sk = _take(torch, bsk, count * sz["sk"], sz["sk"], (name, count, "sk"))
    sc.check((name, count, "keygen"), cleared=True)
    del ba, bb, bc
    return pk, sk


def dev_verify(torch, D, name, pks, msgs, sigs):
    """verify_dev over the instances; `pks`: a list with one key per instance, or bytes (one key for all: pk_stride = 0); returns ok as a list"""
    count, sz = len(sigs), M.sizes(name)
    one = isinstance(pks, bytes)
    bp, pp = _put(torch, [pks] if one else pks)
    msg_len = len(msgs[0])
    assert all(len(m) == msg_len for m in msgs) and len(msgs) == count
    bm, pm = _put(torch, msgs) if msg_len else (None, None)
    bs, ps = _put(torch, sigs)
    bok, pok = _out(torch, count)
    sc = Scratch(torch, D, name, count, "verify")
    torch.cuda.synchronize()
    D.verify_dev(name, count, pp, pm, msg_len, ps, pok, sc.ptr, sc.bytes, pk_stride=0 if one else sz["pk"])
    ok = [b[0] for b in _take(torch, bok, count, 1, (name, count, "ok"))]
    sc.check((name, count, "verify"), cleared=False)
    del bp, bm, bs
    return ok
