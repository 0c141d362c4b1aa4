"""The harness of the ML-DSA signing device tests (tests/test_gpu_mldsa_sign.py): one function that runs begin / round / end over a batch under a
schedule of `active` values with every check that holds for any call (guard bytes around the signatures, nothing written outside the workspace, the
signature bytes of unsigned instances untouched by a round, d_live against d_rounds after every round, the workspace all zero after end, the flag
unchanged), the batches the tests share, and the cached runs of the restated signer they are compared with.  Nothing here imports the library or
torch: both are arguments."""
import functools
import random

from tests.helpers import mldsa_model as M
from tests.helpers import mldsa_sign_cases as K
from tests.helpers import mldsa_sign_model as S
from tests.helpers.mldsa_gpu import NAMES, _put_pitched, keys
from tests.helpers.mlkem_gpu import FILL, GUARD, _off, _out, _put

MU = 1
MAX_ROUNDS = 400


def schedule_readback(count, live, r):
    return live


def schedule_full(count, live, r):
    return count


def schedule_half(count, live, r):
    """the true value and half of it in turn: some live instances sit out every second round"""
    return live if r % 2 == 0 else live // 2


@functools.lru_cache(maxsize=None)
def batch(name, one_key):
    """40 instances with mu given, as (sks, mus, rnds): the case instances (all under the first case key when one_key) and seeded random ones.  The
    first 30 are the same under both arrangements, so their reference runs once."""
    rng = random.Random(911 * NAMES.index(name) + 5)
    key0 = K.sk_of(name, K.instance(name, 0)[0])
    inst = [(sk, mu, rnd) for sk, mu, rnd in K.case_instances(name) if sk == key0]
    while len(inst) < 30:
        inst.append((key0, rng.randbytes(64), rng.randbytes(32)))
    if one_key:
        while len(inst) < 40:
            inst.append((key0, rng.randbytes(64), rng.randbytes(32)))
    else:
        inst += [c for c in K.case_instances(name) if c[0] != key0]
        other = keys(name, 3)["sk"]
        while len(inst) < 40:
            inst.append((other[len(inst) % 3], rng.randbytes(64), rng.randbytes(32)))
    return tuple(zip(*inst))


@functools.lru_cache(maxsize=None)
def reference(name, sk, msg, rnd, is_mu):
    """(signature, attempts) of the restated signer, cached by content"""
    return (S.sign_trace(sk, name, mu=msg, rnd=rnd) if is_mu else S.sign_trace(sk, name, m_prime=msg, rnd=rnd))[:2]


def dev_sign(torch, D, name, sks, msgs, rnds=None, msg_kind=0, schedule=schedule_readback, off=1, flag=0, max_rounds=MAX_ROUNDS, offs=None, sk_stride=None,
             msg_stride=None, gap=0xC3, with_rounds=True, with_fail=True):
    """signs the instances on the device through begin / round / end; `sks`: bytes (one key for all, sk_stride = 0) or a list with one key per instance;
    rnds None: d_rnd = NULL.  `offs` as in tests/helpers/mldsa_gpu.py (`off`: the same offset for every buffer); `sk_stride` / `msg_stride`: the pitch
    of the keys (of a list) / the messages, None: packed.  with_rounds / with_fail False: d_rounds / d_fail = NULL; without d_rounds the unsigned
    instances are those whose signature bytes are all FILL.  Returns (signatures, rounds, live after each round); an unsigned instance's signature is
    all FILL bytes, and rounds is None without d_rounds."""
    count, sz = len(msgs), M.sizes(name)
    one = isinstance(sks, bytes)
    assert not (one and sk_stride)
    stride = 0 if one else (sk_stride or sz["sk"])
    if offs is None:
        offs = off
    off = _off(offs, "out_sig")
    msg_len = len(msgs[0])
    assert all(len(m) == msg_len for m in msgs)
    bsk, psk = _put_pitched(torch, [sks] if one else sks, _off(offs, "in_sk"), sk_stride, gap)
    bm, pm = _put_pitched(torch, msgs, _off(offs, "in_msg"), msg_stride, gap ^ 0x5F) if msg_len else (None, None)
    br, pr = _put(torch, rnds, _off(offs, "in_rnd")) if rnds is not None else (None, None)
    bsig, psig = _out(torch, count * sz["sig"], off)
    rounds = torch.zeros(count, dtype=torch.int32, device="cuda")
    live = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    fail = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    p_rounds, p_fail = rounds.data_ptr() if with_rounds else None, fail.data_ptr() if with_fail else None
    wsb = D.sign_workspace_bytes(name, count, stride)
    assert wsb % 256 == 0 and wsb > 0
    ws = torch.full((wsb + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    pws = (ws.data_ptr() + 255) // 256 * 256
    lo = pws - ws.data_ptr()
    what = (name, count, "one key" if one else "key per instance", schedule.__name__)
    torch.cuda.synchronize()
    D.sign_begin_dev(name, count, psk, pm, msg_len, pws, wsb, live.data_ptr(), d_rnd=pr, sk_stride=stride, msg_stride=msg_stride, msg_kind=msg_kind, d_fail=p_fail)
    torch.cuda.synchronize()
    now = int(live.item())
    assert now == count, (what, "d_live after begin", now)
    sig_rows = bsig[GUARD + off:GUARD + off + count * sz["sig"]].view(count, sz["sig"])
    trail = []
    for r in range(max_rounds):
        if now == 0:
            break
        D.sign_round_dev(name, count, schedule(count, now, r), psig, pws, wsb, live.data_ptr(), d_rounds=p_rounds, sk_stride=stride, d_fail=p_fail)
        torch.cuda.synchronize()
        now = int(live.item())
        trail.append(now)
        unsigned = rounds == 0 if with_rounds else (sig_rows == FILL).all(dim=1)
        assert now == int(unsigned.sum().item()), (what, "d_live against the zero entries of d_rounds", r, now)
        assert bool((sig_rows[unsigned] == FILL).all().item()), (what, "a round touched the signature of an instance it did not accept", r)
    D.sign_end_dev(name, count, pws, wsb, sk_stride=stride)
    torch.cuda.synchronize()
    assert not bool(ws[lo:lo + wsb].any().item()), (what, "the workspace is not all zero after end")
    assert bool((ws[:lo] == 0x5A).all().item()) and bool((ws[lo + wsb:] == 0x5A).all().item()), (what, "wrote outside the workspace")
    assert int(fail.item()) == flag, (what, "the flag changed")
    host = bsig.cpu().numpy()
    assert (host[:GUARD + off] == FILL).all() and (host[GUARD + off + count * sz["sig"]:] == FILL).all(), (what, "wrote outside the signatures")
    sigs = [bytes(host[GUARD + off + i * sz["sig"]:GUARD + off + (i + 1) * sz["sig"]]) for i in range(count)]
    del bsk, bm, br
    return sigs, [int(v) for v in rounds.cpu()] if with_rounds else None, trail
