"""What the tests of the SHA-2 sets of SLH-DSA share (tests/test_slhdsa_sha2_*.py, tests/test_gpu_slhdsa_sha2.py): keys and honest signatures of the
pure-Python model of tests/helpers/slhdsa_sha2_model.py (its sign_internal, with HMAC for PRF_msg), made once per process and never modified, as
tests/helpers/slhdsa_cases.py does for the SHAKE sets: three (key, message, signature) triples per f set and one per s set, plus the four message
lengths around the padding edges of H_msg's inner hash on SHA2-128f (SHA-256, and two MGF1 counters) and SHA2-256f (SHA-512); batches are made by
tiling those and tampering per instance, and the expected verdict of every instance is the model's verify."""
import functools
import random

from tests.helpers import slhdsa_sha2_model as M
from tests.helpers.slhdsa_cases import flip  # noqa: F401

NAMES = M.NAMES
F_SETS = [n for n in NAMES if n.endswith("f")]
S_SETS = [n for n in NAMES if n.endswith("s")]
MSG_LEN = 33
F128, F192, F256 = "SLH-DSA-SHA2-128f", "SLH-DSA-SHA2-192f", "SLH-DSA-SHA2-256f"
EDGE_SETS = (F128, F256)


def distinct(name):
    return 3 if name in F_SETS else 1


def edge_lens(name):
    """message lengths with R || PK.seed || PK.root || M at: the last length whose padding fits the block, the first whose padding spills into a block
    of its own, exactly one block; and the empty message.  The block is 64 bytes with a 9-byte padding (SHA-256, n = 16) or 128 with 17 (SHA-512)."""
    n = M.PARAMS[name].n
    block, pad = (64, 9) if n == 16 else (128, 17)
    return [block - pad - 3 * n, block - pad + 1 - 3 * n, block - 3 * n, 0]


@functools.lru_cache(maxsize=None)
def keys(name, count):
    """the model's slh_keygen_internal of `count` fixed seed triples: {"sk_seed", "sk_prf", "pk_seed", "pk", "sk"}, lists"""
    n = M.PARAMS[name].n
    rng = random.Random(5231 * NAMES.index(name) + count)
    out = {k: [] for k in ("sk_seed", "sk_prf", "pk_seed", "pk", "sk")}
    for _ in range(count):
        a, b, c = rng.randbytes(n), rng.randbytes(n), rng.randbytes(n)
        sk, pk = M.keygen_internal(name, a, b, c)
        for k, v in zip(("sk_seed", "sk_prf", "pk_seed", "pk", "sk"), (a, b, c, pk, sk)):
            out[k].append(v)
    return out


@functools.lru_cache(maxsize=None)
def signed(name):
    """distinct(name) honest (pk, M, SIG) of the model, each under its own key, messages of MSG_LEN bytes, hedged (addrnd random)"""
    ks = keys(name, distinct(name))
    n = M.PARAMS[name].n
    rng = random.Random(7919 * NAMES.index(name) + 3)
    out = []
    for i in range(distinct(name)):
        msg = rng.randbytes(MSG_LEN)
        out.append((ks["pk"][i], msg, M.sign_internal(name, msg, ks["sk"][i], rng.randbytes(n))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_signed(name):
    """{msg_len: (pk, M, SIG)} for the lengths of edge_lens(name), under the first key"""
    assert name in EDGE_SETS
    ks = keys(name, distinct(name))
    rng = random.Random(6113 * NAMES.index(name) + 1)
    return {ln: (ks["pk"][0], msg, M.sign_internal(name, msg, ks["sk"][0])) for ln in edge_lens(name) for msg in [rng.randbytes(ln)]}


@functools.lru_cache(maxsize=None)
def full_tree_signed():
    """(pk, M, SIG) on SHA2-256f whose idx_tree has its top bit set: all 64 bits of the tree address are in use (found by trying messages)"""
    name = F256
    ks = keys(name, distinct(name))
    sch = M.Scheme(name)
    n, sk, pk = M.PARAMS[name].n, ks["sk"][0], ks["pk"][0]
    for t in range(64):
        msg = b"idx_tree %d" % t
        r = sch.f.prf_msg(sk[n:2 * n], pk[:n], msg)
        if M.split_digest(name, sch.f.h_msg(r, pk[:n], pk[n:], msg))[1] >> 63:
            return pk, msg, sch.sign_internal(msg, sk)
    raise AssertionError("no message with the top bit of idx_tree among 64")


CTX_SET = F128
CTX_LENS = (0, 1, 255)


@functools.lru_cache(maxsize=None)
def ctx_signed():
    """{len(ctx): (pk, M, ctx, SIG)}: slh_sign (Algorithm 22) of the model on CTX_SET under the first key, deterministic"""
    ks = keys(CTX_SET, distinct(CTX_SET))
    rng = random.Random(78)
    out = {}
    for ln in CTX_LENS:
        msg, ctx = rng.randbytes(40), rng.randbytes(ln)
        out[ln] = (ks["pk"][0], msg, ctx, M.sign(CTX_SET, msg, ctx, ks["sk"][0]))
    return out


def fixture():
    """every honest signature the suite uses, made once: {"signed": {name: triples}, "edge": {name: {msg_len: triple}}, "ctx": {len(ctx): ...}}"""
    return {"signed": {name: signed(name) for name in NAMES}, "edge": {name: edge_signed(name) for name in EDGE_SETS}, "ctx": ctx_signed()}


@functools.lru_cache(maxsize=None)
def expect(name, pk, msg, sig):
    """the model's verdict, cached by content: tiled batches repeat a few distinct instances"""
    return M.verify_internal(name, msg, sig, pk)


def tiled(name, count):
    """`count` instances: instance i is triple i mod distinct(name); returns (pks, msgs, sigs)"""
    t = signed(name)
    return tuple([t[i % len(t)][f] for i in range(count)] for f in range(3))


def region_positions(name):
    """[(what, byte position in the signature)]: one position in R, in every FORS tree's secret value and path, in every layer's WOTS part and path"""
    n = M.PARAMS[name].n
    reg = M.regions(name)
    out = [("R", reg["R"][0] + 3)]
    for t, ((a, _), (b, e)) in enumerate(zip(reg["fors_sk"], reg["fors_auth"])):
        out.append((f"fors_sk{t}", a + t % n))
        out.append((f"fors_auth{t}", b + (7 * t) % (e - b)))
    for j, ((a, e), (b, f)) in enumerate(zip(reg["wots"], reg["auth"])):
        out.append((f"wots{j}", a + (37 * j + 5) % (e - a)))
        out.append((f"auth{j}", b + (11 * j) % (f - b)))
    return out
