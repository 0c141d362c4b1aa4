"""What the signing tests of SLH-DSA's SHA-2 sets share (tests/test_slhdsa_sha2_sign_cpu.py, tests/test_gpu_slhdsa_sha2_sign*.py), over
tests/helpers/slhdsa_sha2_cases.py: the (sk, M, addrnd) behind every honest signature of the shared fixture, and a check of a signature against the model
that costs about 0.1 s instead of a model signature (0.3 to 15 s).  tests/helpers/slhdsa_sign_cases.py over Scheme(name) of the SHA-2 model.  No new
model signature of an s set is made here."""
import functools
import random

from tests.helpers import slhdsa_sha2_cases as K
from tests.helpers import slhdsa_sha2_model as M


@functools.lru_cache(maxsize=None)
def hedged(name):
    """the (sk, M, addrnd, SIG) behind K.signed(name): that function's generator replayed (per triple the message, then addrnd).  The replayed message is
    compared with the fixture's, and the replayed addrnd must give the fixture's R."""
    ks = K.keys(name, K.distinct(name))
    n = M.PARAMS[name].n
    sch = M.Scheme(name)
    rng = random.Random(7919 * K.NAMES.index(name) + 3)
    out = []
    for i, (pk, msg, sig) in enumerate(K.signed(name)):
        m = rng.randbytes(K.MSG_LEN)
        addrnd = rng.randbytes(n)
        sk = ks["sk"][i]
        assert m == msg and ks["pk"][i] == pk and sch.f.prf_msg(sk[n:2 * n], addrnd, msg) == sig[:n]
        out.append((sk, msg, addrnd, sig))
    return tuple(out)


def edge_inputs(name):
    """[(sk, M, SIG)] of K.edge_signed(name): deterministic signatures under the first key"""
    sk = K.keys(name, K.distinct(name))["sk"][0]
    return [(sk, msg, sig) for _, msg, sig in K.edge_signed(name).values()]


def prf_edge_lens(name):
    """message lengths with opt_rand || M, what HMAC's inner hash absorbs past its key block, at: the last length whose padding fits the block, the first
    whose padding opens a block of its own, exactly one block.  The block is 64 bytes with a 9-byte padding (SHA-256, n = 16) or 128 with 17 (SHA-512)."""
    n = M.PARAMS[name].n
    block, pad = (64, 9) if n == 16 else (128, 17)
    return [block - pad - n, block - pad + 1 - n, block - n]


@functools.lru_cache(maxsize=None)
def degenerate_sign():
    """[(what, sk, M, addrnd, SIG)] on SHA2-128f: secret keys of all 0x00 and all 0xFF, hedged and deterministic, with the model's own signature.  PK.root
    inside such a key is not the root of its hypertree, so the model's verification rejects these signatures and exact_by_parts, whose first step is that
    verification, cannot serve: the whole signature of the model it is (two signatures, about a second)."""
    name = K.F128
    n = M.PARAMS[name].n
    rng = random.Random(20507)
    out = []
    for what, sk, with_rnd in (("sk 0x00", bytes(4 * n), True), ("sk 0xFF", b"\xff" * (4 * n), False)):
        msg, addrnd = rng.randbytes(K.MSG_LEN), rng.randbytes(n) if with_rnd else None
        out.append((what, sk, msg, addrnd, M.sign_internal(name, msg, sk, addrnd)))
    return out


def exact_by_parts(name, sk, msg, addrnd, sig):
    """None when `sig` is the model's sign_internal(msg, sk, addrnd), else the first part that differs: "size", "verify" (the model rejects it), "R",
    "fors_sk<t>", "wots<j>".  R, the k FORS secret values and each layer's WOTS+ values are compared with the model's own; the authentication nodes are
    then pinned by the model's verification, which recomputes PK.root from those leaves.  About 0.1 s."""
    sch = M.Scheme(name)
    s = M.PARAMS[name]
    n = s.n
    if len(sig) != M.sizes(name)["sig"]:
        return "size"
    sk_seed, sk_prf, pk_seed, pk_root = (sk[i * n:(i + 1) * n] for i in range(4))
    if not sch.verify_internal(msg, sig, pk_seed + pk_root):
        return "verify"
    r = sig[:n]
    if r != sch.f.prf_msg(sk_prf, pk_seed if addrnd is None else addrnd, msg):
        return "R"
    md, idx_tree, idx_leaf = M.split_digest(name, sch.f.h_msg(r, pk_seed, pk_root, msg))
    adrs = M.Adrs()
    adrs.set_tree(idx_tree)
    adrs.set_type_and_clear(M.FORS_TREE)
    adrs.set_keypair(idx_leaf)
    reg = M.regions(name)
    for t, (index, (lo, hi)) in enumerate(zip(M.base_2b(md, s.a, s.k), reg["fors_sk"])):
        if sig[lo:hi] != sch.fors_sk_gen(sk_seed, pk_seed, adrs, (t << s.a) + index):
            return f"fors_sk{t}"
    sig_fors = sig[n:n + s.k * (1 + s.a) * n]
    node = sch.fors_pk_from_sig(sig_fors, md, pk_seed, adrs)
    for j in range(s.d):
        if j:
            idx_leaf = idx_tree % (1 << s.hp)
            idx_tree >>= s.hp
        adrs = M.Adrs()
        adrs.set_layer(j)
        adrs.set_tree(idx_tree)
        adrs.set_type_and_clear(M.WOTS_HASH)
        adrs.set_keypair(idx_leaf)
        (lo, hi), (_, end) = reg["wots"][j], reg["auth"][j]
        if sig[lo:hi] != sch.wots_sign(node, sk_seed, pk_seed, adrs):
            return f"wots{j}"
        node = sch.xmss_pk_from_sig(idx_leaf, sig[lo:end], node, pk_seed, adrs)
    return None
