"""What the SLH-DSA signing tests share (tests/test_slhdsa_sign_cpu.py, tests/test_gpu_slhdsa_sign.py), over tests/helpers/slhdsa_cases.py: the
(sk, M, addrnd) behind every honest signature of the shared fixture, and a check of a signature against the model that costs about 0.1 s instead of a
model signature (0.3 to 15 s).  No new model signature of an s set is made here."""
import functools
import random

from tests.helpers import slhdsa_cases as K
from tests.helpers import slhdsa_model as M


@functools.lru_cache(maxsize=None)
def hedged(name):
    """the (sk, M, addrnd, SIG) behind K.signed(name): that function's generator replayed (per triple the message, then addrnd).  The replayed message is
    compared with the fixture's; a wrong addrnd could only make a byte comparison with SIG fail."""
    ks = K.keys(name, K.distinct(name))
    n = M.PARAMS[name].n
    rng = random.Random(9001 * K.NAMES.index(name) + 5)
    out = []
    for i, (pk, msg, sig) in enumerate(K.signed(name)):
        m = rng.randbytes(K.MSG_LEN)
        addrnd = rng.randbytes(n)
        assert m == msg and ks["pk"][i] == pk
        out.append((ks["sk"][i], msg, addrnd, sig))
    return tuple(out)


def edge_inputs(name):
    """[(sk, M, SIG)] of K.edge_signed(name): deterministic signatures under the first key"""
    sk = K.keys(name, K.distinct(name))["sk"][0]
    return [(sk, msg, sig) for _, msg, sig in K.edge_signed(name).values()]


def prf_edge_lens(name):
    """message lengths with SK.prf || opt_rand || M one byte short of a SHAKE256 block, exactly one block, one byte more"""
    n = M.PARAMS[name].n
    return [135 - 2 * n, 136 - 2 * n, 137 - 2 * n]


def exact_by_parts(name, sk, msg, addrnd, sig):
    """None when `sig` is the model's sign_internal(msg, sk, addrnd), else the first part that differs: "verify" (the model rejects it), "R", "fors_sk<t>",
    "wots<j>".  R, the k FORS secret values and each layer's WOTS+ values are compared with the model's own; the authentication nodes are then pinned by
    the model's verification, which recomputes PK.root from those leaves.  About 0.1 s."""
    s = M.PARAMS[name]
    n, ln = s.n, M.wots_len(name)[2]
    if len(sig) != M.sizes(name)["sig"]:
        return "size"
    sk_seed, sk_prf, pk_seed, pk_root = (sk[i * n:(i + 1) * n] for i in range(4))
    if not M.verify_internal(name, msg, sig, pk_seed + pk_root):
        return "verify"
    r = sig[:n]
    if r != M.prf_msg(name, sk_prf, pk_seed if addrnd is None else addrnd, msg):
        return "R"
    md, idx_tree, idx_leaf = M.split_digest(name, M.h_msg(name, r, pk_seed, pk_root, msg))
    adrs = M.Adrs()
    adrs.set_tree(idx_tree)
    adrs.set_type_and_clear(M.FORS_TREE)
    adrs.set_keypair(idx_leaf)
    reg = M.regions(name)
    for t, (index, (lo, hi)) in enumerate(zip(M.base_2b(md, s.a, s.k), reg["fors_sk"])):
        if sig[lo:hi] != M.fors_sk_gen(name, sk_seed, pk_seed, adrs, (t << s.a) + index):
            return f"fors_sk{t}"
    sig_fors = sig[n:n + s.k * (1 + s.a) * n]
    node = M.fors_pk_from_sig(name, sig_fors, md, pk_seed, adrs)
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
        if sig[lo:hi] != M.wots_sign(name, node, sk_seed, pk_seed, adrs):
            return f"wots{j}"
        node = M.xmss_pk_from_sig(name, idx_leaf, sig[lo:end], node, pk_seed, adrs)
    return None
