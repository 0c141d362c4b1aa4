"""The tables of the SLH-DSA edge suite (tests/test_gpu_slhdsa_edges.py), with the hash family as a parameter: SHAKE (tests/helpers/slhdsa_model.py
over tests/helpers/slhdsa_cases.py) or SHA2 (tests/helpers/slhdsa_sha2_model.py over tests/helpers/slhdsa_sha2_cases.py).  Every expected value a GPU
test takes from here is tied to the model by tests/test_slhdsa_edge_cases_cpu.py.

  chosen(fam, name, case)    signatures whose digest fields sit at an edge: (M, addrnd) found by a search with the model's own PRF_msg and H_msg under
                             the first fixture key; the search's counter is recorded in COUNTERS, so nothing searches at test time
  degenerate_verify / degenerate_sign   signatures, a public key and secret keys of all 0x00 / all 0xFF
  flips(fam, name)           the batch with one flipped bit in every byte of one honest signature
  coverage(fam)              which WOTS+ digits and idx_leaf parities the fixtures of the GPU tests reach

All of it is made once per process (lru_cache) and never modified."""
import functools
import random

import numpy as np

from tests.helpers import slhdsa_cases, slhdsa_model, slhdsa_sha2_cases, slhdsa_sha2_model


class Family:
    """one hash family: `K` its fixture module, `M` its model module, and the model's PRF_msg and H_msg under one signature"""

    def __init__(self, tag, K, M):
        self.tag, self.K, self.M = tag, K, M

    def __repr__(self):
        return self.tag

    def name(self, short):
        """"128f" -> "SLH-DSA-SHAKE-128f" or "SLH-DSA-SHA2-128f" """
        return f"SLH-DSA-{self.tag}-{short}"

    def prf_msg(self, name, sk_prf, opt_rand, msg):
        if self.tag == "SHAKE":
            return self.M.prf_msg(name, sk_prf, opt_rand, msg)
        return self.M.Scheme(name).f.prf_msg(sk_prf, opt_rand, msg)

    def h_msg(self, name, r, pk_seed, pk_root, msg):
        if self.tag == "SHAKE":
            return self.M.h_msg(name, r, pk_seed, pk_root, msg)
        return self.M.Scheme(name).f.h_msg(r, pk_seed, pk_root, msg)

    def layer_messages(self, name, pk, msg, sig):
        """(idx_leaf of layer 0, [the n-byte message that layer j's WOTS+ signs]) of a signature the model accepts"""
        s, M = self.M.PARAMS[name], self.M
        n = s.n
        sch = slhdsa_sha2_model.Scheme(s, slhdsa_sha2_model.Shake if self.tag == "SHAKE" else slhdsa_sha2_model.Sha2)
        md, idx_tree, idx_leaf = M.split_digest(name, self.h_msg(name, sig[:n], pk[:n], pk[n:], msg))
        first = idx_leaf
        fors_len = s.k * (1 + s.a) * n
        node = sch.fors_pk_from_sig(sig[n:n + fors_len], md, pk[:n], sch._fors_adrs(idx_tree, idx_leaf))
        out, step = [], (sch.len + s.hp) * n
        for j in range(s.d):
            out.append(node)
            adrs = slhdsa_model.Adrs()
            adrs.set_layer(j)
            adrs.set_tree(idx_tree)
            at = n + fors_len + j * step
            node = sch.xmss_pk_from_sig(idx_leaf, sig[at:at + step], node, pk[:n], adrs)
            idx_leaf = idx_tree % (1 << s.hp)
            idx_tree >>= s.hp
        assert node == pk[n:]
        return first, out


SHAKE = Family("SHAKE", slhdsa_cases, slhdsa_model)
SHA2 = Family("SHA2", slhdsa_sha2_cases, slhdsa_sha2_model)
FAMILIES = {"SHAKE": SHAKE, "SHA2": SHA2}
SHORT = ("128s", "128f", "192s", "192f", "256s", "256f")
CHOSEN_SETS = ("128f", "256f")


def flip(data, pos, bit=0):
    b = bytearray(data)
    b[pos] ^= 1 << bit
    return bytes(b)


def first_key(fam, name):
    """(pk, sk) of the first fixture key"""
    ks = fam.K.keys(name, fam.K.distinct(name))
    return ks["pk"][0], ks["sk"][0]


# ---- chosen digests ------------------------------------------------------------------------------------------------------------------------------------
CASES = ("leaf_0_tree_top_clear", "leaf_max_tree_top_set", "fors_edges")
SEED = 20506
# the first counter t at which candidate(name, case, t) meets wanted(): found by search(), which the CPU test repeats
COUNTERS = {
    ("SHAKE", "128f", "leaf_0_tree_top_clear"): 2,
    ("SHAKE", "128f", "leaf_max_tree_top_set"): 15,
    ("SHAKE", "128f", "fors_edges"): 3612,
    ("SHAKE", "256f", "leaf_0_tree_top_clear"): 28,
    ("SHAKE", "256f", "leaf_max_tree_top_set"): 2,
    ("SHAKE", "256f", "fors_edges"): 748,
    ("SHA2", "128f", "leaf_0_tree_top_clear"): 26,
    ("SHA2", "128f", "leaf_max_tree_top_set"): 2,
    ("SHA2", "128f", "fors_edges"): 4450,
    ("SHA2", "256f", "leaf_0_tree_top_clear"): 3,
    ("SHA2", "256f", "leaf_max_tree_top_set"): 31,
    ("SHA2", "256f", "fors_edges"): 692,
}


def fields(fam, name, sk, msg, addrnd):
    """(R, md, idx_tree, idx_leaf, the k FORS indices) of slh_sign_internal(msg, sk, addrnd): two hashes"""
    s = fam.M.PARAMS[name]
    n = s.n
    r = fam.prf_msg(name, sk[n:2 * n], sk[2 * n:3 * n] if addrnd is None else addrnd, msg)
    md, idx_tree, idx_leaf = fam.M.split_digest(name, fam.h_msg(name, r, sk[2 * n:3 * n], sk[3 * n:], msg))
    return r, md, idx_tree, idx_leaf, slhdsa_model.base_2b(md, s.a, s.k)


def wanted(fam, name, case, idx_tree, idx_leaf, fors):
    """(a) idx_leaf = 0 and the top bit of idx_tree clear; (b) idx_leaf = 2^h' - 1 and that bit set (bit 63 on 256f, bit 62 on 128f); (c) on 128f FORS
    tree 0 at index 0 and tree k - 1 at index 2^a - 1, on 256f tree k - 1 at index 2^a - 1 alone (its bits end inside byte 39 of md; the joint event
    would cost about 2^18 candidates)"""
    s = fam.M.PARAMS[name]
    top = (idx_tree >> (s.h - s.hp - 1)) & 1
    if case == CASES[0]:
        return idx_leaf == 0 and top == 0
    if case == CASES[1]:
        return idx_leaf == (1 << s.hp) - 1 and top == 1
    assert case == CASES[2]
    return fors[s.k - 1] == (1 << s.a) - 1 and (fors[0] == 0 or s.n == 32)


def candidate(fam, name, case, t):
    """the t-th (M, addrnd) of the search for one case: a generator of its own per candidate, so that the recorded counter alone gives the pair back"""
    rng = random.Random(f"{SEED} {name} {case} {t}")
    return rng.randbytes(fam.K.MSG_LEN), rng.randbytes(fam.M.PARAMS[name].n)


def search(fam, name, case, limit=1 << 16):
    sk = first_key(fam, name)[1]
    for t in range(limit):
        msg, addrnd = candidate(fam, name, case, t)
        if wanted(fam, name, case, *fields(fam, name, sk, msg, addrnd)[2:]):
            return t
    raise AssertionError((name, case, "nothing among", limit))


def chosen_inputs(fam, short, case):
    """(name, pk, sk, M, addrnd) of one case, from its recorded counter"""
    name = fam.name(short)
    pk, sk = first_key(fam, name)
    return (name, pk, sk) + candidate(fam, name, case, COUNTERS[fam.tag, short, case])


@functools.lru_cache(maxsize=None)
def chosen(fam, short, case):
    """(name, pk, sk, M, addrnd, SIG): the model's hedged signature of one case, signed once"""
    name, pk, sk, msg, addrnd = chosen_inputs(fam, short, case)
    return name, pk, sk, msg, addrnd, fam.M.sign_internal(name, msg, sk, addrnd)


def all_chosen(fam):
    return [chosen(fam, short, case) for short in CHOSEN_SETS for case in CASES]


# ---- degenerate bytes ----------------------------------------------------------------------------------------------------------------------------------
def degenerate_verify(fam, short):
    """[(what, pk, M, SIG)]: signatures of all 0x00 and all 0xFF under an honest key, and an honest signature under a public key of all 0x00; the
    expected verdict of each is the model's (fam.K.expect)"""
    name = fam.name(short)
    pk, msg, sig = fam.K.signed(name)[0]
    return [("sig 0x00", pk, msg, bytes(len(sig))), ("sig 0xFF", pk, msg, b"\xff" * len(sig)), ("pk 0x00", bytes(len(pk)), msg, sig)]


DEGENERATE_SIGN_SET = "128f"


@functools.lru_cache(maxsize=None)
def degenerate_sign():
    """[(what, sk, M, addrnd, SIG)] on SHAKE-128f: secret keys of all 0x00 and all 0xFF, hedged and deterministic, with the model's own signature.
    PK.root inside such a key is not the root of its hypertree, so the model's verification rejects these signatures and
    tests/helpers/slhdsa_sign_cases.py's exact_by_parts, whose first step is that verification, cannot serve: the whole signature of the model it is (two
    signatures, about a second)."""
    name = SHAKE.name(DEGENERATE_SIGN_SET)
    n = SHAKE.M.PARAMS[name].n
    rng = random.Random(SEED + 1)
    out = []
    for what, sk, hedged in (("sk 0x00", bytes(4 * n), True), ("sk 0xFF", b"\xff" * (4 * n), False)):
        msg, addrnd = rng.randbytes(SHAKE.K.MSG_LEN), rng.randbytes(n) if hedged else None
        out.append((what, sk, msg, addrnd, SHAKE.M.sign_internal(name, msg, sk, addrnd)))
    return out


# ---- a flipped bit in every byte -----------------------------------------------------------------------------------------------------------------------
EVERY = 61


@functools.lru_cache(maxsize=None)
def flips(fam, name):
    """The batch over the first honest signature of `name`: instance j is that signature untouched when j mod 61 = 0, else the signature with bit
    b mod 8 of byte b flipped, b counting the flipped instances in order: every byte of the signature exactly once, none left out.  Returns {"pk", "msg",
    "sig", "count", "byte": int64 array (-1: untouched), "bit": uint8 array (the mask 1 << bit, 0: untouched), "want": uint8 array (1: untouched)}."""
    pk, msg, sig = fam.K.signed(name)[0]
    size = len(sig)
    byte, j = [], 0
    b = 0
    while b < size:
        if j % EVERY == 0:
            byte.append(-1)
        else:
            byte.append(b)
            b += 1
        j += 1
    byte = np.array(byte, dtype=np.int64)
    assert sorted(byte[byte >= 0].tolist()) == list(range(size))
    mask = np.where(byte >= 0, 1 << (byte % 8), 0).astype(np.uint8)
    return {"pk": pk, "msg": msg, "sig": sig, "count": len(byte), "byte": byte, "bit": mask, "want": (byte < 0).astype(np.uint8)}


def flipped_instance(table, j):
    """the signature of instance j of flips()"""
    b = int(table["byte"][j])
    return table["sig"] if b < 0 else flip(table["sig"], b, b % 8)


def region_of(fam, name, pos):
    """the name of the region of a signature that byte `pos` lies in"""
    reg = fam.M.regions(name)
    if pos < reg["R"][1]:
        return "R"
    for kind in ("fors_sk", "fors_auth", "wots", "auth"):
        for t, (lo, hi) in enumerate(reg[kind]):
            if lo <= pos < hi:
                return f"{kind}{t}"
    raise AssertionError(pos)


def region_ends(fam, name):
    """the first and the last byte of every region: R, every FORS secret value and path, every layer's WOTS part and path"""
    reg = fam.M.regions(name)
    spans = [reg["R"]] + [x for kind in ("fors_sk", "fors_auth", "wots", "auth") for x in reg[kind]]
    return sorted({p for lo, hi in spans for p in (lo, hi - 1)})


def spread(fam, name, many=16):
    """`many` byte positions spread over the signature, the first and the last byte among them"""
    size = fam.M.sizes(name)["sig"]
    return sorted({(size - 1) * i // (many - 1) for i in range(many)})


def pinned_instances(fam, name):
    """the instances of flips() whose verdict the CPU test asks the model for: the ends of every region on 128f, 16 spread positions elsewhere, and the
    first two untouched instances"""
    table = flips(fam, name)
    at = {int(b): j for j, b in enumerate(table["byte"]) if b >= 0}
    pos = region_ends(fam, name) if name.endswith("128f") else spread(fam, name)
    return [0, EVERY] + [at[p] for p in pos]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coverage(fam):
    """over the f-set fixtures and the chosen signatures, which the GPU tests sign and verify: {"msg": digits seen in a message part of a WOTS+
    signature, "csum": digits seen in a checksum part, "leaf": parities of idx_leaf seen}"""
    out = {"msg": set(), "csum": set(), "leaf": set()}
    triples = [(name, *t) for name in fam.K.F_SETS for t in fam.K.signed(name)] + [(c[0], c[1], c[3], c[5]) for c in all_chosen(fam)]
    for name, pk, msg, sig in triples:
        len1 = fam.M.wots_len(name)[0]
        leaf, layers = fam.layer_messages(name, pk, msg, sig)
        out["leaf"].add(leaf % 2)
        for m1 in layers:
            digits = fam.M.wots_digits(name, m1)
            out["msg"].update(digits[:len1])
            out["csum"].update(digits[len1:])
    return out
