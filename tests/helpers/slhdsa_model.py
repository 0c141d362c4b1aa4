"""A pure-Python model of SLH-DSA (FIPS 205, August 2024) for the SHAKE instantiation of section 11.1, over hashlib: Algorithms 1 to 20 and 22 to 24,
parameterised by (n, h, d, h', a, k, m) with lg_w = 4.  It is written from the standard's pseudocode, one function per algorithm, and shares no text
with the library; tests/test_slhdsa_model_cpu.py pins it by the standard's tables and identities.  There is no other SLH-DSA implementation to compare
with on the hosts the suite runs on, so wherever the suite says "byte-exact" it means: equal to this model.

PARAMS holds the six SHAKE sets of Table 2 and "toy" (n = 16, h = 4, d = 2, a = 3, k = 4), small enough to walk every leaf of its trees."""
import hashlib
from collections import namedtuple

Set = namedtuple("Set", "n h d hp a k m")
PARAMS = {
    "SLH-DSA-SHAKE-128s": Set(16, 63, 7, 9, 12, 14, 30),
    "SLH-DSA-SHAKE-128f": Set(16, 66, 22, 3, 6, 33, 34),
    "SLH-DSA-SHAKE-192s": Set(24, 63, 7, 9, 14, 17, 39),
    "SLH-DSA-SHAKE-192f": Set(24, 66, 22, 3, 8, 33, 42),
    "SLH-DSA-SHAKE-256s": Set(32, 64, 8, 8, 14, 22, 47),
    "SLH-DSA-SHAKE-256f": Set(32, 68, 17, 4, 9, 35, 49),
    "toy": Set(16, 4, 2, 2, 3, 4, 4),
}
NAMES = [n for n in PARAMS if n != "toy"]
IDS = {name: i for i, name in enumerate(NAMES)}                           # the library's numbers of the sets
LG_W, W = 4, 16
WOTS_HASH, WOTS_PK, TREE, FORS_TREE, FORS_ROOTS, WOTS_PRF, FORS_PRF = range(7)


def _set(p):
    return PARAMS[p] if isinstance(p, str) else p


def wots_len(p):
    """(len1, len2, len) of equations 5.1 to 5.4"""
    n = _set(p).n
    len1 = (8 * n + LG_W - 1) // LG_W
    len2 = ((len1 * (W - 1)).bit_length() - 1) // LG_W + 1                    # floor(log2(len1 (w - 1)) / lg_w) + 1
    return len1, len2, len1 + len2


def sizes(p):
    s = _set(p)
    return {"pk": 2 * s.n, "sk": 4 * s.n, "sig": (1 + s.k * (1 + s.a) + s.h + s.d * wots_len(s)[2]) * s.n}


# ---- section 4: integers, bytes, addresses --------------------------------------------------------------------------------------------------------------

def to_int(x):
    """Algorithm 2"""
    total = 0
    for b in x:
        total = 256 * total + b
    return total


def to_byte(x, n):
    """Algorithm 3"""
    out = bytearray(n)
    for i in range(n):
        out[n - 1 - i] = x % 256
        x //= 256
    return bytes(out)


def base_2b(x, b, out_len):
    """Algorithm 4"""
    i = bits = total = 0
    out = []
    for _ in range(out_len):
        while bits < b:
            total = (total << 8) + x[i]
            i += 1
            bits += 8
        bits -= b
        out.append((total >> bits) % (1 << b))
    return out


class Adrs:
    """the 32-byte address of section 4.2: layer 4 || tree 12 || type 4 || 12"""

    def __init__(self, data=None):
        self.b = bytearray(32) if data is None else bytearray(data)

    def copy(self):
        return Adrs(self.b)

    def set_layer(self, v):
        self.b[0:4] = to_byte(v, 4)

    def set_tree(self, v):
        self.b[4:16] = to_byte(v, 12)

    def set_type_and_clear(self, v):
        self.b[16:20] = to_byte(v, 4)
        self.b[20:32] = bytes(12)

    def set_keypair(self, v):
        self.b[20:24] = to_byte(v, 4)

    def get_keypair(self):
        return to_int(self.b[20:24])

    def set_chain(self, v):
        self.b[24:28] = to_byte(v, 4)

    set_tree_height = set_chain

    def set_hash(self, v):
        self.b[28:32] = to_byte(v, 4)

    set_tree_index = set_hash

    def get_tree_index(self):
        return to_int(self.b[28:32])


# ---- section 11.1: the hash functions -----------------------------------------------------------------------------------------------------------------------

def _shake(data, n):
    return hashlib.shake_256(data).digest(n)


def h_msg(p, r, pk_seed, pk_root, msg):
    return _shake(r + pk_seed + pk_root + msg, _set(p).m)


def prf(p, pk_seed, sk_seed, adrs):
    return _shake(pk_seed + adrs.b + sk_seed, _set(p).n)


def prf_msg(p, sk_prf, opt_rand, msg):
    return _shake(sk_prf + opt_rand + msg, _set(p).n)


def F(p, pk_seed, adrs, m1):
    return _shake(pk_seed + adrs.b + m1, _set(p).n)


H = F                                                                      # over a 2 n byte message
T = F                                                                      # over an l n byte message


# ---- section 5: WOTS+ -----------------------------------------------------------------------------------------------------------------------------------

def chain(p, x, i, s, pk_seed, adrs):
    """Algorithm 5"""
    tmp = x
    for j in range(i, i + s):
        adrs.set_hash(j)
        tmp = F(p, pk_seed, adrs, tmp)
    return tmp


def wots_pkgen(p, sk_seed, pk_seed, adrs):
    """Algorithm 6"""
    sk_adrs = adrs.copy()
    sk_adrs.set_type_and_clear(WOTS_PRF)
    sk_adrs.set_keypair(adrs.get_keypair())
    tmp = b""
    for i in range(wots_len(p)[2]):
        sk_adrs.set_chain(i)
        sk = prf(p, pk_seed, sk_seed, sk_adrs)
        adrs.set_chain(i)
        tmp += chain(p, sk, 0, W - 1, pk_seed, adrs)
    pk_adrs = adrs.copy()
    pk_adrs.set_type_and_clear(WOTS_PK)
    pk_adrs.set_keypair(adrs.get_keypair())
    return T(p, pk_seed, pk_adrs, tmp)


def wots_digits(p, m1):
    """lines 1 to 7 of Algorithms 7 and 8: the len base-w digits of the message and its checksum"""
    len1, len2, _ = wots_len(p)
    msg = base_2b(m1, LG_W, len1)
    csum = sum(W - 1 - v for v in msg)
    csum <<= (8 - (len2 * LG_W) % 8) % 8
    return msg + base_2b(to_byte(csum, (len2 * LG_W + 7) // 8), LG_W, len2)


def wots_sign(p, m1, sk_seed, pk_seed, adrs):
    """Algorithm 7"""
    msg = wots_digits(p, m1)
    sk_adrs = adrs.copy()
    sk_adrs.set_type_and_clear(WOTS_PRF)
    sk_adrs.set_keypair(adrs.get_keypair())
    sig = b""
    for i, digit in enumerate(msg):
        sk_adrs.set_chain(i)
        sk = prf(p, pk_seed, sk_seed, sk_adrs)
        adrs.set_chain(i)
        sig += chain(p, sk, 0, digit, pk_seed, adrs)
    return sig


def wots_pk_from_sig(p, sig, m1, pk_seed, adrs):
    """Algorithm 8"""
    n = _set(p).n
    msg = wots_digits(p, m1)
    tmp = b""
    for i, digit in enumerate(msg):
        adrs.set_chain(i)
        tmp += chain(p, sig[i * n:(i + 1) * n], digit, W - 1 - digit, pk_seed, adrs)
    pk_adrs = adrs.copy()
    pk_adrs.set_type_and_clear(WOTS_PK)
    pk_adrs.set_keypair(adrs.get_keypair())
    return T(p, pk_seed, pk_adrs, tmp)


# ---- section 6: XMSS ------------------------------------------------------------------------------------------------------------------------------------

def xmss_node(p, sk_seed, i, z, pk_seed, adrs):
    """Algorithm 9"""
    if z == 0:
        adrs.set_type_and_clear(WOTS_HASH)
        adrs.set_keypair(i)
        return wots_pkgen(p, sk_seed, pk_seed, adrs)
    lnode = xmss_node(p, sk_seed, 2 * i, z - 1, pk_seed, adrs)
    rnode = xmss_node(p, sk_seed, 2 * i + 1, z - 1, pk_seed, adrs)
    adrs.set_type_and_clear(TREE)
    adrs.set_tree_height(z)
    adrs.set_tree_index(i)
    return H(p, pk_seed, adrs, lnode + rnode)


def xmss_sign(p, m1, sk_seed, idx, pk_seed, adrs):
    """Algorithm 10"""
    s = _set(p)
    auth = b""
    for j in range(s.hp):
        k = (idx >> j) ^ 1
        auth += xmss_node(p, sk_seed, k, j, pk_seed, adrs)
    adrs.set_type_and_clear(WOTS_HASH)
    adrs.set_keypair(idx)
    return wots_sign(p, m1, sk_seed, pk_seed, adrs) + auth


def xmss_pk_from_sig(p, idx, sig_xmss, m1, pk_seed, adrs):
    """Algorithm 11"""
    s = _set(p)
    n, ln = s.n, wots_len(p)[2]
    adrs.set_type_and_clear(WOTS_HASH)
    adrs.set_keypair(idx)
    sig, auth = sig_xmss[:ln * n], sig_xmss[ln * n:]
    node = wots_pk_from_sig(p, sig, m1, pk_seed, adrs)
    adrs.set_type_and_clear(TREE)
    adrs.set_tree_index(idx)
    for k in range(s.hp):
        adrs.set_tree_height(k + 1)
        sib = auth[k * n:(k + 1) * n]
        if (idx >> k) % 2 == 0:
            adrs.set_tree_index(adrs.get_tree_index() // 2)
            node = H(p, pk_seed, adrs, node + sib)
        else:
            adrs.set_tree_index((adrs.get_tree_index() - 1) // 2)
            node = H(p, pk_seed, adrs, sib + node)
    return node


# ---- section 7: the hypertree ---------------------------------------------------------------------------------------------------------------------------

def ht_sign(p, m1, sk_seed, pk_seed, idx_tree, idx_leaf):
    """Algorithm 12"""
    s = _set(p)
    adrs = Adrs()
    adrs.set_tree(idx_tree)
    sig_tmp = xmss_sign(p, m1, sk_seed, idx_leaf, pk_seed, adrs)
    sig_ht = sig_tmp
    root = xmss_pk_from_sig(p, idx_leaf, sig_tmp, m1, pk_seed, adrs)
    for j in range(1, s.d):
        idx_leaf = idx_tree % (1 << s.hp)
        idx_tree >>= s.hp
        adrs.set_layer(j)
        adrs.set_tree(idx_tree)
        sig_tmp = xmss_sign(p, root, sk_seed, idx_leaf, pk_seed, adrs)
        sig_ht += sig_tmp
        if j < s.d - 1:
            root = xmss_pk_from_sig(p, idx_leaf, sig_tmp, root, pk_seed, adrs)
    return sig_ht


def ht_verify(p, m1, sig_ht, pk_seed, idx_tree, idx_leaf, pk_root):
    """Algorithm 13"""
    s = _set(p)
    step = (s.hp + wots_len(p)[2]) * s.n
    adrs = Adrs()
    adrs.set_tree(idx_tree)
    node = xmss_pk_from_sig(p, idx_leaf, sig_ht[:step], m1, pk_seed, adrs)
    for j in range(1, s.d):
        idx_leaf = idx_tree % (1 << s.hp)
        idx_tree >>= s.hp
        adrs.set_layer(j)
        adrs.set_tree(idx_tree)
        node = xmss_pk_from_sig(p, idx_leaf, sig_ht[j * step:(j + 1) * step], node, pk_seed, adrs)
    return node == pk_root


# ---- section 8: FORS ------------------------------------------------------------------------------------------------------------------------------------

def fors_sk_gen(p, sk_seed, pk_seed, adrs, idx):
    """Algorithm 14"""
    sk_adrs = adrs.copy()
    sk_adrs.set_type_and_clear(FORS_PRF)
    sk_adrs.set_keypair(adrs.get_keypair())
    sk_adrs.set_tree_index(idx)
    return prf(p, pk_seed, sk_seed, sk_adrs)


def fors_node(p, sk_seed, i, z, pk_seed, adrs):
    """Algorithm 15"""
    if z == 0:
        sk = fors_sk_gen(p, sk_seed, pk_seed, adrs, i)
        adrs.set_tree_height(0)
        adrs.set_tree_index(i)
        return F(p, pk_seed, adrs, sk)
    lnode = fors_node(p, sk_seed, 2 * i, z - 1, pk_seed, adrs)
    rnode = fors_node(p, sk_seed, 2 * i + 1, z - 1, pk_seed, adrs)
    adrs.set_tree_height(z)
    adrs.set_tree_index(i)
    return H(p, pk_seed, adrs, lnode + rnode)


def fors_sign(p, md, sk_seed, pk_seed, adrs):
    """Algorithm 16"""
    s = _set(p)
    sig = b""
    indices = base_2b(md, s.a, s.k)
    for i in range(s.k):
        sig += fors_sk_gen(p, sk_seed, pk_seed, adrs, (i << s.a) + indices[i])
        for j in range(s.a):
            t = (indices[i] >> j) ^ 1
            sig += fors_node(p, sk_seed, (i << (s.a - j)) + t, j, pk_seed, adrs)
    return sig


def fors_pk_from_sig(p, sig_fors, md, pk_seed, adrs):
    """Algorithm 17"""
    s = _set(p)
    n = s.n
    indices = base_2b(md, s.a, s.k)
    root = b""
    for i in range(s.k):
        at = i * (s.a + 1) * n
        sk = sig_fors[at:at + n]
        adrs.set_tree_height(0)
        adrs.set_tree_index((i << s.a) + indices[i])
        node = F(p, pk_seed, adrs, sk)
        auth = sig_fors[at + n:at + (s.a + 1) * n]
        for j in range(s.a):
            adrs.set_tree_height(j + 1)
            sib = auth[j * n:(j + 1) * n]
            if (indices[i] >> j) % 2 == 0:
                adrs.set_tree_index(adrs.get_tree_index() // 2)
                node = H(p, pk_seed, adrs, node + sib)
            else:
                adrs.set_tree_index((adrs.get_tree_index() - 1) // 2)
                node = H(p, pk_seed, adrs, sib + node)
        root += node
    pk_adrs = adrs.copy()
    pk_adrs.set_type_and_clear(FORS_ROOTS)
    pk_adrs.set_keypair(adrs.get_keypair())
    return T(p, pk_seed, pk_adrs, root)


# ---- section 9: SLH-DSA, internal -------------------------------------------------------------------------------------------------------------------------

def keygen_internal(p, sk_seed, sk_prf, pk_seed):
    """Algorithm 18: (sk, pk)"""
    s = _set(p)
    adrs = Adrs()
    adrs.set_layer(s.d - 1)
    root = xmss_node(p, sk_seed, 0, s.hp, pk_seed, adrs)
    return sk_seed + sk_prf + pk_seed + root, pk_seed + root


def split_digest(p, digest):
    """lines 6 to 10 of Algorithm 19 = lines 8 to 12 of Algorithm 20: (md, idx_tree, idx_leaf)"""
    s = _set(p)
    c1, c2, c3 = (s.k * s.a + 7) // 8, (s.h - s.hp + 7) // 8, (s.hp + 7) // 8
    md = digest[:c1]
    idx_tree = to_int(digest[c1:c1 + c2]) % (1 << (s.h - s.hp))
    idx_leaf = to_int(digest[c1 + c2:c1 + c2 + c3]) % (1 << s.hp)
    return md, idx_tree, idx_leaf


def sign_internal(p, msg, sk, addrnd=None):
    """Algorithm 19; addrnd None: the deterministic variant (opt_rand = PK.seed)"""
    s = _set(p)
    n = s.n
    sk_seed, sk_prf, pk_seed, pk_root = (sk[i * n:(i + 1) * n] for i in range(4))
    opt_rand = pk_seed if addrnd is None else addrnd
    r = prf_msg(p, sk_prf, opt_rand, msg)
    md, idx_tree, idx_leaf = split_digest(p, h_msg(p, r, pk_seed, pk_root, msg))
    adrs = Adrs()
    adrs.set_tree(idx_tree)
    adrs.set_type_and_clear(FORS_TREE)
    adrs.set_keypair(idx_leaf)
    sig_fors = fors_sign(p, md, sk_seed, pk_seed, adrs)
    pk_fors = fors_pk_from_sig(p, sig_fors, md, pk_seed, adrs)
    return r + sig_fors + ht_sign(p, pk_fors, sk_seed, pk_seed, idx_tree, idx_leaf)


def verify_internal(p, msg, sig, pk):
    """Algorithm 20"""
    s = _set(p)
    n = s.n
    if len(sig) != sizes(p)["sig"] or len(pk) != 2 * n:
        return False
    pk_seed, pk_root = pk[:n], pk[n:]
    r = sig[:n]
    fors_len = s.k * (1 + s.a) * n
    sig_fors, sig_ht = sig[n:n + fors_len], sig[n + fors_len:]
    md, idx_tree, idx_leaf = split_digest(p, h_msg(p, r, pk_seed, pk_root, msg))
    adrs = Adrs()
    adrs.set_tree(idx_tree)
    adrs.set_type_and_clear(FORS_TREE)
    adrs.set_keypair(idx_leaf)
    pk_fors = fors_pk_from_sig(p, sig_fors, md, pk_seed, adrs)
    return ht_verify(p, pk_fors, sig_ht, pk_seed, idx_tree, idx_leaf, pk_root)


# ---- section 10: SLH-DSA, external (pure) -----------------------------------------------------------------------------------------------------------------

def m_prime(msg, ctx=b""):
    return to_byte(0, 1) + to_byte(len(ctx), 1) + bytes(ctx) + bytes(msg)


def sign(p, msg, ctx, sk, addrnd=None):
    """Algorithm 22"""
    if len(ctx) > 255:
        raise ValueError("ctx longer than 255 bytes")
    return sign_internal(p, m_prime(msg, ctx), sk, addrnd)


def verify(p, msg, sig, ctx, pk):
    """Algorithm 24"""
    if len(ctx) > 255:
        return False
    return verify_internal(p, m_prime(msg, ctx), sig, pk)


def regions(p):
    """byte ranges of a signature: {"R": (lo, hi), "fors_sk": [per tree], "fors_auth": [per tree], "wots": [per layer], "auth": [per layer]}"""
    s = _set(p)
    n, ln = s.n, wots_len(p)[2]
    out = {"R": (0, n), "fors_sk": [], "fors_auth": [], "wots": [], "auth": []}
    at = n
    for _ in range(s.k):
        out["fors_sk"].append((at, at + n))
        out["fors_auth"].append((at + n, at + (1 + s.a) * n))
        at += (1 + s.a) * n
    for _ in range(s.d):
        out["wots"].append((at, at + ln * n))
        out["auth"].append((at + ln * n, at + (ln + s.hp) * n))
        at += (ln + s.hp) * n
    assert at == sizes(p)["sig"]
    return out
