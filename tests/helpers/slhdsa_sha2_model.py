"""A pure-Python model of SLH-DSA (FIPS 205, August 2024) that takes the hash family as a parameter, over hashlib and hmac: Algorithms 5 to 20 and 22
to 24 written once from the standard's pseudocode as methods of Scheme(set, family), with the two families of section 11 beside it:

  Sha2     section 11.2: F, PRF (and, at n = 16, H and T_l) = Trunc_n(SHA-256(PK.seed || toByte(0, 64 - n) || ADRSc || M)); at n = 24, 32 H and T_l on
           SHA-512 with toByte(0, 128 - n); PRF_msg = Trunc_n(HMAC(SK.prf, opt_rand || M)); H_msg = MGF1(R || PK.seed || Hash(R || PK.seed || PK.root || M),
           m); ADRSc the 22-byte compressed address
  Shake    section 11.1, every function SHAKE256 over the 32-byte address

The SHA-2 library code is compared with Scheme(set, Sha2).  Scheme(set, Shake) must reproduce tests/helpers/slhdsa_model.py byte for byte
(tests/test_slhdsa_sha2_model_cpu.py): the algorithms here are then the pinned ones, and what is new is section 11.2's functions alone.  The hash-free
helpers (Adrs, base_2b, wots_len, sizes, regions, split_digest, wots_digits) are those of slhdsa_model.py.  There is no other SLH-DSA implementation, no
ACVP vector and no OpenSSL with SLH-DSA on the hosts the suite runs on: "byte-exact" means equal to this model.

PARAMS holds the six SHA-2 sets of Table 2, "toy" (n = 16) and "toy24" (n = 24: H and T_l on SHA-512), small enough to walk every leaf."""
import hashlib
import hmac

from tests.helpers import slhdsa_model as S
from tests.helpers.slhdsa_model import FORS_PRF, FORS_ROOTS, FORS_TREE, TREE, WOTS_HASH, WOTS_PK, WOTS_PRF, Adrs, Set, W, base_2b, to_byte  # noqa: F401

PARAMS = {
    "SLH-DSA-SHA2-128s": Set(16, 63, 7, 9, 12, 14, 30),
    "SLH-DSA-SHA2-128f": Set(16, 66, 22, 3, 6, 33, 34),
    "SLH-DSA-SHA2-192s": Set(24, 63, 7, 9, 14, 17, 39),
    "SLH-DSA-SHA2-192f": Set(24, 66, 22, 3, 8, 33, 42),
    "SLH-DSA-SHA2-256s": Set(32, 64, 8, 8, 14, 22, 47),
    "SLH-DSA-SHA2-256f": Set(32, 68, 17, 4, 9, 35, 49),
    "toy": Set(16, 4, 2, 2, 3, 4, 4),
    "toy24": Set(24, 4, 2, 2, 3, 4, 4),
}
NAMES = [n for n in PARAMS if not n.startswith("toy")]
IDS = {name: i for i, name in enumerate(NAMES)}                           # the library's numbers of the sets


def _set(p):
    return PARAMS[p] if isinstance(p, str) else p


def wots_len(p):
    return S.wots_len(_set(p))


def sizes(p):
    return S.sizes(_set(p))


def regions(p):
    return S.regions(_set(p))


def split_digest(p, digest):
    return S.split_digest(_set(p), digest)


def wots_digits(p, m1):
    return S.wots_digits(_set(p), m1)


def adrs_c(adrs):
    """the compressed address of section 11.2: ADRS[3] || ADRS[8:16] || ADRS[19] || ADRS[20:32]"""
    b = bytes(adrs.b)
    return b[3:4] + b[8:16] + b[19:20] + b[20:32]


def mgf1(hash_fn, seed, length):
    """MGF1 of NIST SP 800-56B rev. 2, section 7.2.2.2"""
    out = b""
    counter = 0
    while len(out) < length:
        out += hash_fn(seed + to_byte(counter, 4)).digest()
        counter += 1
    return out[:length]


class Sha2:
    """section 11.2.1 (n = 16) and 11.2.2 (n = 24, 32)"""

    def __init__(self, s):
        self.s = s
        self.big, self.block = (hashlib.sha512, 128) if s.n > 16 else (hashlib.sha256, 64)

    def h_msg(self, r, pk_seed, pk_root, msg):
        return mgf1(self.big, r + pk_seed + self.big(r + pk_seed + pk_root + msg).digest(), self.s.m)

    def prf(self, pk_seed, sk_seed, adrs):
        return hashlib.sha256(pk_seed + bytes(64 - self.s.n) + adrs_c(adrs) + sk_seed).digest()[:self.s.n]

    def prf_msg(self, sk_prf, opt_rand, msg):
        return hmac.new(sk_prf, opt_rand + msg, self.big).digest()[:self.s.n]

    def F(self, pk_seed, adrs, m1):
        return hashlib.sha256(pk_seed + bytes(64 - self.s.n) + adrs_c(adrs) + m1).digest()[:self.s.n]

    def H(self, pk_seed, adrs, m2):
        return self.big(pk_seed + bytes(self.block - self.s.n) + adrs_c(adrs) + m2).digest()[:self.s.n]

    T = H


class Shake:
    """section 11.1"""

    def __init__(self, s):
        self.s = s

    def _shake(self, data, n):
        return hashlib.shake_256(data).digest(n)

    def h_msg(self, r, pk_seed, pk_root, msg):
        return self._shake(r + pk_seed + pk_root + msg, self.s.m)

    def prf(self, pk_seed, sk_seed, adrs):
        return self._shake(pk_seed + bytes(adrs.b) + sk_seed, self.s.n)

    def prf_msg(self, sk_prf, opt_rand, msg):
        return self._shake(sk_prf + opt_rand + msg, self.s.n)

    def F(self, pk_seed, adrs, m1):
        return self._shake(pk_seed + bytes(adrs.b) + m1, self.s.n)

    H = F
    T = F


class Scheme:
    """FIPS 205 over one parameter set and one hash family"""

    def __init__(self, p, family=Sha2):
        self.s = _set(p)
        self.f = family(self.s)
        self.n, self.len = self.s.n, wots_len(self.s)[2]

    # ---- section 5: WOTS+ ----
    def chain(self, x, i, s, pk_seed, adrs):
        """Algorithm 5"""
        tmp = x
        for j in range(i, i + s):
            adrs.set_hash(j)
            tmp = self.f.F(pk_seed, adrs, tmp)
        return tmp

    def _sub(self, adrs, kind):
        out = adrs.copy()
        out.set_type_and_clear(kind)
        out.set_keypair(adrs.get_keypair())
        return out

    def wots_pkgen(self, sk_seed, pk_seed, adrs):
        """Algorithm 6"""
        sk_adrs = self._sub(adrs, WOTS_PRF)
        tmp = b""
        for i in range(self.len):
            sk_adrs.set_chain(i)
            sk = self.f.prf(pk_seed, sk_seed, sk_adrs)
            adrs.set_chain(i)
            tmp += self.chain(sk, 0, W - 1, pk_seed, adrs)
        return self.f.T(pk_seed, self._sub(adrs, WOTS_PK), tmp)

    def wots_sign(self, m1, sk_seed, pk_seed, adrs):
        """Algorithm 7"""
        sk_adrs = self._sub(adrs, WOTS_PRF)
        sig = b""
        for i, digit in enumerate(wots_digits(self.s, m1)):
            sk_adrs.set_chain(i)
            sk = self.f.prf(pk_seed, sk_seed, sk_adrs)
            adrs.set_chain(i)
            sig += self.chain(sk, 0, digit, pk_seed, adrs)
        return sig

    def wots_pk_from_sig(self, sig, m1, pk_seed, adrs):
        """Algorithm 8"""
        n = self.n
        tmp = b""
        for i, digit in enumerate(wots_digits(self.s, m1)):
            adrs.set_chain(i)
            tmp += self.chain(sig[i * n:(i + 1) * n], digit, W - 1 - digit, pk_seed, adrs)
        return self.f.T(pk_seed, self._sub(adrs, WOTS_PK), tmp)

    # ---- section 6: XMSS ----
    def xmss_node(self, sk_seed, i, z, pk_seed, adrs):
        """Algorithm 9"""
        if z == 0:
            adrs.set_type_and_clear(WOTS_HASH)
            adrs.set_keypair(i)
            return self.wots_pkgen(sk_seed, pk_seed, adrs)
        lnode = self.xmss_node(sk_seed, 2 * i, z - 1, pk_seed, adrs)
        rnode = self.xmss_node(sk_seed, 2 * i + 1, z - 1, pk_seed, adrs)
        adrs.set_type_and_clear(TREE)
        adrs.set_tree_height(z)
        adrs.set_tree_index(i)
        return self.f.H(pk_seed, adrs, lnode + rnode)

    def xmss_sign(self, m1, sk_seed, idx, pk_seed, adrs):
        """Algorithm 10"""
        auth = b""
        for j in range(self.s.hp):
            auth += self.xmss_node(sk_seed, (idx >> j) ^ 1, j, pk_seed, adrs)
        adrs.set_type_and_clear(WOTS_HASH)
        adrs.set_keypair(idx)
        return self.wots_sign(m1, sk_seed, pk_seed, adrs) + auth

    def _climb(self, node, index, auth, pk_seed, adrs):
        """the path loops of Algorithms 11 and 17: adrs has its tree index set to `index`'s node"""
        n = self.n
        for k in range(len(auth) // n):
            adrs.set_tree_height(k + 1)
            sib = auth[k * n:(k + 1) * n]
            if (index >> k) % 2 == 0:
                adrs.set_tree_index(adrs.get_tree_index() // 2)
                node = self.f.H(pk_seed, adrs, node + sib)
            else:
                adrs.set_tree_index((adrs.get_tree_index() - 1) // 2)
                node = self.f.H(pk_seed, adrs, sib + node)
        return node

    def xmss_pk_from_sig(self, idx, sig_xmss, m1, pk_seed, adrs):
        """Algorithm 11"""
        cut = self.len * self.n
        adrs.set_type_and_clear(WOTS_HASH)
        adrs.set_keypair(idx)
        node = self.wots_pk_from_sig(sig_xmss[:cut], m1, pk_seed, adrs)
        adrs.set_type_and_clear(TREE)
        adrs.set_tree_index(idx)
        return self._climb(node, idx, sig_xmss[cut:], pk_seed, adrs)

    # ---- section 7: the hypertree ----
    def ht_sign(self, m1, sk_seed, pk_seed, idx_tree, idx_leaf):
        """Algorithm 12"""
        s = self.s
        adrs = Adrs()
        adrs.set_tree(idx_tree)
        sig_tmp = self.xmss_sign(m1, sk_seed, idx_leaf, pk_seed, adrs)
        sig_ht = sig_tmp
        root = self.xmss_pk_from_sig(idx_leaf, sig_tmp, m1, pk_seed, adrs)
        for j in range(1, s.d):
            idx_leaf = idx_tree % (1 << s.hp)
            idx_tree >>= s.hp
            adrs.set_layer(j)
            adrs.set_tree(idx_tree)
            sig_tmp = self.xmss_sign(root, sk_seed, idx_leaf, pk_seed, adrs)
            sig_ht += sig_tmp
            if j < s.d - 1:
                root = self.xmss_pk_from_sig(idx_leaf, sig_tmp, root, pk_seed, adrs)
        return sig_ht

    def ht_root(self, m1, sig_ht, pk_seed, idx_tree, idx_leaf):
        """Algorithm 13 up to its comparison: the root the signature leads to"""
        s = self.s
        step = (s.hp + self.len) * s.n
        adrs = Adrs()
        adrs.set_tree(idx_tree)
        node = self.xmss_pk_from_sig(idx_leaf, sig_ht[:step], m1, pk_seed, adrs)
        for j in range(1, s.d):
            idx_leaf = idx_tree % (1 << s.hp)
            idx_tree >>= s.hp
            adrs.set_layer(j)
            adrs.set_tree(idx_tree)
            node = self.xmss_pk_from_sig(idx_leaf, sig_ht[j * step:(j + 1) * step], node, pk_seed, adrs)
        return node

    def ht_verify(self, m1, sig_ht, pk_seed, idx_tree, idx_leaf, pk_root):
        """Algorithm 13"""
        return self.ht_root(m1, sig_ht, pk_seed, idx_tree, idx_leaf) == pk_root

    # ---- section 8: FORS ----
    def fors_sk_gen(self, sk_seed, pk_seed, adrs, idx):
        """Algorithm 14"""
        sk_adrs = self._sub(adrs, FORS_PRF)
        sk_adrs.set_tree_index(idx)
        return self.f.prf(pk_seed, sk_seed, sk_adrs)

    def fors_node(self, sk_seed, i, z, pk_seed, adrs):
        """Algorithm 15"""
        if z == 0:
            sk = self.fors_sk_gen(sk_seed, pk_seed, adrs, i)
            adrs.set_tree_height(0)
            adrs.set_tree_index(i)
            return self.f.F(pk_seed, adrs, sk)
        lnode = self.fors_node(sk_seed, 2 * i, z - 1, pk_seed, adrs)
        rnode = self.fors_node(sk_seed, 2 * i + 1, z - 1, pk_seed, adrs)
        adrs.set_tree_height(z)
        adrs.set_tree_index(i)
        return self.f.H(pk_seed, adrs, lnode + rnode)

    def fors_sign(self, md, sk_seed, pk_seed, adrs):
        """Algorithm 16"""
        s = self.s
        sig = b""
        indices = base_2b(md, s.a, s.k)
        for i in range(s.k):
            sig += self.fors_sk_gen(sk_seed, pk_seed, adrs, (i << s.a) + indices[i])
            for j in range(s.a):
                t = (indices[i] >> j) ^ 1
                sig += self.fors_node(sk_seed, (i << (s.a - j)) + t, j, pk_seed, adrs)
        return sig

    def fors_pk_from_sig(self, sig_fors, md, pk_seed, adrs):
        """Algorithm 17"""
        s, n = self.s, self.n
        indices = base_2b(md, s.a, s.k)
        root = b""
        for i in range(s.k):
            at = i * (s.a + 1) * n
            adrs.set_tree_height(0)
            adrs.set_tree_index((i << s.a) + indices[i])
            node = self.f.F(pk_seed, adrs, sig_fors[at:at + n])
            root += self._climb(node, indices[i], sig_fors[at + n:at + (s.a + 1) * n], pk_seed, adrs)
        return self.f.T(pk_seed, self._sub(adrs, FORS_ROOTS), root)

    # ---- section 9: SLH-DSA, internal ----
    def keygen_internal(self, sk_seed, sk_prf, pk_seed):
        """Algorithm 18: (sk, pk)"""
        adrs = Adrs()
        adrs.set_layer(self.s.d - 1)
        root = self.xmss_node(sk_seed, 0, self.s.hp, pk_seed, adrs)
        return sk_seed + sk_prf + pk_seed + root, pk_seed + root

    def _fors_adrs(self, idx_tree, idx_leaf):
        adrs = Adrs()
        adrs.set_tree(idx_tree)
        adrs.set_type_and_clear(FORS_TREE)
        adrs.set_keypair(idx_leaf)
        return adrs

    def sign_internal(self, msg, sk, addrnd=None):
        """Algorithm 19; addrnd None: the deterministic variant (opt_rand = PK.seed)"""
        n = self.n
        sk_seed, sk_prf, pk_seed, pk_root = (sk[i * n:(i + 1) * n] for i in range(4))
        opt_rand = pk_seed if addrnd is None else addrnd
        r = self.f.prf_msg(sk_prf, opt_rand, msg)
        md, idx_tree, idx_leaf = split_digest(self.s, self.f.h_msg(r, pk_seed, pk_root, msg))
        adrs = self._fors_adrs(idx_tree, idx_leaf)
        sig_fors = self.fors_sign(md, sk_seed, pk_seed, adrs)
        pk_fors = self.fors_pk_from_sig(sig_fors, md, pk_seed, adrs)
        return r + sig_fors + self.ht_sign(pk_fors, sk_seed, pk_seed, idx_tree, idx_leaf)

    def root_from_sig(self, msg, sig, pk):
        """Algorithm 20 up to the comparison of Algorithm 13: the node that is compared with PK.root"""
        s, n = self.s, self.n
        pk_seed, pk_root = pk[:n], pk[n:]
        fors_len = s.k * (1 + s.a) * n
        md, idx_tree, idx_leaf = split_digest(s, self.f.h_msg(sig[:n], pk_seed, pk_root, msg))
        pk_fors = self.fors_pk_from_sig(sig[n:n + fors_len], md, pk_seed, self._fors_adrs(idx_tree, idx_leaf))
        return self.ht_root(pk_fors, sig[n + fors_len:], pk_seed, idx_tree, idx_leaf)

    def verify_internal(self, msg, sig, pk):
        """Algorithm 20"""
        if len(sig) != sizes(self.s)["sig"] or len(pk) != 2 * self.n:
            return False
        return self.root_from_sig(msg, sig, pk) == pk[self.n:]

    # ---- section 10: SLH-DSA, external (pure) ----
    def sign(self, msg, ctx, sk, addrnd=None):
        """Algorithm 22"""
        if len(ctx) > 255:
            raise ValueError("ctx longer than 255 bytes")
        return self.sign_internal(S.m_prime(msg, ctx), sk, addrnd)

    def verify(self, msg, sig, ctx, pk):
        """Algorithm 24"""
        if len(ctx) > 255:
            return False
        return self.verify_internal(S.m_prime(msg, ctx), sig, pk)


# ---- the module-level forms the tests use, shaped like slhdsa_model's, over section 11.2 --------------------------------------------------------------------

def keygen_internal(p, sk_seed, sk_prf, pk_seed):
    return Scheme(p).keygen_internal(sk_seed, sk_prf, pk_seed)


def sign_internal(p, msg, sk, addrnd=None):
    return Scheme(p).sign_internal(msg, sk, addrnd)


def verify_internal(p, msg, sig, pk):
    return Scheme(p).verify_internal(msg, sig, pk)


def sign(p, msg, ctx, sk, addrnd=None):
    return Scheme(p).sign(msg, ctx, sk, addrnd)


def verify(p, msg, sig, ctx, pk):
    return Scheme(p).verify(msg, sig, ctx, pk)
