// psf_slhdsa_core.hpp -- FIPS 205's own part of SLH-DSA for the SHAKE parameter sets, over the sponge of psf_keccak_core.hpp: the 32-byte ADRS and its
// setters, F / H / PRF as ONE permutation each, T_l over a word getter, H_msg over a three-part reader, base_2b and the WOTS+ checksum, the chain, the
// chain end of wots_pkGen, the node steps of XMSS and FORS, and the split of the digest into (md, idx_tree, idx_leaf).
//
// An n-byte string is NW = n / 8 little-endian 64-bit words (n = 16, 24, 32), so PK.seed || ADRS || M is whole words of the state: F fills words
// [0, 2 NW + 4) and H words [0, 3 NW + 4) of the one block (at most 16 of the 17 words of the SHAKE256 rate), every index a constant.  The padded block is
// built in registers; no byte reader runs in the chain loop.  Whatever is indexed by a run-time value (a digit of a message, an index of md, a node of an
// authentication path) is read through a getter from memory, never from a register array.
//
// Written over the Ops back ends: the device kernels of psf_slhdsa.hip and tests/cpp/slhdsa_host_check.cpp (g++, PlainOps) compile this same text.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "psf_keccak_core.hpp"

namespace psf {
namespace slh {

// ---- the parameter sets (FIPS 205 Table 2; lg_w = 4, len = 2 n + 3) -------------------------------------------------------------------------------------
struct Params { uint32_t n, h, d, hp, a, k, m; };
constexpr int kSets = 6;
constexpr Params kParams[kSets] = {{16, 63, 7, 9, 12, 14, 30}, {16, 66, 22, 3, 6, 33, 34}, {24, 63, 7, 9, 14, 17, 39},
                                   {24, 66, 22, 3, 8, 33, 42}, {32, 64, 8, 8, 14, 22, 47}, {32, 68, 17, 4, 9, 35, 49}};
#if defined(__HIPCC__)
#define PSF_SLH_HD __host__ __device__ inline                             // the sizes: asked by the host code of psf_slhdsa.hip too
#else
#define PSF_SLH_HD inline
#endif
PSF_SLH_HD constexpr uint32_t wots_len(uint32_t n) { return 2 * n + 3; }
PSF_SLH_HD constexpr size_t sig_bytes(const Params& p) { return (size_t)(1 + p.k * (1 + p.a) + p.h + p.d * wots_len(p.n)) * p.n; }
constexpr uint32_t kW = 16;                                               // the Winternitz parameter: chains of w - 1 = 15 steps

enum : uint32_t { WOTS_HASH = 0, WOTS_PK = 1, TREE = 2, FORS_TREE = 3, FORS_ROOTS = 4, WOTS_PRF = 5, FORS_PRF = 6 };

// ---- ADRS -----------------------------------------------------------------------------------------------------------------------------------------------
// layer 4 || tree 12 || type 4 || keypair 4 || chain or tree height 4 || hash or tree index 4, every field big-endian; as four words of the state:
// w[0] = layer and the top 4 bytes of the tree address (always zero: a tree address is below 2^64), w[1] = the tree address, w[2] = type and keypair,
// w[3] = the last two fields.
PSF_KC_FN constexpr uint32_t be32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }
PSF_KC_FN constexpr uint64_t be64(uint64_t v) { return ((uint64_t)be32((uint32_t)v) << 32) | be32((uint32_t)(v >> 32)); }
struct Adrs {
  uint64_t w[4];
  PSF_KC_FN void init(uint32_t layer, uint64_t tree, uint32_t type, uint32_t keypair) {
    w[0] = be32(layer);
    w[1] = be64(tree);
    w[2] = (uint64_t)be32(type) | ((uint64_t)be32(keypair) << 32);
    w[3] = 0;
  }
  PSF_KC_FN void set_type_and_clear(uint32_t type) { w[2] = be32(type); w[3] = 0; }
  PSF_KC_FN void set_keypair(uint32_t kp) { w[2] = (w[2] & 0xFFFFFFFFull) | ((uint64_t)be32(kp) << 32); }
  PSF_KC_FN void set_chain(uint32_t c) { w[3] = (w[3] & ~0xFFFFFFFFull) | be32(c); }          // also the tree height
  PSF_KC_FN void set_hash(uint32_t x) { w[3] = (w[3] & 0xFFFFFFFFull) | ((uint64_t)be32(x) << 32); }      // also the tree index
  PSF_KC_FN void set_tree_height(uint32_t z) { set_chain(z); }
  PSF_KC_FN void set_tree_index(uint32_t i) { set_hash(i); }
};

// ---- strings as words -----------------------------------------------------------------------------------------------------------------------------------
template <int NW> PSF_KC_FN void load_words(const uint8_t* p, uint64_t (&w)[NW]) {                 // no alignment asked of p
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v |= (uint64_t)p[8 * i + k] << (8 * k);
    w[i] = v;
  }
}
template <int NW> PSF_KC_FN void store_words(uint8_t* p, const uint64_t (&w)[NW]) {
#pragma unroll
  for (int i = 0; i < NW; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) p[8 * i + k] = (uint8_t)(w[i] >> (8 * k));
}

// ---- F, PRF and H: one permutation ------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kPadLast = 0x8000000000000000ull;                      // the last bit of pad10*1, in word 16 of the 17 of the rate

// out = SHAKE256(seed || adrs || m, 8 n): F; with m = SK.seed, PRF.  `out` may be `m`.
template <int NW, class Ops> PSF_KC_FN void hash_f(const uint64_t (&seed)[NW], const Adrs& a, const uint64_t (&m)[NW], uint64_t (&out)[NW]) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < NW; ++i) s[i] = seed[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[NW + i] = a.w[i];
#pragma unroll
  for (int i = 0; i < NW; ++i) s[NW + 4 + i] = m[i];
#pragma unroll
  for (int i = 2 * NW + 4; i < 25; ++i) s[i] = 0;
  s[2 * NW + 4] = kc::kDomShake;
  s[16] ^= kPadLast;
  kc::f1600<Ops>(s);
#pragma unroll
  for (int i = 0; i < NW; ++i) out[i] = s[i];
}
// out = SHAKE256(seed || adrs || l || r, 8 n): H.  `out` may be `l` or `r`.
template <int NW, class Ops>
PSF_KC_FN void hash_h(const uint64_t (&seed)[NW], const Adrs& a, const uint64_t (&l)[NW], const uint64_t (&r)[NW], uint64_t (&out)[NW]) {
  static_assert(3 * NW + 4 <= 16, "PK.seed || ADRS || two nodes and the domain byte fit one block");
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < NW; ++i) s[i] = seed[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[NW + i] = a.w[i];
#pragma unroll
  for (int i = 0; i < NW; ++i) s[NW + 4 + i] = l[i];
#pragma unroll
  for (int i = 0; i < NW; ++i) s[2 * NW + 4 + i] = r[i];
#pragma unroll
  for (int i = 3 * NW + 4; i < 25; ++i) s[i] = 0;
  s[3 * NW + 4] = kc::kDomShake;
  s[16] ^= kPadLast;
  kc::f1600<Ops>(s);
#pragma unroll
  for (int i = 0; i < NW; ++i) out[i] = s[i];
}

// ---- T_l ------------------------------------------------------------------------------------------------------------------------------------------------
// out = SHAKE256(seed || adrs || the `nwords` words get(0), get(1), ... , 8 n).  get is asked for words below nwords only, in ascending order, and the
// control flow depends on nwords alone.  The first block takes 13 - NW message words, every later one 17; when the message ends on a block edge the
// padding opens a block of its own (T_k of SLH-DSA-SHAKE-128s: 2 + 4 + 28 words are two blocks exactly).
template <int NW, class Ops, class Get>
PSF_KC_FN void hash_t(const uint64_t (&seed)[NW], const Adrs& a, size_t nwords, Get&& get, uint64_t (&out)[NW]) {
  constexpr int kRateWords = kc::kRateShake256 / 8, kFirst = kRateWords - NW - 4;
  auto padded = [&](size_t w) -> uint64_t { return w < nwords ? get(w) : (w == nwords ? (uint64_t)kc::kDomShake : 0); };
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < NW; ++i) s[i] = seed[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[NW + i] = a.w[i];
#pragma unroll
  for (int i = 0; i < kFirst; ++i) s[NW + 4 + i] = padded((size_t)i);
#pragma unroll
  for (int i = kRateWords; i < 25; ++i) s[i] = 0;
  size_t w = kFirst;                                                       // message words absorbed so far, the domain byte's word among them once w > nwords
  while (w <= nwords) {
    kc::f1600<Ops>(s);
#pragma unroll
    for (int i = 0; i < kRateWords; ++i) s[i] ^= padded(w + i);
    w += kRateWords;
  }
  s[kRateWords - 1] ^= kPadLast;
  kc::f1600<Ops>(s);
#pragma unroll
  for (int i = 0; i < NW; ++i) out[i] = s[i];
}

// ---- H_msg ----------------------------------------------------------------------------------------------------------------------------------------------
// R || PK.seed || PK.root || M as the sponge reads it: na bytes of a (R), nb of b (the public key), the rest from c (M).  No alignment is asked.
struct Cat3Reader {
  const uint8_t* a;
  const uint8_t* b;
  const uint8_t* c;
  size_t na, nb;
  PSF_KC_FN uint8_t byte(size_t pos) const { return pos < na ? a[pos] : (pos < na + nb ? b[pos - na] : c[pos - na - nb]); }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte(pos + k) << (8 * k);
    return w;
  }
};
// the first 64 bytes of H_msg(R, PK.seed, PK.root, M) as words: m <= 49 of them are the digest
template <class Ops> PSF_KC_FN void h_msg(uint32_t n, const uint8_t* r, const uint8_t* pk, const uint8_t* msg, size_t msg_len, uint64_t (&digest)[8]) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
  kc::absorb<kc::kRateShake256, Ops>(s, Cat3Reader{r, pk, msg, n, 2 * (size_t)n}, 3 * (size_t)n + msg_len, kc::kDomShake);
#pragma unroll
  for (int i = 0; i < 8; ++i) digest[i] = s[i];
}

// ---- the digest -------------------------------------------------------------------------------------------------------------------------------------------
// digest = md (ceil(k a / 8) bytes) || idx_tree (ceil((h - h') / 8) bytes, big-endian, mod 2^(h - h')) || idx_leaf (ceil(h' / 8) bytes, mod 2^h').
// h - h' is 64 for SLH-DSA-SHAKE-256f: the mask is then all ones and no shift by 64 is formed.  byte(i): byte i of the digest.
struct Split { uint64_t idx_tree; uint32_t idx_leaf; };
template <class GetByte> PSF_KC_FN Split digest_split(const Params& p, GetByte&& byte) {
  const uint32_t md_len = (p.k * p.a + 7) / 8, tree_bits = p.h - p.hp, tree_len = (tree_bits + 7) / 8, leaf_len = (p.hp + 7) / 8;
  uint64_t t = 0;
  for (uint32_t i = 0; i < tree_len; ++i) t = (t << 8) | (uint64_t)byte(md_len + i);
  if (tree_bits < 64) t &= ((uint64_t)1 << tree_bits) - 1;
  uint32_t l = 0;
  for (uint32_t i = 0; i < leaf_len; ++i) l = (l << 8) | (uint32_t)byte(md_len + tree_len + i);
  l &= (1u << p.hp) - 1;
  return Split{t, l};
}
// base_2b(X, b, out_len)[i]: bits [i b, (i + 1) b) of X, the most significant bit of a byte first; b <= 16
template <class GetByte> PSF_KC_FN uint32_t base_2b(GetByte&& byte, uint32_t b, uint32_t i) {
  uint32_t v = 0;
  for (uint32_t j = 0; j < b; ++j) {
    const uint32_t bit = i * b + j;
    v = (v << 1) | (((uint32_t)byte(bit >> 3) >> (7 - (bit & 7))) & 1u);
  }
  return v;
}
// the WOTS+ checksum of the n-byte message: sum over its 2 n base-16 digits of 15 - digit
template <class GetByte> PSF_KC_FN uint32_t wots_csum(uint32_t n, GetByte&& byte) {
  uint32_t csum = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t v = byte(j);
    csum += 2 * (kW - 1) - (v >> 4) - (v & 15u);
  }
  return csum;
}
// digit i of the len = 2 n + 3 that wots_sign and wots_pkFromSig walk: the 2 n digits of the message, then base_2b(toByte(csum << 4, 2), 4, 3)
template <class GetByte> PSF_KC_FN uint32_t wots_digit(uint32_t n, GetByte&& byte, uint32_t i) {
  if (i < 2 * n) return ((uint32_t)byte(i >> 1) >> (4 * (1 - (i & 1)))) & 15u;
  return (wots_csum(n, byte) >> (4 * (2 * n + 2 - i))) & 15u;
}

// ---- WOTS+ ----------------------------------------------------------------------------------------------------------------------------------------------
// chain(X, start, steps): v = F(PK.seed, ADRS with hash address j, v) for j = start ... start + steps - 1.  a: type WOTS_HASH with keypair and chain set.
template <int NW, class Ops> PSF_KC_FN void chain(const uint64_t (&seed)[NW], Adrs a, uint64_t (&v)[NW], uint32_t start, uint32_t steps) {
#pragma clang loop unroll(disable)
  for (uint32_t j = start; j < start + steps; ++j) {
    a.set_hash(j);
    hash_f<NW, Ops>(seed, a, v, v);
  }
}
// the public value of chain `c` of the WOTS+ key of leaf `leaf` (wots_pkGen, lines 4 to 9): PRF, then the whole chain of 15 steps, whatever the secret
template <int NW, class Ops>
PSF_KC_FN void wots_chain_end(const uint64_t (&seed)[NW], const uint64_t (&sk_seed)[NW], uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t c, uint64_t (&v)[NW]) {
  Adrs a;
  a.init(layer, tree, WOTS_PRF, leaf);
  a.set_chain(c);
  hash_f<NW, Ops>(seed, a, sk_seed, v);
  a.init(layer, tree, WOTS_HASH, leaf);
  a.set_chain(c);
  chain<NW, Ops>(seed, a, v, 0, kW - 1);
}
// chain i of wots_pkFromSig: the signature value walked from its digit to the end
template <int NW, class Ops>
PSF_KC_FN void wots_chain_from_sig(const uint64_t (&seed)[NW], uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t c, uint32_t digit, uint64_t (&v)[NW]) {
  Adrs a;
  a.init(layer, tree, WOTS_HASH, leaf);
  a.set_chain(c);
  chain<NW, Ops>(seed, a, v, digit, kW - 1 - digit);
}
// T_len over the len chain ends (get: their len NW words): the WOTS+ public key, leaf `leaf` of its XMSS tree
template <int NW, class Ops, class Get>
PSF_KC_FN void wots_pk(const uint64_t (&seed)[NW], uint32_t layer, uint64_t tree, uint32_t leaf, Get&& get, uint64_t (&out)[NW]) {
  Adrs a;
  a.init(layer, tree, WOTS_PK, leaf);
  hash_t<NW, Ops>(seed, a, (size_t)wots_len(8 * NW) * NW, get, out);
}

// ---- tree nodes -------------------------------------------------------------------------------------------------------------------------------------------
// node (height z, index i) of an XMSS tree from its children: xmss_node, lines 5 to 10
template <int NW, class Ops>
PSF_KC_FN void xmss_parent(const uint64_t (&seed)[NW], uint32_t layer, uint64_t tree, uint32_t z, uint32_t i, const uint64_t (&l)[NW], const uint64_t (&r)[NW],
                           uint64_t (&out)[NW]) {
  Adrs a;
  a.init(layer, tree, TREE, 0);
  a.set_tree_height(z);
  a.set_tree_index(i);
  hash_h<NW, Ops>(seed, a, l, r, out);
}
// one step up an authentication path (xmss_pkFromSig lines 4 to 13, fors_pkFromSig lines 9 to 19): `node` at height z with index `idx` at that height
// becomes its parent; the sibling is `auth`.  a: type TREE, or FORS_TREE with its keypair.  Both orders are formed by selection, not by a branch.
template <int NW, class Ops> PSF_KC_FN void path_step(const uint64_t (&seed)[NW], Adrs a, uint32_t z, uint32_t idx, uint64_t (&node)[NW], const uint64_t (&auth)[NW]) {
  const bool right = idx & 1u;
  uint64_t l[NW], r[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    l[i] = right ? auth[i] : node[i];
    r[i] = right ? node[i] : auth[i];
  }
  a.set_tree_height(z + 1);
  a.set_tree_index(idx >> 1);
  hash_h<NW, Ops>(seed, a, l, r, node);
}
// the root of an XMSS tree from leaf `leaf` and its h' siblings at `auth` (n bytes each)
template <int NW, class Ops>
PSF_KC_FN void xmss_root(const uint64_t (&seed)[NW], uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t hp, const uint8_t* auth, uint64_t (&node)[NW]) {
  Adrs a;
  a.init(layer, tree, TREE, 0);
#pragma clang loop unroll(disable)
  for (uint32_t z = 0; z < hp; ++z) {
    uint64_t sib[NW];
    load_words<NW>(auth + (size_t)z * 8 * NW, sib);
    path_step<NW, Ops>(seed, a, z, leaf >> z, node, sib);
  }
}
// the root of FORS tree t from its part of SIG_FORS (the secret value, then a siblings): fors_pkFromSig, lines 3 to 20
template <int NW, class Ops>
PSF_KC_FN void fors_root(const uint64_t (&seed)[NW], uint64_t idx_tree, uint32_t idx_leaf, uint32_t a_bits, uint32_t t, uint32_t index, const uint8_t* sig,
                         uint64_t (&node)[NW]) {
  Adrs a;
  a.init(0, idx_tree, FORS_TREE, idx_leaf);
  const uint32_t leaf = (t << a_bits) + index;
  a.set_tree_height(0);
  a.set_tree_index(leaf);
  load_words<NW>(sig, node);
  hash_f<NW, Ops>(seed, a, node, node);
#pragma clang loop unroll(disable)
  for (uint32_t z = 0; z < a_bits; ++z) {
    uint64_t sib[NW];
    load_words<NW>(sig + (size_t)(z + 1) * 8 * NW, sib);
    path_step<NW, Ops>(seed, a, z, leaf >> z, node, sib);
  }
}
// T_k over the k roots (get: their k NW words): the FORS public key
template <int NW, class Ops, class Get>
PSF_KC_FN void fors_pk(const uint64_t (&seed)[NW], uint64_t idx_tree, uint32_t idx_leaf, uint32_t k, Get&& get, uint64_t (&out)[NW]) {
  Adrs a;
  a.init(0, idx_tree, FORS_ROOTS, idx_leaf);
  hash_t<NW, Ops>(seed, a, (size_t)k * NW, get, out);
}

// layer j of the hypertree: tree address and leaf index from the split of the digest (ht_verify: idx_leaf = idx_tree mod 2^h', idx_tree >>= h')
PSF_KC_FN uint64_t layer_tree(const Params& p, const Split& s, uint32_t j) {
  const uint32_t sh = j * p.hp;
  return sh >= 64 ? 0 : s.idx_tree >> sh;
}
PSF_KC_FN uint32_t layer_leaf(const Params& p, const Split& s, uint32_t j) {
  return j == 0 ? s.idx_leaf : (uint32_t)(layer_tree(p, s, j - 1) & ((1u << p.hp) - 1));
}

}  // namespace slh
}  // namespace psf
