// psf_slhdsa_sha2_core.hpp -- FIPS 205 section 11.2: SLH-DSA's hash functions for the SHA-2 parameter sets, over psf_sha2_core.hpp, and the WOTS+ / XMSS /
// FORS steps on top of them.  The hash-free parts (Params, sig_bytes, digest_split, base_2b, wots_csum / wots_digit, layer_tree / layer_leaf, the ADRS
// type numbers) are those of psf_slhdsa_core.hpp, by inclusion: the SHA-2 sets have the SHAKE sets' (n, h, d, h', a, k, m).
//
//   n = 16       F, PRF, H, T_l = Trunc_n(SHA-256(PK.seed || toByte(0, 64 - n) || ADRSc || M));  H_msg = MGF1-SHA-256(R || PK.seed || SHA-256(R || PK.seed ||
//                PK.root || M), m)
//   n = 24, 32   F, PRF as above;  H, T_l = Trunc_n(SHA-512(PK.seed || toByte(0, 128 - n) || ADRSc || M));  H_msg = MGF1-SHA-512 over SHA-512
// with the compressed address ADRSc = layer 1 byte || tree 8 || type 1 || keypair 4 || chain or tree height 4 || hash or tree index 4: 22 bytes.
//
// The midstate.  The first block of F, PRF, H and T_l is PK.seed || zeros: it depends on the key alone.  Mid<NQ> holds the state after it (SHA-256, and
// SHA-512 when n > 16); a kernel makes it once per lane at entry, and every function here takes the midstate, never the seed.  Past the midstate F, PRF
// and H are ONE compression (22 + n + 9 <= 64; 22 + 32 + 9 = 63; 22 + 2 n + 17 <= 128), built in registers.
//
// Words.  An n-byte string is NQ = n / 4 big-endian 32-bit words (4, 6, 8), the form of a SHA-2 digest: F's output re-enters F, and H's SHA-512 output
// enters F or H, with no byte swap.  ADRSc is 22 bytes, so the operands sit at a half-word offset in the block: message word j is
// (previous << 16) | (current >> 16), one v_alignbit_b32 each.  Adrs holds ADRSc as the six words w[0 ... 5] of the block, the low half of w[5] left
// zero for the top of M; the chain loop changes only the hash address: the low half of w[4] and the high half of w[5].
//
// Written over the Ops back ends: the device kernels of psf_slhdsa_sha2.hip and tests/cpp/slhdsa_sha2_host_check.cpp (g++, PlainOps) compile this text.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "psf_sha2_core.hpp"
#include "psf_slhdsa_core.hpp"

namespace psf {
namespace slh2 {

using slh::Params;
using slh::Split;
using slh::kParams;
using slh::kSets;
using slh::kW;
using slh::sig_bytes;
using slh::wots_len;
using slh::digest_split;
using slh::base_2b;
using slh::wots_digit;
using slh::layer_tree;
using slh::layer_leaf;
using slh::Cat3Reader;
using slh::WOTS_HASH;
using slh::WOTS_PK;
using slh::TREE;
using slh::FORS_TREE;
using slh::FORS_ROOTS;
using slh::WOTS_PRF;

// ---- ADRSc as block words ---------------------------------------------------------------------------------------------------------------------------------
struct Adrs {
  uint32_t w[6];
  PSF_KC_FN void init(uint32_t layer, uint64_t tree, uint32_t type, uint32_t keypair) {
    w[0] = (layer << 24) | (uint32_t)(tree >> 40);
    w[1] = (uint32_t)(tree >> 8);
    w[2] = ((uint32_t)tree << 24) | (type << 16) | (keypair >> 16);
    w[3] = keypair << 16;
    w[4] = 0;
    w[5] = 0;
  }
  PSF_KC_FN void set_chain(uint32_t c) {                                  // also the tree height
    w[3] = (w[3] & 0xFFFF0000u) | (c >> 16);
    w[4] = (w[4] & 0x0000FFFFu) | (c << 16);
  }
  PSF_KC_FN void set_hash(uint32_t x) {                                   // also the tree index
    w[4] = (w[4] & 0xFFFF0000u) | (x >> 16);
    w[5] = x << 16;
  }
  PSF_KC_FN void set_tree_height(uint32_t z) { set_chain(z); }
  PSF_KC_FN void set_tree_index(uint32_t i) { set_hash(i); }
};

// ---- strings as words -------------------------------------------------------------------------------------------------------------------------------------
template <int NQ> PSF_KC_FN void load_be(const uint8_t* p, uint32_t (&w)[NQ]) {                    // no alignment asked of p
#pragma unroll
  for (int i = 0; i < NQ; ++i) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
}
template <int NQ> PSF_KC_FN void store_be(uint8_t* p, const uint32_t (&w)[NQ]) {
#pragma unroll
  for (int i = 0; i < NQ; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) p[4 * i + k] = (uint8_t)(w[i] >> (24 - 8 * k));
}
// byte i of the string whose words are at w (a node in the workspace)
PSF_KC_FN uint32_t byte_of(const uint32_t* w, uint32_t i) { return (w[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu; }

// ---- the midstate -----------------------------------------------------------------------------------------------------------------------------------------
constexpr bool wide(int NQ) { return NQ > 4; }                            // H and T_l on SHA-512
template <int NQ> struct Mid {
  uint32_t a[8];                                                          // SHA-256 after PK.seed || toByte(0, 64 - n)
  uint64_t b[wide(NQ) ? 8 : 1];                                           // SHA-512 after PK.seed || toByte(0, 128 - n), when n > 16
};
template <int NQ, class Ops> PSF_KC_FN void mid256(const uint32_t (&seed)[NQ], Mid<NQ>& m) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = i < NQ ? seed[i < NQ ? i : 0] : 0u;
  sha2::init256(m.a);
  sha2::compress256<Ops>(m.a, w);
}
template <int NQ, class Ops> PSF_KC_FN void mid512(const uint32_t (&seed)[NQ], Mid<NQ>& m) {
  if constexpr (wide(NQ)) {
    uint64_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 2 * i < NQ ? ((uint64_t)seed[2 * i < NQ ? 2 * i : 0] << 32) | seed[2 * i < NQ ? 2 * i + 1 : 0] : 0ull;
    sha2::init512(m.b);
    sha2::compress512<Ops>(m.b, w);
  }
}
// what a stage needs: F / PRF take the SHA-256 state, H / T_l the SHA-256 state at n = 16 and the SHA-512 state above
template <int NQ, class Ops> PSF_KC_FN void mid_f(const uint8_t* pk_seed, Mid<NQ>& m) {
  uint32_t seed[NQ];
  load_be<NQ>(pk_seed, seed);
  mid256<NQ, Ops>(seed, m);
}
template <int NQ, class Ops> PSF_KC_FN void mid_h(const uint8_t* pk_seed, Mid<NQ>& m) {
  uint32_t seed[NQ];
  load_be<NQ>(pk_seed, seed);
  if constexpr (wide(NQ)) mid512<NQ, Ops>(seed, m);
  else mid256<NQ, Ops>(seed, m);
}
template <int NQ, class Ops> PSF_KC_FN void mid_fh(const uint8_t* pk_seed, Mid<NQ>& m) {
  uint32_t seed[NQ];
  load_be<NQ>(pk_seed, seed);
  mid256<NQ, Ops>(seed, m);
  mid512<NQ, Ops>(seed, m);
}

// ---- F, PRF and H: one compression ------------------------------------------------------------------------------------------------------------------------
// out = Trunc_n(SHA-256(PK.seed || 0 ... || ADRSc || m)): F; with m = SK.seed, PRF.  `out` may be `m`.
template <int NQ, class Ops> PSF_KC_FN void hash_f(const Mid<NQ>& mid, const Adrs& a, const uint32_t (&m)[NQ], uint32_t (&out)[NQ]) {
  uint32_t w[16], h[8];
#pragma unroll
  for (int i = 0; i < 5; ++i) w[i] = a.w[i];
  w[5] = a.w[5] | (m[0] >> 16);
#pragma unroll
  for (int i = 1; i < NQ; ++i) w[5 + i] = (m[i - 1] << 16) | (m[i] >> 16);
  w[5 + NQ] = (m[NQ - 1] << 16) | 0x8000u;
#pragma unroll
  for (int i = 6 + NQ; i < 15; ++i) w[i] = 0;
  w[15] = (64 + 22 + 4 * NQ) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = mid.a[i];
  sha2::compress256<Ops>(h, w);
#pragma unroll
  for (int i = 0; i < NQ; ++i) out[i] = h[i];
}
// out = H(PK.seed, ADRS, l || r).  `out` may be `l` or `r`.
template <int NQ, class Ops> PSF_KC_FN void hash_h(const Mid<NQ>& mid, const Adrs& a, const uint32_t (&l)[NQ], const uint32_t (&r)[NQ], uint32_t (&out)[NQ]) {
  constexpr int kWords = wide(NQ) ? 32 : 16;                              // the block as 32-bit words
  static_assert(6 + 2 * NQ <= kWords - (wide(NQ) ? 4 : 2), "ADRSc, two nodes and the 0x80 leave room for the length");
  uint32_t s[kWords];
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i] = a.w[i];
  s[5] = a.w[5] | (l[0] >> 16);
#pragma unroll
  for (int i = 1; i < NQ; ++i) s[5 + i] = (l[i - 1] << 16) | (l[i] >> 16);
  s[5 + NQ] = (l[NQ - 1] << 16) | (r[0] >> 16);
#pragma unroll
  for (int i = 1; i < NQ; ++i) s[5 + NQ + i] = (r[i - 1] << 16) | (r[i] >> 16);
  s[5 + 2 * NQ] = (r[NQ - 1] << 16) | 0x8000u;
#pragma unroll
  for (int i = 6 + 2 * NQ; i < kWords - 1; ++i) s[i] = 0;
  s[kWords - 1] = (kWords * 4 + 22 + 8 * NQ) * 8;
  if constexpr (wide(NQ)) {
    uint64_t w[16], h[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = ((uint64_t)s[2 * i] << 32) | s[2 * i + 1];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = mid.b[i];
    sha2::compress512<Ops>(h, w);
#pragma unroll
    for (int i = 0; i < NQ; ++i) out[i] = (uint32_t)(h[i / 2] >> (i % 2 ? 0 : 32));
  } else {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = mid.a[i];
    sha2::compress256<Ops>(h, s);
#pragma unroll
    for (int i = 0; i < NQ; ++i) out[i] = h[i];
  }
}

// ---- T_l --------------------------------------------------------------------------------------------------------------------------------------------------
// out = T_l(PK.seed, ADRS, the `nwords` 32-bit words get(0), get(1), ...).  get is asked for words below nwords only, each once, in ascending order, and
// the control flow depends on nwords alone.  The message past the midstate is the stream of 32-bit words S: S[0 ... 4] = ADRSc's first 20 bytes,
// S[5 + i] = (X[i - 1] << 16) | (X[i] >> 16) with X[-1] the last two bytes of ADRSc, X[nwords] = 0x80000000 and zeros after it; the block that holds the
// 0x80 early enough (S index <= 16 b + 13, or 32 b + 27 in a SHA-512 block) ends with the length and is the last.  Blocks past the midstate: T_len 10 / 10 /
// 18 (n = 16 / 24 / 32), T_k 4 / 9 / 4 / 7 / 6 / 10 (128s / 128f / 192s / 192f / 256s / 256f; 128s fills its last block to the byte: 246 + 9 = 255 of 256).
template <int NQ, class Ops, class Get> PSF_KC_FN void hash_t(const Mid<NQ>& mid, const Adrs& a, size_t nwords, Get&& get, uint32_t (&out)[NQ]) {
  constexpr int kWords = wide(NQ) ? 32 : 16, kLen = wide(NQ) ? 4 : 2;
  const size_t pad_at = 5 + nwords;                                       // the S index of the word that holds the 0x80
  const uint32_t bits = (uint32_t)((kWords * 4 + 22 + 4 * nwords) * 8);
  uint32_t prev = a.w[5];                                                 // X[i - 1] << 16
  auto next = [&](size_t j) -> uint32_t {                                 // S[j], for j = 0, 1, 2, ... in turn
    if (j < 5) return a.w[j];
    const size_t i = j - 5;
    const uint32_t x = i < nwords ? get(i) : (i == nwords ? 0x80000000u : 0u);
    const uint32_t s = prev | (x >> 16);
    prev = x << 16;
    return s;
  };
  uint32_t h32[8];
  uint64_t h64[8];
  if constexpr (wide(NQ)) {
#pragma unroll
    for (int i = 0; i < 8; ++i) h64[i] = mid.b[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) h32[i] = mid.a[i];
  }
  for (size_t b = 0;; ++b) {
    const bool last = pad_at <= b * kWords + (kWords - kLen - 1);
    uint32_t s[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) s[i] = next(b * kWords + i);
    if (last) s[kWords - 1] = bits;
    if constexpr (wide(NQ)) {
      uint64_t w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) w[i] = ((uint64_t)s[2 * i] << 32) | s[2 * i + 1];
      sha2::compress512<Ops>(h64, w);
    } else {
      sha2::compress256<Ops>(h32, s);
    }
    if (last) break;
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    if constexpr (wide(NQ)) out[i] = (uint32_t)(h64[i / 2] >> (i % 2 ? 0 : 32));
    else out[i] = h32[i];
  }
}

// ---- H_msg ------------------------------------------------------------------------------------------------------------------------------------------------
// The first 64 bytes of the mask of H_msg(R, PK.seed, PK.root, M) as bytes at out64 (m <= 49 of them are the digest): both counters of MGF1-SHA-256 (m = 34
// of SHA2-128f needs the second), or the one of MGF1-SHA-512.
// n = 16: the MGF1 seed R || PK.seed || digest is exactly one block, so the two counters share its compression; the counter, the 0x80 and the length are
// the second block: ceil((48 + |M| + 9) / 64) + 3 compressions.
template <class Ops> PSF_KC_FN void h_msg_256(const uint8_t* r, const uint8_t* pk, const uint8_t* msg, size_t msg_len, uint8_t* out64) {
  uint32_t d[8];
  sha2::init256(d);
  sha2::absorb256<Ops, sha2::ByteReader<Cat3Reader>, true>(d, {Cat3Reader{r, pk, msg, 16, 32}}, 48 + msg_len, 0);
  uint32_t w[16], seed[8];
  {
    uint32_t t[4];
    load_be<4>(r, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = t[i];
    load_be<4>(pk, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[4 + i] = t[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) w[8 + i] = d[i];
  sha2::init256(seed);
  sha2::compress256<Ops>(seed, w);
#pragma clang loop unroll(disable)
  for (uint32_t c = 0; c < 2; ++c) {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = seed[i];
    w[0] = c;
    w[1] = 0x80000000u;
#pragma unroll
    for (int i = 2; i < 15; ++i) w[i] = 0;
    w[15] = 68 * 8;
    sha2::compress256<Ops>(h, w);
    sha2::put_digest256(h, out64 + 32 * c, 32);
  }
}
// R || PK.seed || the 64 bytes at `dig` || toByte(0, 4): the input of counter 0 of MGF1-SHA-512
struct MgfReader {
  const uint8_t* r;
  const uint8_t* pk;
  const uint8_t* dig;
  size_t n;
  PSF_KC_FN uint8_t byte(size_t pos) const { return pos < n ? r[pos] : (pos < 2 * n ? pk[pos - n] : (pos < 2 * n + 64 ? dig[pos - 2 * n] : (uint8_t)0)); }
};
// n = 24, 32: the inner digest (64 bytes) goes through out64 itself -- it is indexed by a run-time position when MGF1 reads it back, and a register
// array must not be -- and the mask then replaces it.  The lane reads only what it wrote itself.
template <class Ops> PSF_KC_FN void h_msg_512(uint32_t n, const uint8_t* r, const uint8_t* pk, const uint8_t* msg, size_t msg_len, uint8_t* out64) {
  uint64_t d[8];
  sha2::init512(d);
  sha2::absorb512<Ops, sha2::ByteReader<Cat3Reader>, true>(d, {Cat3Reader{r, pk, msg, n, 2 * (size_t)n}}, 3 * (size_t)n + msg_len, 0);
  sha2::put_digest512(d, out64, 64);
  sha2::init512(d);
  sha2::absorb512<Ops, sha2::ByteReader<MgfReader>, true>(d, {MgfReader{r, pk, out64, n}}, 2 * (size_t)n + 68, 0);
  sha2::put_digest512(d, out64, 64);
}

// ---- WOTS+ ------------------------------------------------------------------------------------------------------------------------------------------------
// chain(X, start, steps): v = F(PK.seed, ADRS with hash address j, v) for j = start ... start + steps - 1.  a: type WOTS_HASH with keypair and chain set.
template <int NQ, class Ops> PSF_KC_FN void chain(const Mid<NQ>& mid, Adrs a, uint32_t (&v)[NQ], uint32_t start, uint32_t steps) {
#pragma clang loop unroll(disable)
  for (uint32_t j = start; j < start + steps; ++j) {
    a.set_hash(j);
    hash_f<NQ, Ops>(mid, a, v, v);
  }
}
// the public value of chain `c` of the WOTS+ key of leaf `leaf` (wots_pkGen, lines 4 to 9): PRF, then the whole chain of 15 steps, whatever the secret
template <int NQ, class Ops>
PSF_KC_FN void wots_chain_end(const Mid<NQ>& mid, const uint32_t (&sk_seed)[NQ], uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t c, uint32_t (&v)[NQ]) {
  Adrs a;
  a.init(layer, tree, WOTS_PRF, leaf);
  a.set_chain(c);
  hash_f<NQ, Ops>(mid, a, sk_seed, v);
  a.init(layer, tree, WOTS_HASH, leaf);
  a.set_chain(c);
  chain<NQ, Ops>(mid, a, v, 0, kW - 1);
}
// chain i of wots_pkFromSig: the signature value walked from its digit to the end
template <int NQ, class Ops>
PSF_KC_FN void wots_chain_from_sig(const Mid<NQ>& mid, uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t c, uint32_t digit, uint32_t (&v)[NQ]) {
  Adrs a;
  a.init(layer, tree, WOTS_HASH, leaf);
  a.set_chain(c);
  chain<NQ, Ops>(mid, a, v, digit, kW - 1 - digit);
}
// T_len over the len chain ends (get: their len NQ words): the WOTS+ public key, leaf `leaf` of its XMSS tree
template <int NQ, class Ops, class Get>
PSF_KC_FN void wots_pk(const Mid<NQ>& mid, uint32_t layer, uint64_t tree, uint32_t leaf, Get&& get, uint32_t (&out)[NQ]) {
  Adrs a;
  a.init(layer, tree, WOTS_PK, leaf);
  hash_t<NQ, Ops>(mid, a, (size_t)wots_len(4 * NQ) * NQ, get, out);
}

// ---- tree nodes -------------------------------------------------------------------------------------------------------------------------------------------
// node (height z, index i) of an XMSS tree from its children: xmss_node, lines 5 to 10
template <int NQ, class Ops>
PSF_KC_FN void xmss_parent(const Mid<NQ>& mid, uint32_t layer, uint64_t tree, uint32_t z, uint32_t i, const uint32_t (&l)[NQ], const uint32_t (&r)[NQ],
                           uint32_t (&out)[NQ]) {
  Adrs a;
  a.init(layer, tree, TREE, 0);
  a.set_tree_height(z);
  a.set_tree_index(i);
  hash_h<NQ, Ops>(mid, a, l, r, out);
}
// one step up an authentication path: `node` at height z with index `idx` at that height becomes its parent; the sibling is `auth`.  a: type TREE, or
// FORS_TREE with its keypair.  Both orders are formed by selection, not by a branch.
template <int NQ, class Ops> PSF_KC_FN void path_step(const Mid<NQ>& mid, Adrs a, uint32_t z, uint32_t idx, uint32_t (&node)[NQ], const uint32_t (&auth)[NQ]) {
  const bool right = idx & 1u;
  uint32_t l[NQ], r[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    l[i] = right ? auth[i] : node[i];
    r[i] = right ? node[i] : auth[i];
  }
  a.set_tree_height(z + 1);
  a.set_tree_index(idx >> 1);
  hash_h<NQ, Ops>(mid, a, l, r, node);
}
// the root of an XMSS tree from leaf `leaf` and its h' siblings at `auth` (n bytes each)
template <int NQ, class Ops>
PSF_KC_FN void xmss_root(const Mid<NQ>& mid, uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t hp, const uint8_t* auth, uint32_t (&node)[NQ]) {
  Adrs a;
  a.init(layer, tree, TREE, 0);
#pragma clang loop unroll(disable)
  for (uint32_t z = 0; z < hp; ++z) {
    uint32_t sib[NQ];
    load_be<NQ>(auth + (size_t)z * 4 * NQ, sib);
    path_step<NQ, Ops>(mid, a, z, leaf >> z, node, sib);
  }
}
// the root of FORS tree t from its part of SIG_FORS (the secret value, then a siblings): fors_pkFromSig, lines 3 to 20
template <int NQ, class Ops>
PSF_KC_FN void fors_root(const Mid<NQ>& mid, uint64_t idx_tree, uint32_t idx_leaf, uint32_t a_bits, uint32_t t, uint32_t index, const uint8_t* sig,
                         uint32_t (&node)[NQ]) {
  Adrs a;
  a.init(0, idx_tree, FORS_TREE, idx_leaf);
  const uint32_t leaf = (t << a_bits) + index;
  a.set_tree_height(0);
  a.set_tree_index(leaf);
  load_be<NQ>(sig, node);
  hash_f<NQ, Ops>(mid, a, node, node);
#pragma clang loop unroll(disable)
  for (uint32_t z = 0; z < a_bits; ++z) {
    uint32_t sib[NQ];
    load_be<NQ>(sig + (size_t)(z + 1) * 4 * NQ, sib);
    path_step<NQ, Ops>(mid, a, z, leaf >> z, node, sib);
  }
}
// T_k over the k roots (get: their k NQ words): the FORS public key
template <int NQ, class Ops, class Get>
PSF_KC_FN void fors_pk(const Mid<NQ>& mid, uint64_t idx_tree, uint32_t idx_leaf, uint32_t k, Get&& get, uint32_t (&out)[NQ]) {
  Adrs a;
  a.init(0, idx_tree, FORS_ROOTS, idx_leaf);
  hash_t<NQ, Ops>(mid, a, (size_t)k * NQ, get, out);
}

}  // namespace slh2
}  // namespace psf
