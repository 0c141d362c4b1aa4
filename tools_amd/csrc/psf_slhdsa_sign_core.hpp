// psf_slhdsa_sign_core.hpp -- what slh_sign_internal (FIPS 205 Algorithm 19) adds to psf_slhdsa_core.hpp, over the same Ops back ends: PRF_msg, the FORS
// secret value, leaf and inner node (Algorithms 14 and 15), the rule that says which node of a tree reduction is slot z of an authentication path
// (xmss_sign line 3, fors_sign line 7), and the chain of wots_sign (Algorithm 7, lines 11 to 15).  Everything else a signature needs -- the chain end,
// T_len, the XMSS node, T_k, the digest split, the digits -- is the text KeyGen and Verify already compile.
//
// Which values are secret: SK.seed, SK.prf, every PRF output and every chain value below its signed digit.  The functions here return them in registers;
// the callers store only what the signature reveals (psf_slhdsa_sign.hip).  Every index, digit and loop bound comes from the digest or from a root,
// which a verifier recomputes.
//
// Compiled by the device kernels of psf_slhdsa_sign.hip and by tests/cpp/slhdsa_sign_host_check.cpp (g++, PlainOps).
#pragma once
#include "psf_slhdsa_core.hpp"

namespace psf {
namespace slh {

// ---- PRF_msg ----------------------------------------------------------------------------------------------------------------------------------------------
// R = SHAKE256(SK.prf || opt_rand || M, 8 n) as words: the first NW of r are R.  No alignment is asked; msg may be NULL when msg_len = 0.
template <class Ops> PSF_KC_FN void prf_msg(uint32_t n, const uint8_t* sk_prf, const uint8_t* opt_rand, const uint8_t* msg, size_t msg_len, uint64_t (&r)[4]) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
  kc::absorb<kc::kRateShake256, Ops>(s, Cat3Reader{sk_prf, opt_rand, msg, n, n}, 2 * (size_t)n + msg_len, kc::kDomShake);
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = s[i];
}

// ---- FORS -------------------------------------------------------------------------------------------------------------------------------------------------
// The k trees of one FORS key share one index space: leaf x of tree t is leaf (t << a) + x, and node i of tree t at height z is node (t << (a - z)) + i.
// `leaf` and `i` below are those global indices.
// fors_skGen: the secret value of leaf `leaf` (SECRET unless it is the signed leaf of its tree)
template <int NW, class Ops>
PSF_KC_FN void fors_sk(const uint64_t (&seed)[NW], const uint64_t (&sk_seed)[NW], uint64_t idx_tree, uint32_t idx_leaf, uint32_t leaf, uint64_t (&out)[NW]) {
  Adrs a;
  a.init(0, idx_tree, FORS_PRF, idx_leaf);
  a.set_tree_index(leaf);
  hash_f<NW, Ops>(seed, a, sk_seed, out);
}
// fors_node at height 0: F of the secret value (public)
template <int NW, class Ops>
PSF_KC_FN void fors_leaf(const uint64_t (&seed)[NW], uint64_t idx_tree, uint32_t idx_leaf, uint32_t leaf, const uint64_t (&sk)[NW], uint64_t (&out)[NW]) {
  Adrs a;
  a.init(0, idx_tree, FORS_TREE, idx_leaf);
  a.set_tree_height(0);
  a.set_tree_index(leaf);
  hash_f<NW, Ops>(seed, a, sk, out);
}
// fors_node at height z >= 1 from its children
template <int NW, class Ops>
PSF_KC_FN void fors_parent(const uint64_t (&seed)[NW], uint64_t idx_tree, uint32_t idx_leaf, uint32_t z, uint32_t i, const uint64_t (&l)[NW], const uint64_t (&r)[NW],
                           uint64_t (&out)[NW]) {
  Adrs a;
  a.init(0, idx_tree, FORS_TREE, idx_leaf);
  a.set_tree_height(z);
  a.set_tree_index(i);
  hash_h<NW, Ops>(seed, a, l, r, out);
}

// ---- authentication paths -----------------------------------------------------------------------------------------------------------------------------
// Slot z of the authentication path of leaf `idx` is the node at height z with index (idx >> z) ^ 1 in its own tree (xmss_sign: k = floor(idx / 2^j)
// xor 1; fors_sign: s = floor(indices[i] / 2^j) xor 1).  True when node i at height z is that node.
PSF_KC_FN bool is_auth_node(uint32_t idx, uint32_t z, uint32_t i) { return i == ((idx >> z) ^ 1u); }

// ---- WOTS+ ------------------------------------------------------------------------------------------------------------------------------------------------
// value c of wots_sign: the secret value of chain c walked `digit` steps.  The loop bound is the digit, which the signed message (a root or the FORS
// public key) fixes for every verifier; v is SECRET until the last step and is returned in registers.
template <int NW, class Ops>
PSF_KC_FN void wots_sig_value(const uint64_t (&seed)[NW], const uint64_t (&sk_seed)[NW], uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t c, uint32_t digit,
                              uint64_t (&v)[NW]) {
  Adrs a;
  a.init(layer, tree, WOTS_PRF, leaf);
  a.set_chain(c);
  hash_f<NW, Ops>(seed, a, sk_seed, v);
  a.init(layer, tree, WOTS_HASH, leaf);
  a.set_chain(c);
  chain<NW, Ops>(seed, a, v, 0, digit);
}

}  // namespace slh
}  // namespace psf
