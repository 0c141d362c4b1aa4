// psf_slhdsa_sha2_sign_core.hpp -- what slh_sign_internal (FIPS 205 Algorithm 19) adds to psf_slhdsa_sha2_core.hpp for the SHA-2 parameter sets, over the
// same Ops back ends: PRF_msg (HMAC, sections 11.2.1 / 11.2.2 and RFC 2104), the FORS secret value, leaf and inner node (Algorithms 14 and 15) and the
// chain of wots_sign (Algorithm 7, lines 11 to 15), all past the PK.seed midstate.  It is to psf_slhdsa_sha2_core.hpp what psf_slhdsa_sign_core.hpp is to
// the SHAKE core; the rule that says which node of a tree reduction is slot z of an authentication path (is_auth_node) is that header's, by inclusion.
// Everything else a signature needs -- the chain end, T_len, the XMSS node, T_k, H_msg, the digest split, the digits -- is the text KeyGen and Verify
// already compile.
//
// Which values are secret: SK.seed, SK.prf, the two key blocks of HMAC and its inner digest, every PRF output and every chain value below its signed
// digit.  The functions here hold them in registers and return them in registers; the callers store only what the signature reveals
// (psf_slhdsa_sha2_sign.hip).  Every index, digit and loop bound comes from the digest, from a root or from the message length.
//
// Compiled by the device kernels of psf_slhdsa_sha2_sign.hip and by tests/cpp/slhdsa_sha2_sign_host_check.cpp (g++, PlainOps).
#pragma once
#include "psf_slhdsa_sha2_core.hpp"
#include "psf_slhdsa_sign_core.hpp"

namespace psf {
namespace slh2 {

using slh::FORS_PRF;
using slh::is_auth_node;

// ---- PRF_msg ----------------------------------------------------------------------------------------------------------------------------------------------
// opt_rand || M: what HMAC's inner hash absorbs after its key block.  msg may be NULL when there are no message bytes: it is then never read.
struct Cat2Reader {
  const uint8_t* a;
  const uint8_t* b;
  size_t na;
  PSF_KC_FN uint8_t byte(size_t pos) const { return pos < na ? a[pos] : b[pos - na]; }
};

// R = Trunc_n(HMAC-H(SK.prf, opt_rand || M)) as words, H = SHA-256 at n = 16 and SHA-512 at n = 24, 32.  The key is n bytes, shorter than a block, so
// K0 = SK.prf || zeros.  Inner hash: the block K0 ^ ipad from registers, then opt_rand || M absorbed with `prior` = one block.  Outer hash: the block
// K0 ^ opad, then ONE more block built in registers with constant indices: the inner digest || 0x80 || zeros || the length (32 + 9 <= 64; 64 + 17 <= 128).
// 3 + ceil((n + |M| + 9) / 64) SHA-256 compressions, or 3 + ceil((n + |M| + 17) / 128) SHA-512 compressions.  The key blocks and the inner digest never
// leave registers.  No alignment is asked of any pointer.
template <int NQ, class Ops>
PSF_KC_FN void prf_msg(const uint8_t* sk_prf, const uint8_t* opt_rand, const uint8_t* msg, size_t msg_len, uint32_t (&r)[NQ]) {
  constexpr size_t n = 4 * NQ;
  uint32_t key[NQ];
  load_be<NQ>(sk_prf, key);
  if constexpr (wide(NQ)) {
    constexpr uint64_t kIpad = 0x3636363636363636ull, kOpad = 0x5c5c5c5c5c5c5c5cull;
    uint64_t w[16], in[8], out[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = (2 * i < NQ ? ((uint64_t)key[2 * i < NQ ? 2 * i : 0] << 32) | key[2 * i < NQ ? 2 * i + 1 : 0] : 0ull) ^ kIpad;
    sha2::init512(in);
    sha2::compress512<Ops>(in, w);
    sha2::absorb512<Ops, sha2::ByteReader<Cat2Reader>, true>(in, {Cat2Reader{opt_rand, msg, n}}, n + msg_len, 128);
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = (2 * i < NQ ? ((uint64_t)key[2 * i < NQ ? 2 * i : 0] << 32) | key[2 * i < NQ ? 2 * i + 1 : 0] : 0ull) ^ kOpad;
    sha2::init512(out);
    sha2::compress512<Ops>(out, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = in[i];
    w[8] = 0x8000000000000000ull;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (128 + 64) * 8;
    sha2::compress512<Ops>(out, w);
#pragma unroll
    for (int i = 0; i < NQ; ++i) r[i] = (uint32_t)(out[i / 2] >> (i % 2 ? 0 : 32));
  } else {
    constexpr uint32_t kIpad = 0x36363636u, kOpad = 0x5c5c5c5cu;
    uint32_t w[16], in[8], out[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = (i < NQ ? key[i < NQ ? i : 0] : 0u) ^ kIpad;
    sha2::init256(in);
    sha2::compress256<Ops>(in, w);
    sha2::absorb256<Ops, sha2::ByteReader<Cat2Reader>, true>(in, {Cat2Reader{opt_rand, msg, n}}, n + msg_len, 64);
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = (i < NQ ? key[i < NQ ? i : 0] : 0u) ^ kOpad;
    sha2::init256(out);
    sha2::compress256<Ops>(out, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = in[i];
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 32) * 8;
    sha2::compress256<Ops>(out, w);
#pragma unroll
    for (int i = 0; i < NQ; ++i) r[i] = out[i];
  }
}

// ---- FORS -------------------------------------------------------------------------------------------------------------------------------------------------
// The k trees of one FORS key share one index space: leaf x of tree t is leaf (t << a) + x, and node i of tree t at height z is node (t << (a - z)) + i.
// `leaf` and `i` below are those global indices.
// fors_skGen: the secret value of leaf `leaf` (SECRET unless it is the signed leaf of its tree)
template <int NQ, class Ops>
PSF_KC_FN void fors_sk(const Mid<NQ>& mid, const uint32_t (&sk_seed)[NQ], uint64_t idx_tree, uint32_t idx_leaf, uint32_t leaf, uint32_t (&out)[NQ]) {
  Adrs a;
  a.init(0, idx_tree, FORS_PRF, idx_leaf);
  a.set_tree_index(leaf);
  hash_f<NQ, Ops>(mid, a, sk_seed, out);
}
// fors_node at height 0: F of the secret value (public)
template <int NQ, class Ops>
PSF_KC_FN void fors_leaf(const Mid<NQ>& mid, uint64_t idx_tree, uint32_t idx_leaf, uint32_t leaf, const uint32_t (&sk)[NQ], uint32_t (&out)[NQ]) {
  Adrs a;
  a.init(0, idx_tree, FORS_TREE, idx_leaf);
  a.set_tree_height(0);
  a.set_tree_index(leaf);
  hash_f<NQ, Ops>(mid, a, sk, out);
}
// fors_node at height z >= 1 from its children
template <int NQ, class Ops>
PSF_KC_FN void fors_parent(const Mid<NQ>& mid, uint64_t idx_tree, uint32_t idx_leaf, uint32_t z, uint32_t i, const uint32_t (&l)[NQ], const uint32_t (&r)[NQ],
                           uint32_t (&out)[NQ]) {
  Adrs a;
  a.init(0, idx_tree, FORS_TREE, idx_leaf);
  a.set_tree_height(z);
  a.set_tree_index(i);
  hash_h<NQ, Ops>(mid, a, l, r, out);
}

// ---- WOTS+ ------------------------------------------------------------------------------------------------------------------------------------------------
// value c of wots_sign: the secret value of chain c walked `digit` steps.  The loop bound is the digit, which the signed message (a root or the FORS
// public key) fixes for every verifier; v is SECRET until the last step and is returned in registers.
template <int NQ, class Ops>
PSF_KC_FN void wots_sig_value(const Mid<NQ>& mid, const uint32_t (&sk_seed)[NQ], uint32_t layer, uint64_t tree, uint32_t leaf, uint32_t c, uint32_t digit,
                              uint32_t (&v)[NQ]) {
  Adrs a;
  a.init(layer, tree, WOTS_PRF, leaf);
  a.set_chain(c);
  hash_f<NQ, Ops>(mid, a, sk_seed, v);
  a.init(layer, tree, WOTS_HASH, leaf);
  a.set_chain(c);
  chain<NQ, Ops>(mid, a, v, 0, digit);
}

}  // namespace slh2
}  // namespace psf
