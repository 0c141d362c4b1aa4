// psf_mldsa_api.hpp -- what psf_mldsa.hip (ML-DSA KeyGen / Verify and the FIPS 204 stages) offers psf_mldsa_sign.hip (ML-DSA signing), as
// psf_ntt_api.hpp does for the transforms: the parameter sets, the map between FIPS 204's NTT-domain order and the product images, the launches of
// ExpandA, SampleInBall and the field (un)packing, and the readers that feed tr || M' and mu || w1Encode(...) to the sponge.  The functions are defined
// in psf_mldsa.hip; the templates and small structs live here.  What is not ML-DSA's own (checks, layout, grid limits, host staging) is psf_call.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_keccak_core.hpp"
#include "psf_mldsa_core.hpp"

namespace psf {
namespace dsa {

using kc::aligned8;
using kc::put_words;
using kc::zero_state;

// na bytes of a, then nb bytes of b.  fast: both start at multiples of 8 and so is na.
struct CatReader {
  const uint8_t* a;
  const uint8_t* b;
  size_t na, nb;
  bool fast;
  PSF_KC_FN uint8_t byte(size_t pos) const { return pos < na ? a[pos] : b[pos - na]; }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    uint64_t w = 0;
    if (fast && pos + 8 <= na) { __builtin_memcpy(&w, __builtin_assume_aligned(a + pos, 8), 8); return w; }
    if (fast && pos >= na) { __builtin_memcpy(&w, __builtin_assume_aligned(b + (pos - na), 8), 8); return w; }
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte(pos + k) << (8 * k);
    return w;
  }
};

// ---- the parameter sets ----------------------------------------------------------------------------------------------------------------------------
struct Set { uint32_t k, l, eta, tau, cb, omega; int32_t gamma1, gamma2, beta; int zbits; size_t pk, sk, sig; };
bool set_of(int param, Set* s);

// ---- NTT images ----------------------------------------------------------------------------------------------------------------------------------
// At (8380417, 256) the transform splits completely and the wave kernels compute in canonical 32-bit residues: an image word is f at one of the 256
// odd powers of a 512th root of unity, as a FIPS 204 NTT-domain coefficient is.  What differs is which point sits where: image_map() matches the
// points of the library's plan with those of Algorithm 41 (zeta = 1753).  The change of scale is the reduction of any 64-bit value to [0, q).
struct ImageMap { bool ok = false; uint8_t word_of[256] = {}, fips_of[256] = {}; };
const ImageMap& image_map();

// ---- launches of the stages (arguments checked by the caller; `device` is current) ------------------------------------------------------------------
psf_status rej_ntt_launch(size_t total, uint32_t k, uint32_t l, const uint8_t* d_seed, size_t seed_stride, void* d_out, bool img, int* d_fail, hipStream_t st);
psf_status ball_launch(size_t total, uint32_t tau, const uint8_t* d_ct, size_t len, size_t stride, int64_t* d_out, int* d_fail, hipStream_t st);

// A segment: `polys` polynomials per item, item c's bytes at bytes + c pitch (32 bits bytes per polynomial), its 64-bit words at words + c polys 256.
// A thread moves 8 values = `bits` bytes: 64 bytes of words (four vectors, the workspace is 256-byte aligned) and `bits` single bytes (no alignment
// asked of keys and signatures); neighbouring threads touch neighbouring bytes.
enum { MAP_PLAIN = 0, MAP_T1_SHIFT = 1, MAP_NORM = 2, MAP_T1 = 3, MAP_T0 = 4 };
// unpack: PLAIN the value of the field; T1_SHIFT the value times 2^d; NORM the value, and flags[c] |= NORM when |value| >= bound
// pack: PLAIN the field of the value; T1 / T0 the field of the high / low part of Power2Round(word)
struct Seg { const uint8_t* bytes; int64_t* words; size_t pitch, count; uint32_t polys; int bits; int32_t top; int map; };
psf_status launch_segs(bool pack, const Seg* segs, int nseg, uint32_t* flags, int32_t bound, hipStream_t st);
inline Seg seg_of(const uint8_t* bytes, int64_t* words, size_t pitch, size_t count, uint32_t polys, Packing p, int map) {
  return Seg{bytes, words, pitch, count, polys, kPackTable[p].bits, kPackTable[p].top, map};
}

// ---- the reader of mu || w1Encode(...) ---------------------------------------------------------------------------------------------------------------
// The message mu || w1Encode(w1) of one instance as the sponge reads it: 64 bytes of mu, then fields of BITS bits made on the fly from the words of
// w.  HINT: w1 = UseHint(h, w') with the bits of h (verification); else w1 = HighBits(w) and h is not read (signing).  Its length is a multiple of
// 8, so the sponge asks for whole words only.
template <uint32_t G2, bool HINT = true> struct W1Reader {
  static constexpr int BITS = G2 == kGamma2Low ? 6 : 4;
  const uint8_t* mu;
  bool mu_aligned;
  const uint64_t* w;
  const uint8_t* h;
  size_t fields;
  PSF_KC_FN uint64_t field(size_t f) const {
    if (f >= fields) return 0;
    if constexpr (HINT) return use_hint<G2>((h[f >> 3] >> (f & 7)) & 1u, (uint32_t)w[f]);
    else return high_bits<G2>((uint32_t)w[f]);
  }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    if (pos < 64) return kc::PtrReader{mu, mu_aligned}.le64(pos);
    const size_t bit = (pos - 64) * 8, f0 = bit / BITS;
    const int skew = (int)(bit - f0 * BITS);                              // bits of field f0 that belong to the byte before
    uint64_t acc = field(f0) >> skew;
#pragma clang loop unroll(disable)                                        // kept rolled: the sponge unrolls its 17 words around this, and the state stays in registers
    for (int t = 1; t <= 64 / BITS + 1; ++t) {                            // 6-bit fields at skew 4: the twelfth field starts at bit 62
      const int sh = t * BITS - skew;
      if (sh < 64) acc |= field(f0 + t) << sh;
    }
    return acc;
  }
  PSF_KC_FN uint8_t byte(size_t pos) const { return pos < 64 ? mu[pos] : 0; }      // the length is a multiple of 8: the sponge reads whole words, never this
};

}  // namespace dsa
}  // namespace psf
