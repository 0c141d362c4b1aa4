// psf_mldsa_api.hpp -- what psf_mldsa.hip (ML-DSA KeyGen / Verify and the FIPS 204 stages) offers psf_mldsa_sign.hip (ML-DSA signing), as
// psf_ntt_api.hpp does for the transforms: the parameter sets, the map between FIPS 204's NTT-domain order and the product images, the workspace
// layout helper, the argument checks of a call's buffers, the launches of ExpandA, SampleInBall and the field (un)packing, and the reader that feeds
// mu || w1Encode(...) to the sponge.  The functions are defined in psf_mldsa.hip; the templates and small structs live here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "psf_hip_util.hpp"
#include "psf_keccak_core.hpp"
#include "psf_mldsa_core.hpp"

namespace psf {
namespace dsa {

__device__ __forceinline__ void zero_state(uint64_t (&s)[25]) {
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
}
// words s[first ... first + COUNT - 1] of a state as 8 COUNT bytes at p
template <int FIRST, int COUNT> __device__ __forceinline__ void put_words(const uint64_t (&s)[25], uint8_t* p) {
  const kc::PtrWriter wr{p, (uintptr_t)p % 8 == 0};
#pragma unroll
  for (int i = 0; i < COUNT; ++i) wr.put64(8 * i, s[FIRST + i]);
}
__device__ __forceinline__ bool aligned8(const void* p, size_t pitch) { return ((uintptr_t)p | pitch) % 8 == 0; }

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

// ---- the workspace ---------------------------------------------------------------------------------------------------------------------------------
// The workspace of an operation: sections in a fixed order, each rounded up to 256 bytes.  A polynomial of 64-bit words takes 2048 bytes, an image
// 1024 bytes.
typedef unsigned __int128 u128;
struct Layout {
  size_t total = 0;
  bool ok = true;
  size_t take(u128 bytes) {
    const size_t at = total;
    const u128 end = (u128)total + ((bytes + 255) / 256) * 256;
    if (end > (u128)SIZE_MAX) { ok = false; return 0; }
    total = (size_t)end;
    return at;
  }
};
template <class T> T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(ws) + off); }

// ---- the buffers of a call -------------------------------------------------------------------------------------------------------------------------
// `count` items of `len` bytes, item c at base + c stride (stride 0: one item): the bytes from the first of item 0 to the last of the last item;
// false: the span or its end address does not fit size_t
bool span_of(const void* base, size_t count, size_t len, size_t stride, size_t* span);
bool overlap(const void* a, size_t na, const void* b, size_t nb);
// a buffer of a call: `count` items of `len` bytes at `stride`; ok_null: may be NULL (an empty message, d_why)
struct Buf { const void* p; size_t len, stride; bool out, ok_null; size_t span; };
// the header's order after `param`, `op`, `msg_kind` and count = 0: NULL pointers, [strides: the caller], byte counts, the workspace (device forms), overlaps
psf_status check_null(const Buf* b, int nb);
psf_status check_spans(size_t count, Buf* b, int nb);
psf_status check_ws(bool dev, const void* ws, size_t ws_bytes, size_t need);
psf_status check_overlaps(const Buf* b, int nb, bool dev, const void* ws, size_t need);

#define PSF_TRY(expr)                      \
  do {                                     \
    const psf_status rc__ = (expr);        \
    if (rc__ != PSF_OK) return rc__;       \
  } while (0)

constexpr unsigned kMaxGrid = 0x7fffffffu;
inline unsigned blocks_of(size_t items, size_t per_block) { return (unsigned)((items + per_block - 1) / per_block); }
inline bool grid_fits(size_t count) { return count <= kMaxGrid; }

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
