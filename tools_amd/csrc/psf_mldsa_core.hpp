// psf_mldsa_core.hpp -- what FIPS 204 (ML-DSA, August 2024) adds to the sponge of psf_keccak_core.hpp: the parse loops of its three rejection
// samplers (RejNTTPoly, Algorithm 30; RejBoundedPoly, Algorithm 31; SampleInBall, Algorithm 29), HintBitUnpack (Algorithm 21), Power2Round, Decompose
// and UseHint (Algorithms 35, 36 and 40) for both values of gamma2, the bit fields of its packings (Algorithms 16 to 19), and what signing adds:
// HighBits, LowBits and MakeHint (Algorithms 37 to 39), the norm tests of Algorithm 7, the parse of ExpandMask (Algorithm 34), HintBitPack
// (Algorithm 20) and the rule for the two-byte counter.
//
// Written over the same back ends Ops as the sponge: the device kernels of psf_mldsa.hip and psf_mldsa_sign.hip use DevOps, and g++ compiles this
// same text over PlainOps for tests/cpp/mldsa_host_check.cpp and tests/cpp/mldsa_sign_host_check.cpp, which tests/test_mldsa_core_cpu.py and
// tests/test_mldsa_sign_cpu.py compare with the Python model without a GPU.
//
// The parse loops follow sample_ntt_parse: one Keccak state per lane in registers, every index into the state a compile-time constant (the byte
// positions of a block are unrolled), the lane's own progress in a counter, and one wave-level question per block ("is every lane done?") through
// Ops::all.  A lane that is still short after max_blocks blocks leaves zeros for what is missing and the function returns true.
#pragma once
#include <type_traits>
#include "psf_keccak_core.hpp"

namespace psf {
namespace dsa {

constexpr uint32_t kQ = 8380417, kN = 256, kD = 13;
constexpr uint32_t kGamma2Low = (kQ - 1) / 88, kGamma2High = (kQ - 1) / 32;    // ML-DSA-44; ML-DSA-65 and -87
// The block cap of the three samplers.  A sampler that needs more returns the flag; with acceptance rate p per candidate that is the event "fewer than
// 256 (tau) accepted among the candidates of 8 blocks", bounded by the Chernoff bound exp(-m D(a || p)) with a = 256 / m (DESIGN.md "ML-DSA"):
//   RejNTTPoly      8 x 56 = 448 candidates,  p = q / 2^23 = 0.99902:  below 2^-1479
//   RejBoundedPoly  8 x 272 = 2176 candidates, p = 15 / 16 (eta = 2):  below 2^-6566;  p = 9 / 16 (eta = 4):  below 2^-1365
//   SampleInBall    8 x 136 - 8 = 1080 bytes for tau <= 64 draws, draw i accepted with (i + 1) / 256 >= 3 / 4:  below 2^-1708
constexpr int kMaxBlocks = 8;

// ---- RejNTTPoly -------------------------------------------------------------------------------------------------------------------------------------
// s: the state after absorb<168>(rho || s || r, 34 bytes, 0x1F).  Every 3 bytes give z = b0 + 2^8 b1 + 2^16 (b2 mod 128); each one below q is the
// next coefficient: put(j, z).
template <class Ops, class Put> PSF_KC_FN bool rej_ntt_parse(uint64_t (&s)[25], Put&& put, int max_blocks) {
  uint32_t j = 0;
  for (int blk = 1;; ++blk) {
#pragma unroll
    for (int t = 0; t < kc::kRateShake128 / 3; ++t) {
      const int w = (24 * t) / 64, sh = (24 * t) % 64;
      uint32_t c = (uint32_t)(s[w] >> sh);
      if (sh > 64 - 24) c |= (uint32_t)(s[w + 1] << (64 - sh));
      const uint32_t z = c & 0x7FFFFFu;
      if (z < kQ && j < kN) put(j++, z);
    }
    if (Ops::all(j >= kN) || blk >= max_blocks) break;
    kc::f1600<Ops>(s);
  }
  const bool fail = j < kN;
  for (; j < kN; ++j) put(j, 0u);
  return fail;
}

// ---- RejBoundedPoly ---------------------------------------------------------------------------------------------------------------------------------
// CoeffFromHalfByte: eta = 2: b < 15 gives 2 - (b mod 5); eta = 4: b < 9 gives 4 - b.  b mod 5 = b - 5 floor(13 b / 64) for b < 15.
template <int ETA> PSF_KC_FN bool half_byte_ok(uint32_t b) { return ETA == 2 ? b < 15u : b < 9u; }
template <int ETA> PSF_KC_FN int half_byte_value(uint32_t b) { return ETA == 2 ? 2 - (int)(b - 5u * ((b * 13u) >> 6)) : 4 - (int)b; }

// s: the state after absorb<136>(rho' || le16(nonce), 66 bytes, 0x1F).  The low half of a byte comes first.
template <int ETA, class Ops, class Put> PSF_KC_FN bool rej_bounded_parse(uint64_t (&s)[25], Put&& put, int max_blocks) {
  static_assert(ETA == 2 || ETA == 4, "FIPS 204 uses eta = 2 and eta = 4");
  uint32_t j = 0;
  for (int blk = 1;; ++blk) {
#pragma unroll
    for (int w = 0; w < kc::kRateShake256 / 8; ++w) {
#pragma unroll
      for (int h = 0; h < 16; ++h) {
        const uint32_t b = (uint32_t)(s[w] >> (4 * h)) & 15u;
        if (half_byte_ok<ETA>(b) && j < kN) put(j++, half_byte_value<ETA>(b));
      }
    }
    if (Ops::all(j >= kN) || blk >= max_blocks) break;
    kc::f1600<Ops>(s);
  }
  const bool fail = j < kN;
  for (; j < kN; ++j) put(j, 0);
  return fail;
}

// ---- SampleInBall -----------------------------------------------------------------------------------------------------------------------------------
// s: the state after absorb<136>(c~, lambda / 4 bytes, 0x1F).  The first 8 bytes are the sign bits; every later byte j is a candidate for the current
// i (from 256 - tau to 255): j <= i gives c_i = c_j, c_j = (-1)^h[i + tau - 256].  The polynomial is behind get(j) / put(j, v) (v in {-1, 0, 1}) and
// is all zero on entry: it is indexed by data, so the device keeps it in LDS, not in registers.
template <int FIRST, class Get, class Put>
PSF_KC_FN void ball_bytes(const uint64_t (&s)[25], uint64_t signs, uint32_t tau, uint32_t& i, Get&& get, Put&& put) {
#pragma unroll
  for (int t = FIRST; t < kc::kRateShake256; ++t) {
    const uint32_t j = (uint32_t)(s[t / 8] >> (8 * (t % 8))) & 255u;
    if (i < kN && j <= i) {
      const int v = get(j);
      put(i, v);
      put(j, 1 - 2 * (int)((signs >> (i + tau - kN)) & 1u));
      ++i;
    }
  }
}
template <class Ops, class Get, class Put> PSF_KC_FN bool sample_in_ball_parse(uint64_t (&s)[25], uint32_t tau, Get&& get, Put&& put, int max_blocks) {
  const uint64_t signs = s[0];
  uint32_t i = kN - tau;
  ball_bytes<8>(s, signs, tau, i, get, put);
  for (int blk = 1; !Ops::all(i >= kN) && blk < max_blocks; ++blk) {
    kc::f1600<Ops>(s);
    ball_bytes<0>(s, signs, tau, i, get, put);
  }
  return i < kN;
}

// ---- HintBitUnpack ----------------------------------------------------------------------------------------------------------------------------------
// y(pos): byte pos of the omega + k hint bytes; set(i, j): h[i][j] = 1 (h is all zero on entry).  false stands for the standard's bottom: a count
// byte below the running index or above omega, indices of one polynomial not strictly increasing, a non-zero byte after the last index.
template <class Rd, class Set> PSF_KC_FN bool hint_bit_unpack(Rd&& y, uint32_t k, uint32_t omega, Set&& set) {
  uint32_t index = 0;
  for (uint32_t i = 0; i < k; ++i) {
    const uint32_t end = y(omega + i);
    if (end < index || end > omega) return false;
    const uint32_t first = index;
    uint32_t prev = 0;
    for (; index < end; ++index) {
      const uint32_t cur = y(index);
      if (index > first && prev >= cur) return false;
      set(i, cur);
      prev = cur;
    }
  }
  for (uint32_t p = index; p < omega; ++p)
    if (y(p) != 0) return false;
  return true;
}

// ---- rounding ---------------------------------------------------------------------------------------------------------------------------------------
// r in [0, q) throughout.  Power2Round: r = r1 2^13 + r0 with r0 in (-2^12, 2^12].
PSF_KC_FN void power2round(uint32_t r, uint32_t& r1, int32_t& r0) {
  r1 = (r + (1u << (kD - 1)) - 1) >> kD;
  r0 = (int32_t)r - (int32_t)(r1 << kD);
}
// Decompose: r = r1 (2 gamma2) + r0 with r0 in (-gamma2, gamma2], except that r - r0 = q - 1 gives r1 = 0 and r0 - 1
template <uint32_t G2> PSF_KC_FN void decompose(uint32_t r, uint32_t& r1, int32_t& r0) {
  static_assert(G2 == kGamma2Low || G2 == kGamma2High, "gamma2 = (q - 1) / 88 or (q - 1) / 32");
  constexpr uint32_t m = (kQ - 1) / (2 * G2);
  r1 = (r + G2 - 1) / (2 * G2);                                           // a division by a constant: a multiplication and a shift
  r0 = (int32_t)r - (int32_t)(r1 * 2 * G2);
  if (r1 == m) { r1 = 0; r0 -= 1; }
}
template <uint32_t G2> PSF_KC_FN uint32_t use_hint(uint32_t h, uint32_t r) {
  constexpr uint32_t m = (kQ - 1) / (2 * G2);
  uint32_t r1;
  int32_t r0;
  decompose<G2>(r, r1, r0);
  if (h == 0) return r1;
  if (r0 > 0) return r1 + 1 == m ? 0u : r1 + 1;
  return r1 == 0 ? m - 1 : r1 - 1;
}

// ---- what signing adds (Algorithm 7) -----------------------------------------------------------------------------------------------------------------
// HighBits, LowBits (Algorithms 37 and 38) and MakeHint (Algorithm 39) on residues: MakeHint(z, r) = [HighBits(r) != HighBits(r + z)], called with
// r and r + z mod q both at hand (signing has r = w - c s2 and r + z = r + c t0).  Selects and arithmetic only: nothing here branches on its data.
template <uint32_t G2> PSF_KC_FN uint32_t high_bits(uint32_t r) {
  uint32_t r1;
  int32_t r0;
  decompose<G2>(r, r1, r0);
  return r1;
}
template <uint32_t G2> PSF_KC_FN int32_t low_bits(uint32_t r) {
  uint32_t r1;
  int32_t r0;
  decompose<G2>(r, r1, r0);
  return r0;
}
template <uint32_t G2> PSF_KC_FN uint32_t make_hint(uint32_t r, uint32_t r_plus_z) { return high_bits<G2>(r) != high_bits<G2>(r_plus_z) ? 1u : 0u; }
// r in [0, q) as its representative in (-q / 2, q / 2], and the absolute value of that
PSF_KC_FN int32_t centered(uint32_t r) { return (int32_t)r - (int32_t)(kQ & (0u - (uint32_t)(r > (kQ - 1) / 2))); }
PSF_KC_FN uint32_t centered_abs(uint32_t r) {
  const int32_t c = centered(r), m = c >> 31;
  return (uint32_t)((c ^ m) - m);
}
// 1 when the residue's centred absolute value reaches the bound: the tests ||z|| >= gamma1 - beta and ||c t0|| >= gamma2 of Algorithm 7
PSF_KC_FN uint32_t norm_reaches(uint32_t r, uint32_t bound) { return centered_abs(r) >= bound ? 1u : 0u; }
// the same for a LowBits value: ||r0|| >= gamma2 - beta
PSF_KC_FN uint32_t low_reaches(int32_t r0, uint32_t bound) {
  const int32_t m = r0 >> 31;
  return (uint32_t)((r0 ^ m) - m) >= bound ? 1u : 0u;
}
// The counter of ExpandMask is two bytes: an attempt at kappa draws the nonces kappa ... kappa + l - 1, so it may start only while
// kappa + l <= 2^16.  true: the instance has used up its counter and is retired unsigned.
PSF_KC_FN bool kappa_exhausted(uint32_t kappa, uint32_t l) { return kappa + l > 65536u; }

// ExpandMask (Algorithm 34), one polynomial: s is the state after absorb<136>(rho'' || le16(kappa + r), 66 bytes, 0x1F); the first 32 BITS bytes of
// the stream (576 for gamma1 = 2^17, 640 for 2^19: five blocks) are 256 fields of BITS bits and coefficient j = gamma1 - field: put(j, value).
// Every position is a constant once the loops are unrolled: a field that straddles two words takes its low part from the word kept from before.
template <int BITS, class Ops, class Put> PSF_KC_FN void expand_mask_parse(uint64_t (&s)[25], Put&& put) {
  static_assert(BITS == 18 || BITS == 20, "gamma1 = 2^17 or 2^19");
  constexpr int kWords = kc::kRateShake256 / 8, kTotal = 4 * BITS, kBlocks = (kTotal + kWords - 1) / kWords;       // 64-bit words of the stream
  constexpr int32_t g1 = 1 << (BITS - 1);
  uint64_t prev = 0;
#pragma unroll
  for (int blk = 0; blk < kBlocks; ++blk) {
    if (blk) kc::f1600<Ops>(s);
#pragma unroll
    for (int i = 0; i < kWords; ++i) {
      const int g = blk * kWords + i;
      if (g < kTotal) {
        const uint64_t cur = s[i];
        // the fields that end inside word g: their last bit is in [64 g, 64 g + 63]
        const int first = (64 * g) / BITS - 1, last = (64 * g + 64) / BITS - 1;
#pragma unroll
        for (int t = first; t <= last; ++t) {
          const int start = t * BITS;
          if (start + BITS > 64 * g && start + BITS <= 64 * g + 64 && t >= 0) {
            uint64_t v;
            if (start >= 64 * g) v = cur >> (start - 64 * g);
            else v = (prev >> (start - 64 * (g - 1))) | (cur << (64 * g - start));
            put((uint32_t)t, g1 - (int32_t)((uint32_t)v & ((1u << BITS) - 1)));
          }
        }
        prev = cur;
      }
    }
  }
}

// HintBitPack (Algorithm 20): mask(i, b) is the byte of the bits h[i][8 b ... 8 b + 7] (bit 0 first); put(pos, v) gets every one of the omega + k
// bytes, zeros included.  The caller has checked that at most omega bits are set.
template <class Mask, class Put> PSF_KC_FN void hint_bit_pack(Mask&& mask, uint32_t k, uint32_t omega, Put&& put) {
  uint32_t index = 0;
  for (uint32_t i = 0; i < k; ++i) {
    for (uint32_t b = 0; b < kN / 8; ++b) {
      uint32_t m = mask(i, b) & 255u;
      for (; m != 0 && index < omega; m &= m - 1) put(index++, 8 * b + (uint32_t)__builtin_ctz(m));
    }
    put(omega + i, index);
  }
  for (; index < omega; ++index) put(index, 0u);
}

// ---- packings ---------------------------------------------------------------------------------------------------------------------------------------
// Every packing of FIPS 204 is a row of this table: fields of `bits` bits, least significant first, field = value (SimpleBitPack: top < 0) or
// field = top - value (BitPack(w, a, b) with b = top).  256 fields are 32 bits bytes; 8 fields are `bits` whole bytes, the unit a thread moves.
enum Packing : int { kPackT1 = 0, kPackT0, kPackEta2, kPackEta4, kPackZ17, kPackZ19, kPackW1Low, kPackW1High, kPackings };
struct PackSpec { int bits; int32_t top; };
constexpr PackSpec kPackTable[kPackings] = {
    {10, -1},                  // t1: SimpleBitPack(t1, 2^10 - 1)
    {13, 1 << 12},             // t0: BitPack(t0, 2^12 - 1, 2^12)
    {3, 2},                    // s1, s2 at eta = 2: BitPack(s, 2, 2)
    {4, 4},                    // s1, s2 at eta = 4: BitPack(s, 4, 4)
    {18, 1 << 17},             // z at gamma1 = 2^17: BitPack(z, 2^17 - 1, 2^17)
    {20, 1 << 19},             // z at gamma1 = 2^19
    {6, -1},                   // w1 at gamma2 = (q - 1) / 88: SimpleBitPack(w1, 43)
    {4, -1},                   // w1 at gamma2 = (q - 1) / 32: SimpleBitPack(w1, 15)
};
PSF_KC_FN int32_t field_to_value(int32_t top, uint32_t f) { return top < 0 ? (int32_t)f : top - (int32_t)f; }
PSF_KC_FN uint32_t value_to_field(int32_t top, int32_t v) { return (uint32_t)(top < 0 ? v : top - v); }

// 8 fields <-> BITS bytes at any address
template <int BITS> PSF_KC_FN void unpack8(const uint8_t* src, uint32_t (&f)[8]) {
  static_assert(BITS >= 1 && BITS <= 24, "at most three 64-bit words");
  uint64_t w[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < BITS; ++k) w[k / 8] |= (uint64_t)src[k] << (8 * (k % 8));
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int bit = j * BITS, wd = bit / 64, sh = bit % 64;
    uint64_t v = w[wd] >> sh;
    if (sh + BITS > 64) v |= w[wd + 1] << (64 - sh);
    f[j] = (uint32_t)v & ((1u << BITS) - 1);
  }
}
template <int BITS> PSF_KC_FN void pack8(uint8_t* dst, const uint32_t (&f)[8]) {
  static_assert(BITS >= 1 && BITS <= 24, "at most three 64-bit words");
  uint64_t w[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int bit = j * BITS, wd = bit / 64, sh = bit % 64;
    const uint64_t v = f[j] & ((1u << BITS) - 1);
    w[wd] |= v << sh;
    if (sh + BITS > 64) w[wd + 1] |= v >> (64 - sh);
  }
#pragma unroll
  for (int k = 0; k < BITS; ++k) dst[k] = (uint8_t)(w[k / 8] >> (8 * (k % 8)));
}
// f(ic) for the integral constant of `bits` among the widths of the table; false when it is none of them
template <class F> PSF_KC_FN bool for_bits(int bits, F&& f) {
  switch (bits) {
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 10: f(std::integral_constant<int, 10>{}); return true;
    case 13: f(std::integral_constant<int, 13>{}); return true;
    case 18: f(std::integral_constant<int, 18>{}); return true;
    case 20: f(std::integral_constant<int, 20>{}); return true;
  }
  return false;
}

}  // namespace dsa
}  // namespace psf
