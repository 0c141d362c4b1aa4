// psf_ntt_fips.hpp -- between FIPS 203's NTT-domain representation (q = 3329, n = 256: the order Algorithm 9 leaves a polynomial in) and the
// register image of the wave kernels (psf_ntt_kernels.hpp: hat[r * 64 + lane] = register r of lane `lane` after Core::forward).
//
// Both are the residues of f modulo the same 128 leaf moduli X^2 - gamma, so a leaf's two coefficients are the same numbers in both; what differs
// is which leaf sits where, and the scale.  Leaf g of the image (positions 2g and 2g + 1 of the lane-major order, position p in register
// reg_of_nat(p mod 4) of lane floor(p / 4)) has gamma = (-1)^g zetas[64 + floor(g / 2)] of the plan; leaf i of FIPS 203 (coefficients 2i, 2i + 1) has
// gamma = 17^(2 BitRev7(i) + 1).  The image carries R^-nrf in the signed 16-bit Montgomery form (R = 2^16, nrf of Bounds16<12, 8, 1>).
// make_fips203_image_map (psf_host.cpp) matches the gammas and composes the three; the two word maps below are one Montgomery product each.
// Plain C++: tests/ntt_model/ntt_fips_model.cpp runs the map and these functions on the CPU against Algorithm 9 written out with zeta = 17.
#pragma once
#include <stdint.h>
#include "psf_ntt_core.hpp"

namespace psf {
namespace ntt {

struct FipsImageMap {
  bool ok = false;
  uint8_t word_of[256] = {};     // FIPS 203 coefficient k -> word of the image
  uint8_t fips_of[256] = {};     // word of the image -> FIPS 203 coefficient
  int32_t q = 0, qinv16 = 0;     // q and q^-1 mod 2^16 (signed), as in NttTables
  int32_t c_from = 0, c_to = 0;  // R^(1 - nrf) and R^(1 + nrf) mod q, centred: mont(c_from v) = v R^-nrf, mont(c_to x) = x R^nrf
};

// (t - m q) / 2^16 with m = the signed low half of t q^-1: t R^-1 mod q, |result| <= |t| / 2^16 + q / 2, for |t| + 2^15 q < 2^31
PSF_NTT_FN int32_t fips_mont16(int32_t t, int32_t q, int32_t qinv16) {
  const int32_t m = (int16_t)(uint16_t)((uint32_t)t * (uint32_t)qinv16);
  return (t - m * q) >> 16;
}
// v in [0, q) -> the word of an image: |word| < q, inside what Bounds16 assumes of a forward output (xf >= 2^QB > q)
PSF_NTT_FN uint32_t fips_word_from(uint32_t v, int32_t q, int32_t qinv16, int32_t c_from) {
  return (uint32_t)fips_mont16(c_from * (int32_t)v, q, qinv16);
}
// the word of an image (|x| < 2^23 as every operand of a 24-bit multiply; |c_to x| / 2^16 + q / 2 < q for |x| <= xf) -> its residue in [0, q)
PSF_NTT_FN uint32_t fips_word_to(uint32_t x, int32_t q, int32_t qinv16, int32_t c_to) {
  const int32_t r = fips_mont16(c_to * (int32_t)x, q, qinv16);
  return (uint32_t)(r < 0 ? r + q : r);
}

}  // namespace ntt

// built from make_ntt_plan(3329, 256); ok = false if the plan's leaf moduli are not FIPS 203's
ntt::FipsImageMap make_fips203_image_map();

}  // namespace psf
