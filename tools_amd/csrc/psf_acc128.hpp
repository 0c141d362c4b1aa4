// psf_acc128.hpp -- the signed 128-bit running total of the exact integer products over Z_q, and its reduction mod q.  Device helpers only (no kernel),
// so that both psf_kernels.hpp (the PSF unit) and psf_rq_kernels.hpp (the R_q product unit) can include it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psf {

struct Acc128 { uint64_t lo; int64_t hi; };
__device__ inline void acc128_add(Acc128& t, int64_t v) {
  const uint64_t nl = t.lo + (uint64_t)v;
  t.hi += (v >> 63) + (nl < t.lo ? 1 : 0);
  t.lo = nl;
}
// (hi * 2^64 + lo) mod q for |hi| small; two64 = 2^64 mod q
__device__ inline uint64_t acc128_mod(Acc128 t, uint64_t q, uint64_t two64) {
  uint64_t r = t.lo % q;
  int64_t h = t.hi;
  const bool neg = h < 0;
  uint64_t hm = (uint64_t)(neg ? -h : h);
  // hm * two64 mod q by double-and-add (hm < 2^16 in every use)
  uint64_t term = 0, base = two64;
  while (hm) {
    if (hm & 1) { term += base; if (term >= q) term -= q; }
    base += base; if (base >= q) base -= q;
    hm >>= 1;
  }
  if (neg) { r = r >= term ? r - term : r + q - term; }
  else { r += term; if (r >= q) r -= q; }
  return r;
}

}  // namespace psf
