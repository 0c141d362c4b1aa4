// psf_keccak_core.hpp -- Keccak-f[1600] with ONE state per lane, and what FIPS 202 / FIPS 203 build on it: the sponge (absorb with pad10*1 and the
// domain bytes 0x06 of SHA3 and 0x1F of SHAKE, squeeze), the parse loop of SampleNTT (FIPS 203 Algorithm 7) and the bit fields of SamplePolyCBD
// (Algorithm 8).
//
// The state is 25 64-bit lanes s[x + 5 y] held in registers: every index into it is a compile-time constant once the loops below are unrolled, and
// the 24 rounds are a rolled loop (theta and rho-pi write a second array b, chi writes s back, so no lane is ever moved).  All messages of a launch
// have one length, so the control flow of the sponge is uniform across a wave; only the rejection loop of SampleNTT is per lane, and its one
// wave-level question ("is every lane done?") goes through Ops::all.
//
// The code is written over a small back end Ops (a three-input xor, chi, a rotation, the wave vote): the device back end uses the three-operand bit
// operation and the 64-bit funnel shift of gfx950 on 32-bit halves (180 vector instructions per round against 290 for the plain C++ form compiled
// for the device, and faster on the MI355X in every call that was timed: DESIGN.md); the plain C++ back end is what g++ compiles for
// tests/cpp/keccak_host_check.cpp, which checks this same text against hashlib without a GPU (tests/test_keccak_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PSF_KC_FN __device__ __forceinline__
#else
#define PSF_KC_FN inline
#endif

namespace psf {
namespace kc {

enum : uint32_t { kDomSha3 = 0x06, kDomShake = 0x1F };
constexpr int kRateSha3_256 = 136, kRateSha3_512 = 72, kRateShake128 = 168, kRateShake256 = 136;
constexpr uint32_t kQ = 3329, kN = 256;                                 // FIPS 203

// ---- back ends --------------------------------------------------------------------------------------------------------------------------------
struct PlainOps {
  static PSF_KC_FN uint64_t xor3(uint64_t a, uint64_t b, uint64_t c) { return a ^ (b ^ c); }
  static PSF_KC_FN uint64_t chi(uint64_t a, uint64_t b, uint64_t c) { return a ^ (~b & c); }
  static PSF_KC_FN uint64_t rotl(uint64_t a, int r) { return r == 0 ? a : (a << r) | (a >> (64 - r)); }
  static PSF_KC_FN bool all(bool p) { return p; }
};

#if defined(__HIPCC__)
// v_bitop3_b32 takes the truth table of f(a, b, c) with a = 0xF0, b = 0xCC, c = 0xAA; v_alignbit_b32(hi, lo, s) is the low word of (hi:lo) >> s
struct DevOps {
  static PSF_KC_FN uint64_t join(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
  static PSF_KC_FN uint64_t xor3(uint64_t a, uint64_t b, uint64_t c) {
    return join(__builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b, (uint32_t)c, 0x96),
                __builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32), 0x96));
  }
  static PSF_KC_FN uint64_t chi(uint64_t a, uint64_t b, uint64_t c) {     // a ^ (~b & c): 0xF0 ^ (0x33 & 0xAA)
    return join(__builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b, (uint32_t)c, 0xD2),
                __builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32), 0xD2));
  }
  static PSF_KC_FN uint64_t rotl(uint64_t a, int r) {                     // r is a constant after unrolling
    const uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
    if (r == 0) return a;
    if (r == 32) return join(hi, lo);
    if (r < 32) return join(__builtin_amdgcn_alignbit(lo, hi, 32 - r), __builtin_amdgcn_alignbit(hi, lo, 32 - r));
    return join(__builtin_amdgcn_alignbit(hi, lo, 64 - r), __builtin_amdgcn_alignbit(lo, hi, 64 - r));
  }
  static PSF_KC_FN bool all(bool p) { return __all(p); }
};
#endif

// ---- the permutation ----------------------------------------------------------------------------------------------------------------------------
template <class Ops> PSF_KC_FN void f1600(uint64_t (&s)[25]) {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
      0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
      0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
      0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // rho, at x + 5 y
#pragma clang loop unroll(disable)
  for (int round = 0; round < 24; ++round) {
    uint64_t c[5], r1[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; ++x) c[x] = Ops::xor3(Ops::xor3(s[x], s[x + 5], s[x + 10]), s[x + 15], s[x + 20]);
#pragma unroll
    for (int x = 0; x < 5; ++x) r1[x] = Ops::rotl(c[(x + 1) % 5], 1);
    // theta, rho and pi in one pass: b[y, 2x + 3y] = rotl(s[x, y] ^ c[x - 1] ^ rotl(c[x + 1], 1), ROT[x, y])
#pragma unroll
    for (int y = 0; y < 5; ++y)
#pragma unroll
      for (int x = 0; x < 5; ++x) b[y + 5 * ((2 * x + 3 * y) % 5)] = Ops::rotl(Ops::xor3(s[x + 5 * y], c[(x + 4) % 5], r1[x]), ROT[x + 5 * y]);
#pragma unroll
    for (int y = 0; y < 5; ++y)
#pragma unroll
      for (int x = 0; x < 5; ++x) s[x + 5 * y] = Ops::chi(b[x + 5 * y], b[(x + 1) % 5 + 5 * y], b[(x + 2) % 5 + 5 * y]);
    s[0] ^= RC[round];
  }
}

// ---- the sponge ---------------------------------------------------------------------------------------------------------------------------------
// A message is read through Rd: byte(pos), and le64(pos) for 8 bytes that all lie inside the message.  A digest leaves through Wr: put64(pos, w) and
// put8(pos, b).  Bytes at or beyond the length are never read or written.

// bytes of a buffer; `aligned`: the address of byte 0 is a multiple of 8 (every pos asked of le64 / put64 is one: the rates are)
struct PtrReader {
  const uint8_t* p;
  bool aligned;
  PSF_KC_FN uint8_t byte(size_t pos) const { return p[pos]; }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    uint64_t w = 0;
    if (aligned) { __builtin_memcpy(&w, __builtin_assume_aligned(p + pos, 8), 8); return w; }
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)p[pos + k] << (8 * k);
    return w;
  }
};
struct PtrWriter {
  uint8_t* p;
  bool aligned;
  PSF_KC_FN void put8(size_t pos, uint8_t v) const { p[pos] = v; }
  PSF_KC_FN void put64(size_t pos, uint64_t w) const {
    if (aligned) { __builtin_memcpy(__builtin_assume_aligned(p + pos, 8), &w, 8); return; }
#pragma unroll
    for (int k = 0; k < 8; ++k) p[pos + k] = (uint8_t)(w >> (8 * k));
  }
};
// n bytes of a buffer followed by the bytes of `tail`, least significant first: rho || j || i of SampleNTT, sigma || N of PRF
struct SeedReader {
  const uint8_t* p;
  uint32_t n, tail;
  PSF_KC_FN uint8_t byte(size_t pos) const { return pos < n ? p[pos] : (uint8_t)(tail >> (8 * (pos - n))); }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte(pos + k) << (8 * k);
    return w;
  }
};

// the 8 bytes at pos of message || dom || 0 ..., with `avail` message bytes left from pos on (may be negative)
template <class Rd> PSF_KC_FN uint64_t le64_padded(const Rd& rd, size_t pos, long long avail, uint32_t dom) {
  if (avail >= 8) return rd.le64(pos);
  uint64_t w = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint64_t v = 0;
    if (k < avail) v = rd.byte(pos + k);
    else if (k == avail) v = dom;
    w |= v << (8 * k);
  }
  return w;
}

// absorbs the whole message and the padding: on return the state holds the first block of output
template <int RATE, class Ops, class Rd> PSF_KC_FN void absorb(uint64_t (&s)[25], const Rd& rd, size_t len, uint32_t dom) {
  static_assert(RATE % 8 == 0 && RATE > 0 && RATE < 200, "rate in whole lanes");
  size_t off = 0;
  for (; len - off >= (size_t)RATE; off += RATE) {
#pragma unroll
    for (int i = 0; i < RATE / 8; ++i) s[i] ^= rd.le64(off + 8 * i);
    f1600<Ops>(s);
  }
  const long long rem = (long long)(len - off);                           // 0 ... RATE - 1
#pragma unroll
  for (int i = 0; i < RATE / 8; ++i) s[i] ^= le64_padded(rd, off + 8 * i, rem - 8 * i, dom);
  s[RATE / 8 - 1] ^= 0x8000000000000000ull;
  f1600<Ops>(s);
}

template <int RATE, class Ops, class Wr> PSF_KC_FN void squeeze(uint64_t (&s)[25], const Wr& wr, size_t out_len) {
  for (size_t off = 0;; off += RATE) {
    const size_t rem = out_len - off;                                     // >= 1
#pragma unroll
    for (int i = 0; i < RATE / 8; ++i) {
      const long long avail = (long long)(rem < (size_t)RATE ? rem : (size_t)RATE) - 8 * i;
      if (avail >= 8) wr.put64(off + 8 * i, s[i]);
      else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < avail) wr.put8(off + 8 * i + k, (uint8_t)(s[i] >> (8 * k)));
      }
    }
    if (rem <= (size_t)RATE) return;
    f1600<Ops>(s);
  }
}

// what the kernels with a state of their own do around absorb: the empty state, words of the state as bytes, the `aligned` of a reader over rows
PSF_KC_FN void zero_state(uint64_t (&s)[25]) {
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
}
// words s[first ... first + COUNT - 1] of a state as 8 COUNT bytes at p
template <int FIRST, int COUNT> PSF_KC_FN void put_words(const uint64_t (&s)[25], uint8_t* p) {
  const PtrWriter wr{p, (uintptr_t)p % 8 == 0};
#pragma unroll
  for (int i = 0; i < COUNT; ++i) wr.put64(8 * i, s[FIRST + i]);
}
PSF_KC_FN bool aligned8(const void* p, size_t pitch) { return ((uintptr_t)p | pitch) % 8 == 0; }

template <int RATE, class Ops, class Rd, class Wr>
PSF_KC_FN void hash(const Rd& rd, size_t in_len, uint32_t dom, const Wr& wr, size_t out_len) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
  absorb<RATE, Ops>(s, rd, in_len, dom);
  squeeze<RATE, Ops>(s, wr, out_len);
}

// ---- SampleNTT (FIPS 203 Algorithm 7) --------------------------------------------------------------------------------------------------------------
// s: the state after absorb<168>(B, 34 bytes, 0x1F).  Every 3 bytes of the stream give d1 = b0 + 256 (b1 mod 16) and d2 = floor(b1 / 16) + 16 b2;
// each one below q is the next coefficient: put(j, d).  The loop ends when every lane of the wave (Ops::all) has its 256 coefficients, or after
// max_blocks blocks of 168 bytes: a lane that is still short then gets zeros for the rest and the function returns true.
constexpr int kSampleNttMaxBlocks = 8;                                    // P(more than 6 blocks) < 2^-440 at acceptance 3329 / 4096
template <class Ops, class Put> PSF_KC_FN bool sample_ntt_parse(uint64_t (&s)[25], Put&& put, int max_blocks) {
  uint32_t j = 0;
  for (int blk = 1;; ++blk) {
#pragma unroll
    for (int t = 0; t < kRateShake128 / 3; ++t) {
      constexpr int kLane = 64;
      const int w = (24 * t) / kLane, sh = (24 * t) % kLane;
      uint32_t c = (uint32_t)(s[w] >> sh);
      if (sh > kLane - 24) c |= (uint32_t)(s[w + 1] << (kLane - sh));
      const uint32_t d1 = c & 0xFFFu, d2 = (c >> 12) & 0xFFFu;
      if (d1 < kQ && j < kN) put(j++, d1);
      if (d2 < kQ && j < kN) put(j++, d2);
    }
    if (Ops::all(j >= kN) || blk >= max_blocks) break;
    f1600<Ops>(s);
  }
  const bool fail = j < kN;
  for (; j < kN; ++j) put(j, 0u);
  return fail;
}

// ---- SamplePolyCBD_eta (Algorithm 8) ---------------------------------------------------------------------------------------------------------------
// w: the 64 eta bytes of PRF_eta as 8 eta little-endian words.  Coefficient i = popcount(bits [2 eta i, 2 eta i + eta)) - popcount(the next eta bits);
// ETA words hold 32 coefficients exactly.
template <int ETA, class Put> PSF_KC_FN void cbd_fields(const uint64_t (&w)[8 * ETA], Put&& put) {
  static_assert(ETA == 2 || ETA == 3, "FIPS 203 uses eta = 2 and eta = 3");
  constexpr uint32_t lomask = (1u << ETA) - 1;
#pragma unroll
  for (int g = 0; g < 8; ++g)
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const int bit = 2 * ETA * k, wd = bit / 64, sh = bit % 64;
      uint32_t f = (uint32_t)(w[g * ETA + wd] >> sh);
      if (sh > 64 - 2 * ETA) f |= (uint32_t)(w[g * ETA + wd + 1] << (64 - sh));
      const int v = __builtin_popcount(f & lomask) - __builtin_popcount((f >> ETA) & lomask);
      put((uint32_t)(32 * g + k), v);
    }
}

// PRF_eta(sigma, N) = SHAKE256(sigma || N, 64 eta) into w, through a state the caller no longer needs
template <int ETA, class Ops, class Rd> PSF_KC_FN void prf_words(const Rd& rd, uint64_t (&w)[8 * ETA]) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
  absorb<kRateShake256, Ops>(s, rd, 33, kDomShake);
  constexpr int first = 8 * ETA < kRateShake256 / 8 ? 8 * ETA : kRateShake256 / 8;
#pragma unroll
  for (int i = 0; i < first; ++i) w[i] = s[i];
  if constexpr (8 * ETA > first) {
    f1600<Ops>(s);
#pragma unroll
    for (int i = first; i < 8 * ETA; ++i) w[i] = s[i - first];
  }
}

}  // namespace kc
}  // namespace psf
