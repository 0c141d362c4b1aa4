// psf_sha2_core.hpp -- SHA-256 and SHA-512 (FIPS 180-4) with ONE hash state per lane: the two compression functions, the general absorb over a byte
// reader (any length, the padding opening a block of its own when it must) and, through its `prior` argument, the "more blocks from a midstate" form that
// FIPS 205 section 11.2 needs: the state after whole blocks that depend on the key alone is kept, and only what follows is compressed.
//
// State and digest are big-endian WORDS (uint32_t[8] / uint64_t[8]): a digest feeds the next block without byte swaps.  The 64 / 80 rounds are fully
// unrolled (a fold over the round number) over the eight working variables and the 16-word schedule, all in registers: every index is a compile-time constant, so there is no
// run-time-indexed array and no private segment.  Only the loop over the blocks of a message is rolled.
//
// Written over a back end Ops like psf_keccak_core.hpp: the device back end takes rotations from v_alignbit_b32 and Sigma / sigma / Ch / Maj from the
// three-operand bit operation of gfx950, 64-bit values as pairs of 32-bit words; the plain C++ back end is what g++ compiles for
// tests/cpp/sha2_host_check.cpp, which checks this same text against hashlib without a GPU (tests/test_sha2_cpu.py).  Ops::tick(family) is called once
// per compression: nothing in both back ends, a counter in the host check of the FIPS 205 core.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>

#if defined(__HIPCC__)
#define PSF_KC_FN __device__ __forceinline__
#else
#define PSF_KC_FN inline
#endif

namespace psf {
namespace sha2 {

enum : int { kSha256 = 0, kSha512 = 1 };

// ---- back ends --------------------------------------------------------------------------------------------------------------------------------------
struct PlainOps {
  static PSF_KC_FN uint32_t rotr(uint32_t a, int r) { return (a >> r) | (a << (32 - r)); }
  static PSF_KC_FN uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
  static PSF_KC_FN uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return (e & f) ^ (~e & g); }
  static PSF_KC_FN uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) ^ (a & c) ^ (b & c); }
  static PSF_KC_FN uint64_t rotr(uint64_t a, int r) { return (a >> r) | (a << (64 - r)); }
  static PSF_KC_FN uint64_t xor3(uint64_t a, uint64_t b, uint64_t c) { return a ^ b ^ c; }
  static PSF_KC_FN uint64_t ch(uint64_t e, uint64_t f, uint64_t g) { return (e & f) ^ (~e & g); }
  static PSF_KC_FN uint64_t maj(uint64_t a, uint64_t b, uint64_t c) { return (a & b) ^ (a & c) ^ (b & c); }
  template <uint64_t K> static PSF_KC_FN uint64_t add_k(uint64_t x) { return x + K; }
  template <uint32_t K> static PSF_KC_FN uint32_t t1_256(uint32_t h, uint32_t s1, uint32_t ch, uint32_t w) { return h + s1 + ch + K + w; }
  static PSF_KC_FN void fence() {}
  static PSF_KC_FN void tick(int) {}
};

#if defined(__HIPCC__)
// v_bitop3_b32 takes the truth table of f(a, b, c) with a = 0xF0, b = 0xCC, c = 0xAA; v_alignbit_b32(hi, lo, s) is the low word of (hi:lo) >> s
struct DevOps {
  static PSF_KC_FN uint64_t join(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
  static PSF_KC_FN uint32_t rotr(uint32_t a, int r) { return __builtin_amdgcn_alignbit(a, a, r); }
  static PSF_KC_FN uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
  static PSF_KC_FN uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }       // (a & b) | (~a & c)
  static PSF_KC_FN uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
  static PSF_KC_FN uint64_t rotr(uint64_t a, int r) {                      // r is a constant, 1 ... 63
    const uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
    if (r == 32) return join(hi, lo);
    if (r < 32) return join(__builtin_amdgcn_alignbit(hi, lo, r), __builtin_amdgcn_alignbit(lo, hi, r));
    return join(__builtin_amdgcn_alignbit(lo, hi, r - 32), __builtin_amdgcn_alignbit(hi, lo, r - 32));
  }
  static PSF_KC_FN uint64_t xor3(uint64_t a, uint64_t b, uint64_t c) {
    return join(xor3((uint32_t)a, (uint32_t)b, (uint32_t)c), xor3((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32)));
  }
  static PSF_KC_FN uint64_t ch(uint64_t e, uint64_t f, uint64_t g) {
    return join(ch((uint32_t)e, (uint32_t)f, (uint32_t)g), ch((uint32_t)(e >> 32), (uint32_t)(f >> 32), (uint32_t)(g >> 32)));
  }
  static PSF_KC_FN uint64_t maj(uint64_t a, uint64_t b, uint64_t c) {
    return join(maj((uint32_t)a, (uint32_t)b, (uint32_t)c), maj((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32)));
  }
  // x + K for a round constant of SHA-512, the constant as literals of the add instructions.  Left to the compiler the 80 constants become 160
  // scalar registers that it treats as invariants of the loops around a compression: more than the scalar file holds, so they are spilled.
  template <uint64_t K> static PSF_KC_FN uint64_t add_k(uint64_t x) {
    uint32_t lo, hi;
    asm("v_add_co_u32_e32 %0, vcc, %2, %3\n\tv_addc_co_u32_e32 %1, vcc, 0, %5, vcc\n\tv_add_u32_e32 %1, %4, %1"   // a literal and vcc as a source are one too many
        : "=&v"(lo), "=v"(hi)
        : "i"((uint32_t)K), "v"((uint32_t)x), "i"((uint32_t)(K >> 32)), "v"((uint32_t)(x >> 32))
        : "vcc");
    return join(lo, hi);
  }
  template <uint32_t K> static PSF_KC_FN uint32_t t1_256(uint32_t h, uint32_t s1, uint32_t ch, uint32_t w) { return h + s1 + ch + K + w; }
  // Between two rounds of SHA-512: nothing is scheduled across.  Without it the scheduler runs the message schedule of all 80 rounds ahead of the
  // rounds that use it, and inside a loop with barriers (k_kg_tree) that needs more registers than there are.
  static PSF_KC_FN void fence() { __builtin_amdgcn_sched_barrier(0); }
  static PSF_KC_FN void tick(int) {}
};
#endif

// the round constants of SHA-256 and SHA-512: at namespace scope, so that one can be a template argument (DevOps::add_k)
constexpr uint32_t kK256[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
    0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
    0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
    0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
    0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
    0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
constexpr uint64_t kK512[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

// ---- the compression functions ------------------------------------------------------------------------------------------------------------------------
PSF_KC_FN void init256(uint32_t (&h)[8]) {
  constexpr uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = iv[i];
}
PSF_KC_FN void init512(uint64_t (&h)[8]) {
  constexpr uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                              0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = iv[i];
}

// Round T of SHA-256 / SHA-512, T a template argument: the rounds are unrolled by the language (a fold over 0 ... 63 / 79), not by an optimiser's
// threshold -- left as a loop with an unroll pragma, the 80 rounds of SHA-512 are over the threshold, stay a loop, and the schedule becomes a
// run-time-indexed register array.  The working variables a ... h are v[(0 - T) & 7] ... v[(7 - T) & 7]: nothing moves, the names do.
template <class Ops, int T> PSF_KC_FN void round256(uint32_t (&v)[8], uint32_t (&w)[16]) {
  if constexpr (T >= 16) {
    const uint32_t w15 = w[(T + 1) & 15], w2 = w[(T + 14) & 15];
    const uint32_t s0 = Ops::xor3(Ops::rotr(w15, 7), Ops::rotr(w15, 18), w15 >> 3);
    const uint32_t s1 = Ops::xor3(Ops::rotr(w2, 17), Ops::rotr(w2, 19), w2 >> 10);
    w[T & 15] = w[T & 15] + s0 + w[(T + 9) & 15] + s1;
  }
  uint32_t &a = v[(0 - T) & 7], &b = v[(1 - T) & 7], &c = v[(2 - T) & 7], &d = v[(3 - T) & 7];
  uint32_t &e = v[(4 - T) & 7], &f = v[(5 - T) & 7], &g = v[(6 - T) & 7], &hh = v[(7 - T) & 7];
  const uint32_t t1 = Ops::template t1_256<kK256[T]>(hh, Ops::xor3(Ops::rotr(e, 6), Ops::rotr(e, 11), Ops::rotr(e, 25)), Ops::ch(e, f, g), w[T & 15]);
  const uint32_t t2 = Ops::xor3(Ops::rotr(a, 2), Ops::rotr(a, 13), Ops::rotr(a, 22)) + Ops::maj(a, b, c);
  d += t1;
  hh = t1 + t2;
}
template <class Ops, int... T> PSF_KC_FN void rounds256(uint32_t (&v)[8], uint32_t (&w)[16], std::integer_sequence<int, T...>) {
  (round256<Ops, T>(v, w), ...);
}
template <class Ops, int T> PSF_KC_FN void round512(uint64_t (&v)[8], uint64_t (&w)[16]) {
  if constexpr (T % 2 == 0) Ops::fence();
  if constexpr (T >= 16) {
    const uint64_t w15 = w[(T + 1) & 15], w2 = w[(T + 14) & 15];
    const uint64_t s0 = Ops::xor3(Ops::rotr(w15, 1), Ops::rotr(w15, 8), w15 >> 7);
    const uint64_t s1 = Ops::xor3(Ops::rotr(w2, 19), Ops::rotr(w2, 61), w2 >> 6);
    w[T & 15] = w[T & 15] + s0 + w[(T + 9) & 15] + s1;
  }
  uint64_t &a = v[(0 - T) & 7], &b = v[(1 - T) & 7], &c = v[(2 - T) & 7], &d = v[(3 - T) & 7];
  uint64_t &e = v[(4 - T) & 7], &f = v[(5 - T) & 7], &g = v[(6 - T) & 7], &hh = v[(7 - T) & 7];
  const uint64_t t1 = Ops::template add_k<kK512[T]>(hh + Ops::xor3(Ops::rotr(e, 14), Ops::rotr(e, 18), Ops::rotr(e, 41)) + Ops::ch(e, f, g) + w[T & 15]);
  const uint64_t t2 = Ops::xor3(Ops::rotr(a, 28), Ops::rotr(a, 34), Ops::rotr(a, 39)) + Ops::maj(a, b, c);
  d += t1;
  hh = t1 + t2;
}
template <class Ops, int... T> PSF_KC_FN void rounds512(uint64_t (&v)[8], uint64_t (&w)[16], std::integer_sequence<int, T...>) {
  (round512<Ops, T>(v, w), ...);
}

// h = compress(h, the block w[0 ... 15]); w is used up as the schedule
template <class Ops> PSF_KC_FN void compress256(uint32_t (&h)[8], uint32_t (&w)[16]) {
  Ops::tick(kSha256);
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = h[i];
  rounds256<Ops>(v, w, std::make_integer_sequence<int, 64>{});
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] += v[i];
}

template <class Ops> PSF_KC_FN void compress512(uint64_t (&h)[8], uint64_t (&w)[16]) {
  Ops::tick(kSha512);
  uint64_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = h[i];
  rounds512<Ops>(v, w, std::make_integer_sequence<int, 80>{});
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] += v[i];
}

// ---- messages -------------------------------------------------------------------------------------------------------------------------------------------
// A message is read through Rd: byte(pos), and be32(pos) for 4 bytes that all lie inside the message.  Bytes at or beyond the length are never read.

// bytes of a buffer; `aligned`: the address of byte 0 is a multiple of 4 (every pos asked of be32 is one)
struct PtrReader {
  const uint8_t* p;
  bool aligned;
  PSF_KC_FN uint8_t byte(size_t pos) const { return p[pos]; }
  PSF_KC_FN uint32_t be32(size_t pos) const {
    if (aligned) {
      uint32_t w;
      __builtin_memcpy(&w, __builtin_assume_aligned(p + pos, 4), 4);
      return __builtin_bswap32(w);
    }
    return ((uint32_t)p[pos] << 24) | ((uint32_t)p[pos + 1] << 16) | ((uint32_t)p[pos + 2] << 8) | p[pos + 3];
  }
};
// a reader with byte() alone
template <class Rd> struct ByteReader {
  Rd rd;
  PSF_KC_FN uint8_t byte(size_t pos) const { return rd.byte(pos); }
  PSF_KC_FN uint32_t be32(size_t pos) const {
    return ((uint32_t)rd.byte(pos) << 24) | ((uint32_t)rd.byte(pos + 1) << 16) | ((uint32_t)rd.byte(pos + 2) << 8) | rd.byte(pos + 3);
  }
};

// the 4 bytes at pos of message || 0x80 || 0 ..., big-endian, with `avail` message bytes left from pos on (may be negative)
template <class Rd> PSF_KC_FN uint32_t be32_padded(const Rd& rd, size_t pos, long long avail) {
  if (avail >= 4) return rd.be32(pos);
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t v = 0;
    if (k < avail) v = rd.byte(pos + k);
    else if (k == avail) v = 0x80;
    w |= v << (24 - 8 * k);
  }
  return w;
}

// The 16 words word(0) ... word(15) of a block into w.  ROLLED (always, for the padded last blocks: every byte of those is a comparison with the
// length, which is uniform, so unrolled they hold a scalar mask per byte, more than the scalar file has): one word per turn of a loop that is not unrolled, w moving down one place each turn, so
// that every index stays a constant: for readers whose every byte is a choice between buffers (H_msg's), where sixteen unrolled copies of the reading
// cost more registers than there are; 16 register moves per word are nothing beside a compression.
template <bool ROLLED, class W, class F> PSF_KC_FN void fill_block(W (&w)[16], F&& word) {
  if constexpr (ROLLED) {
#pragma clang loop unroll(disable)
    for (int i = 0; i < 16; ++i) {
#pragma unroll
      for (int j = 0; j < 15; ++j) w[j] = w[j + 1];
      w[15] = word(i);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = word(i);
  }
}

// Absorbs the `len` bytes of rd and the padding into h, which holds the state after `prior` bytes (a multiple of 64; 0 with init256): on return h is the
// digest of those prior bytes followed by the message.  rem <= 55: the padding and the length share the last block; else they open one more.
template <class Ops, class Rd, bool ROLLED = false> PSF_KC_FN void absorb256(uint32_t (&h)[8], const Rd& rd, size_t len, uint64_t prior) {
  uint32_t w[16];
  size_t off = 0;
  for (; len - off >= 64; off += 64) {
    fill_block<ROLLED>(w, [&](int i) { return rd.be32(off + 4 * i); });
    compress256<Ops>(h, w);
  }
  const long long rem = (long long)(len - off);                           // 0 ... 63
  const uint64_t bits = (prior + len) * 8;
  // one or two more blocks through ONE call site of the compression: block 0 is the tail and the 0x80, the length goes into the last
  const int last = rem <= 55 ? 0 : 1;
  for (int b = 0; b <= last; ++b) {
    fill_block<true>(w, [&](int i) { return b == 0 ? be32_padded(rd, off + 4 * i, rem - 4 * i) : 0u; });
    if (b == last) {
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    compress256<Ops>(h, w);
  }
}

// the same for SHA-512: blocks of 128 bytes, `prior` a multiple of 128, a 128-bit length of which the low 67 bits can be other than zero
template <class Ops, class Rd, bool ROLLED = false> PSF_KC_FN void absorb512(uint64_t (&h)[8], const Rd& rd, size_t len, uint64_t prior) {
  uint64_t w[16];
  size_t off = 0;
  for (; len - off >= 128; off += 128) {
    fill_block<ROLLED>(w, [&](int i) { return ((uint64_t)rd.be32(off + 8 * i) << 32) | rd.be32(off + 8 * i + 4); });
    compress512<Ops>(h, w);
  }
  const long long rem = (long long)(len - off);                           // 0 ... 127
  const uint64_t bytes = prior + len;
  const int last = rem <= 111 ? 0 : 1;
  for (int b = 0; b <= last; ++b) {
    fill_block<true>(w, [&](int i) {
      return b == 0 ? ((uint64_t)be32_padded(rd, off + 8 * i, rem - 8 * i) << 32) | be32_padded(rd, off + 8 * i + 4, rem - 8 * i - 4) : 0ull;
    });
    if (b == last) {
      w[14] = bytes >> 61;
      w[15] = bytes << 3;
    }
    compress512<Ops>(h, w);
  }
}

// ---- digests ----------------------------------------------------------------------------------------------------------------------------------------------
// the leading out_len bytes (1 ... 32) of the digest h at p: FIPS 205's Trunc
PSF_KC_FN void put_digest256(const uint32_t (&h)[8], uint8_t* p, size_t out_len) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((size_t)(4 * i + k) < out_len) p[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
}
PSF_KC_FN void put_digest512(const uint64_t (&h)[8], uint8_t* p, size_t out_len) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if ((size_t)(8 * i + k) < out_len) p[8 * i + k] = (uint8_t)(h[i] >> (56 - 8 * k));
}

}  // namespace sha2
}  // namespace psf
