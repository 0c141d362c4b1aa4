// psf_mlkem.hip -- ML-KEM (FIPS 203) on the device, batched: KeyGen_internal, Encaps_internal and Decaps_internal (Algorithms 16 to 18) and the two
// input checks of sections 7.2 / 7.3, bytes in and bytes out, `count` instances per call.  The pieces below the KEM are the library's own entry
// points (the SHAKE samplers, the NTT-domain interop, the forward transform, the fused products E +- A B); this unit adds what ties them together:
//   k_g            G over gathered inputs (d || k, m || H(ek), m' || h with h read in place from dk), through the sponge of psf_keccak_core.hpp
//   k_encaps_hash  H(ek) and G(m || H(ek)) in one lane
//   k_unpack       ByteDecode_12 / Decompress_d(ByteDecode_d) from an instance pitch (ek, dk, c) into 16-bit words
//   k_pack         ByteEncode_12 / ByteEncode_d(Compress_d) from 16-bit words to an instance pitch (ek, dk, c, c', m')
//   k_canon        the canonical residues of s before its forward transform
//   k_add_msg      e2 + Decompress_1(m): the message bytes go straight into the addend of the v product
//   k_keygen_tail  H(ek), and rho, H(ek), z placed in dk
//   k_decaps_tail  J(z || c), the comparison of c with c' and the selection of K, in one kernel
//   k_check_ek / k_check_dk   the per-instance modulus check and hash check
// Everything secret lives in the caller's workspace, which the last operation of every entry point clears (DESIGN.md "ML-KEM").
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_keccak_core.hpp"

namespace psf {
namespace mlkem {

using kc::aligned8;
using kc::kDomSha3;
using kc::kDomShake;
using kc::kN;
using kc::kQ;
using kc::put_words;
using kc::zero_state;

// ---- readers ---------------------------------------------------------------------------------------------------------------------------------
// na bytes of a, then nb bytes of b, then the bytes of `tail`, least significant first.  fast: a and b are multiples of 8 and so is na, so every
// 8-byte group that lies inside one buffer is one load.
struct CatReader {
  const uint8_t* a;
  const uint8_t* b;
  uint32_t na, nb, tail;
  bool fast;
  PSF_KC_FN uint8_t byte(size_t pos) const {
    if (pos < na) return a[pos];
    if (pos - na < nb) return b[pos - na];
    return (uint8_t)(tail >> (8 * (pos - na - nb)));
  }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    uint64_t w = 0;
    if (fast && pos + 8 <= na) { __builtin_memcpy(&w, __builtin_assume_aligned(a + pos, 8), 8); return w; }
    if (fast && pos >= na && pos - na + 8 <= nb) { __builtin_memcpy(&w, __builtin_assume_aligned(b + (pos - na), 8), 8); return w; }
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte(pos + k) << (8 * k);
    return w;
  }
};

// ---- hashes ------------------------------------------------------------------------------------------------------------------------------------
// (o0, o1) = G(a_c || b_c || tail): a_c is 32 bytes at a + c a_pitch, b_c nb bytes at b + c b_pitch; 32 bytes each to o0 + c o0_pitch and o1 + c o1_pitch
struct GArgs {
  size_t count;
  const uint8_t* a; size_t a_pitch;
  const uint8_t* b; size_t b_pitch;
  uint32_t nb, tail, len;
  uint8_t* o0; size_t o0_pitch;
  uint8_t* o1; size_t o1_pitch;
};
__global__ __launch_bounds__(256) void k_g(GArgs g) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= g.count) return;
  uint64_t s[25];
  zero_state(s);
  const CatReader rd{g.a + c * g.a_pitch, g.b + c * g.b_pitch, 32, g.nb, g.tail, aligned8(g.a, g.a_pitch) && aligned8(g.b, g.b_pitch)};
  kc::absorb<kc::kRateSha3_512, kc::DevOps>(s, rd, g.len, kDomSha3);
  put_words<0, 4>(s, g.o0 + c * g.o0_pitch);
  put_words<4, 4>(s, g.o1 + c * g.o1_pitch);
}

// Encaps: h = H(ek_c) (kept in the workspace: public), (K, r) = G(m_c || h)
struct EncHashArgs { size_t count, ek_len; const uint8_t* ek; const uint8_t* m; uint8_t* h; uint8_t* K; uint8_t* r; };
__global__ __launch_bounds__(256) void k_encaps_hash(EncHashArgs e) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= e.count) return;
  uint64_t s[25];
  zero_state(s);
  kc::absorb<kc::kRateSha3_256, kc::DevOps>(s, kc::PtrReader{e.ek + c * e.ek_len, aligned8(e.ek, e.ek_len)}, e.ek_len, kDomSha3);
  uint8_t* h = e.h + c * 32;
  put_words<0, 4>(s, h);
  uint64_t g[25];
  zero_state(g);
  const CatReader rd{e.m + c * 32, h, 32, 32, 0, aligned8(e.m, 32)};     // h is read back by the lane that wrote it
  kc::absorb<kc::kRateSha3_512, kc::DevOps>(g, rd, 64, kDomSha3);
  put_words<0, 4>(g, e.K + c * 32);
  put_words<4, 4>(g, e.r + c * 32);
}

// KeyGen: dk_c = dk_pke || ek || H(ek) || z -- the two encodings are in place (k_pack); this adds rho, H(ek) and z
struct KgTailArgs { size_t count, ek_len, dk_len; uint32_t k; const uint8_t* ek; const uint8_t* z; uint8_t* dk; };
__global__ __launch_bounds__(256) void k_keygen_tail(KgTailArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* ek = a.ek + c * a.ek_len;
  uint8_t* dk = a.dk + c * a.dk_len;
  uint64_t s[25];
  zero_state(s);
  kc::absorb<kc::kRateSha3_256, kc::DevOps>(s, kc::PtrReader{ek, aligned8(a.ek, a.ek_len)}, a.ek_len, kDomSha3);
  put_words<0, 4>(s, dk + 768 * a.k + 32);
  for (int i = 0; i < 32; ++i) {
    dk[768 * a.k + i] = ek[384 * a.k + i];
    dk[768 * a.k + 64 + i] = a.z[c * 32 + i];
  }
}

// ---- the polynomial glue -------------------------------------------------------------------------------------------------------------------------
// A segment: `polys` polynomials per instance, instance c's bytes at bytes + c pitch (32 d bytes per polynomial), its words at words + c polys 256.
// A thread moves 8 values = d bytes: 16 bytes of words (one vector, the workspace is 256-byte aligned) and d single bytes (no alignment asked of
// keys and ciphertexts); neighbouring threads touch neighbouring bytes.
enum { MODE_RAW = 0, MODE_MAP = 1 };      // unpack: the residue mod q (d = 12) / Decompress_d; pack: the value as it is / Compress_d
struct Seg { const uint8_t* bytes; uint16_t* words; size_t pitch; uint32_t polys, d, mode; };
struct SegArgs { size_t count; Seg seg[4]; };

__global__ __launch_bounds__(256) void k_unpack(SegArgs a) {
  const Seg sg = a.seg[blockIdx.y];
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)sg.polys * 32;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint8_t* src = sg.bytes + inst * sg.pitch + (g - inst * per) * sg.d;
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (uint32_t k = 0; k < 12; ++k)
    if (k < sg.d) {
      const uint64_t by = src[k];
      if (k < 8) lo |= by << (8 * k);
      else hi |= by << (8 * (k - 8));
    }
  const uint32_t mask = (1u << sg.d) - 1;
  uint32_t x[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t bit = j * sg.d;                                       // <= 84
    uint64_t v;
    if (bit < 64) { v = lo >> bit; if (bit + sg.d > 64) v |= hi << (64 - bit); }     // bit + d > 64 only for bit >= 53
    else v = hi >> (bit - 64);
    const uint32_t y = (uint32_t)v & mask;
    x[j] = sg.mode == MODE_RAW ? y - (y >= kQ ? kQ : 0u) : (y * kQ + (1u << (sg.d - 1))) >> sg.d;      // y < 2^12 < 2 q; Decompress_d < q for d < 12
  }
  v4u r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = x[2 * j] | (x[2 * j + 1] << 16);
  *reinterpret_cast<v4u*>(sg.words + g * 8) = r;
}

// words in [0, q)
__global__ __launch_bounds__(256) void k_pack(SegArgs a) {
  const Seg sg = a.seg[blockIdx.y];
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)sg.polys * 32;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  uint8_t* dst = const_cast<uint8_t*>(sg.bytes) + inst * sg.pitch + (g - inst * per) * sg.d;
  const v4u w = *reinterpret_cast<const v4u*>(sg.words + g * 8);
  const uint32_t mask = (1u << sg.d) - 1;
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t x = (w[j / 2] >> (16 * (j & 1))) & 0xffffu;
    const uint64_t y = (sg.mode == MODE_RAW ? x : ((x << sg.d) + kQ / 2) / kQ) & mask;       // (q - 1) 2^12 + q / 2 < 2^24
    const uint32_t bit = j * sg.d;
    if (bit < 64) { lo |= y << bit; if (bit + sg.d > 64) hi |= y >> (64 - bit); }
    else hi |= y << (bit - 64);
  }
#pragma unroll
  for (uint32_t k = 0; k < 12; ++k)
    if (k < sg.d) dst[k] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
}

// signed words in (-q, q) -> [0, q), in place; 8 words per thread
__global__ __launch_bounds__(256) void k_canon(uint16_t* __restrict__ words, size_t nvec) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nvec) return;
  v4u w = reinterpret_cast<v4u*>(words)[g];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t lo = w[j] & 0xffffu, hi = w[j] >> 16;
    const uint32_t lo_c = (lo + (lo >> 15) * kQ) & 0xffffu, hi_c = (hi + (hi >> 15) * kQ) & 0xffffu;     // bit 15: the sign of the half
    w[j] = lo_c | (hi_c << 16);
  }
  reinterpret_cast<v4u*>(words)[g] = w;
}

// e2_c += Decompress_1(ByteDecode_1(m_c)): bit i of the 32 bytes at m + 32 c adds ceil(q / 2) = 1665 to coefficient i; e2 in [-eta2, eta2] stays in (-q, q)
__global__ __launch_bounds__(256) void k_add_msg(uint16_t* __restrict__ e2, const uint8_t* __restrict__ m, size_t nvec) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nvec) return;
  const uint32_t by = m[g];                                              // instance g / 32, byte g mod 32: the buffer is contiguous
  v4u w = reinterpret_cast<v4u*>(e2)[g];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t b0 = (by >> (2 * j)) & 1u, b1 = (by >> (2 * j + 1)) & 1u;
    w[j] = (((w[j] & 0xffffu) + b0 * ((kQ + 1) / 2)) & 0xffffu) | ((((w[j] >> 16) + b1 * ((kQ + 1) / 2)) & 0xffffu) << 16);
  }
  reinterpret_cast<v4u*>(e2)[g] = w;
}

// ---- the decapsulation tail ----------------------------------------------------------------------------------------------------------------------
// A workgroup of four waves, 64 instances.  First the comparison: each wave takes 16 of the instances, 8 at a time with the whole wave on each -- lane
// l reads elements l, l + 64, ... of c and of c' (consecutive lanes, consecutive addresses; the loads of the 8 instances are independent and in
// flight together), ORs their differences, and a butterfly of 6 exchanges leaves the OR of all 64 lanes in every lane, which goes to LDS.  Every byte
// is read, the trip counts depend on the parameter set and on `count` alone.  Then the first wave runs J, one state per lane like every other hash
// here, and selects K = K' xor (mask and (K' xor K_bar)) with mask = all ones exactly when c != c'.
struct TailArgs { size_t count, ct_len, dk_len; uint32_t k; const uint8_t* dk; const uint8_t* ct; const uint8_t* cp; const uint8_t* kp; uint8_t* ss; };
__global__ __launch_bounds__(256) void k_decaps_tail(TailArgs a) {
  __shared__ uint32_t s_diff[64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t p0 = (size_t)blockIdx.x * 64, left = a.count - p0;
  const uint32_t np = left < 64 ? (uint32_t)left : 64u;
  const bool words = ((uintptr_t)a.ct | (uintptr_t)a.cp) % 4 == 0;        // ct_len is a multiple of 32
  for (uint32_t g = 0; g < 2; ++g) {
    const uint32_t first = wave * 16 + g * 8;
    const uint8_t* c[8];
    const uint8_t* c2[8];
    uint32_t d[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      const uint32_t p = first + u < np ? first + u : np - 1;            // past the end: the last instance again, its result unused
      c[u] = a.ct + (p0 + p) * a.ct_len;
      c2[u] = a.cp + (p0 + p) * a.ct_len;
      d[u] = 0;
    }
    if (words) {
      for (uint32_t i = lane; i < a.ct_len / 4; i += 64) {
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) d[u] |= reinterpret_cast<const uint32_t*>(c[u])[i] ^ reinterpret_cast<const uint32_t*>(c2[u])[i];
      }
    } else {
      for (uint32_t i = lane; i < a.ct_len; i += 64) {
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) d[u] |= (uint32_t)(c[u][i] ^ c2[u][i]);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
#pragma unroll
      for (int off = 32; off; off >>= 1) d[u] |= (uint32_t)__shfl_xor((int)d[u], off);
      if (lane == 0) s_diff[first + u] = d[u];
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const uint32_t mine = s_diff[lane];
  const size_t c = p0 + lane < a.count ? p0 + lane : a.count - 1;        // a lane past the end repeats the last instance and writes nothing
  const uint8_t* z = a.dk + c * a.dk_len + 768 * a.k + 64;
  const uint8_t* ct = a.ct + c * a.ct_len;
  uint64_t s[25];
  zero_state(s);
  const CatReader rd{z, ct, 32, (uint32_t)a.ct_len, 0, ((uintptr_t)z | (uintptr_t)ct) % 8 == 0};
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, rd, 32 + a.ct_len, kDomShake);
  const uint64_t mask = 0ull - (uint64_t)((mine | (0u - mine)) >> 31);
  const uint64_t* kp = reinterpret_cast<const uint64_t*>(a.kp) + c * 4;   // in the workspace: aligned
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t k1 = kp[i];
    s[i] = k1 ^ (mask & (k1 ^ s[i]));
  }
  if (p0 + lane < a.count) put_words<0, 4>(s, a.ss + c * 32);
}

// ---- the input checks ----------------------------------------------------------------------------------------------------------------------------
// section 7.2: a workgroup per instance, a thread per 3 bytes = two 12-bit fields of ek[0 : 384 k]
__global__ __launch_bounds__(256) void k_check_ek(const uint8_t* __restrict__ ek, size_t ek_len, uint32_t k, uint8_t* __restrict__ ok) {
  const uint8_t* p = ek + (size_t)blockIdx.x * ek_len;
  int bad = 0;
  for (uint32_t g = threadIdx.x; g < 128 * k; g += 256) {
    const uint32_t b0 = p[3 * g], b1 = p[3 * g + 1], b2 = p[3 * g + 2];
    bad |= (b0 | ((b1 & 15u) << 8)) >= kQ || ((b1 >> 4) | (b2 << 4)) >= kQ;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) ok[blockIdx.x] = bad ? 0 : 1;
}
// section 7.3: H(dk[384 k : 768 k + 32]) against dk[768 k + 32 : 768 k + 64], one instance per lane
__global__ __launch_bounds__(256) void k_check_dk(const uint8_t* dk, size_t dk_len, uint32_t k, size_t count, uint8_t* ok) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const uint8_t* p = dk + c * dk_len;
  uint64_t s[25];
  zero_state(s);
  const uint8_t* ek = p + 384 * k;
  kc::absorb<kc::kRateSha3_256, kc::DevOps>(s, kc::PtrReader{ek, (uintptr_t)ek % 8 == 0}, 384 * (size_t)k + 32, kDomSha3);
  const kc::PtrReader h{p + 768 * k + 32, false};
  uint64_t d = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) d |= s[i] ^ h.le64(8 * i);
  ok[c] = d == 0 ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
struct Set { uint32_t k, eta1, eta2, du, dv; size_t ek, dk, ct; };
bool set_of(int param, Set* s) {
  switch (param) {
    case PSF_MLKEM_512: *s = {2, 3, 2, 10, 4, 0, 0, 0}; break;
    case PSF_MLKEM_768: *s = {3, 2, 2, 10, 4, 0, 0, 0}; break;
    case PSF_MLKEM_1024: *s = {4, 2, 2, 11, 5, 0, 0, 0}; break;
    default: return false;
  }
  s->ek = 384 * (size_t)s->k + 32;
  s->dk = 768 * (size_t)s->k + 96;
  s->ct = 32 * ((size_t)s->du * s->k + s->dv);
  return true;
}

// The workspace of an operation: sections in a fixed order, each rounded up to 256 bytes.  `P` polynomials of 16-bit words take 512 P bytes, of image
// words 1024 P bytes.  Sections that one library call reads or writes as a whole are adjacent ([A | t | s]: one image_from; [t | s]: one forward
// transform and one image_to).
struct KeygenWs : Layout { size_t sigma, a_fips, a_hat, e, ts, st_hat, st_fips; };
struct EncapsWs : Layout { size_t h, r, fips, hat, y, e1, e2, u, v; };
struct DecapsWs : Layout { size_t fips, hat, u2, v2, w, mp, kp, rp, y, e1, e2, u, v, cp; };

KeygenWs keygen_ws(const Set& s, size_t count) {
  KeygenWs w;
  const u128 c = count, k = s.k, poly = 512;
  w.sigma = w.take(c * 32);
  w.a_fips = w.take(c * k * k * poly);
  w.a_hat = w.take(c * k * k * poly * 2);
  w.e = w.take(c * k * poly);
  w.ts = w.take(c * 2 * k * poly);
  w.st_hat = w.take(c * 2 * k * poly * 2);
  w.st_fips = w.take(c * 2 * k * poly);
  return w;
}
EncapsWs encaps_ws(const Set& s, size_t count) {
  EncapsWs w;
  const u128 c = count, k = s.k, poly = 512;
  w.h = w.take(c * 32);
  w.r = w.take(c * 32);
  w.fips = w.take(c * (k * k + k) * poly);
  w.hat = w.take(c * (k * k + k) * poly * 2);
  w.y = w.take(c * k * poly);
  w.e1 = w.take(c * k * poly);
  w.e2 = w.take(c * poly);
  w.u = w.take(c * k * poly);
  w.v = w.take(c * poly);
  return w;
}
DecapsWs decaps_ws(const Set& s, size_t count) {
  DecapsWs w;
  const u128 c = count, k = s.k, poly = 512;
  w.fips = w.take(c * (k * k + 2 * k) * poly);
  w.hat = w.take(c * (k * k + 2 * k) * poly * 2);
  w.u2 = w.take(c * k * poly);
  w.v2 = w.take(c * poly);
  w.w = w.take(c * poly);
  w.mp = w.take(c * 32);
  w.kp = w.take(c * 32);
  w.rp = w.take(c * 32);
  w.y = w.take(c * k * poly);
  w.e1 = w.take(c * k * poly);
  w.e2 = w.take(c * poly);
  w.u = w.take(c * k * poly);
  w.v = w.take(c * poly);
  w.cp = w.take(c * s.ct);
  return w;
}
Layout ws_need(const Set& s, size_t count, int op) {
  if (op == PSF_MLKEM_OP_KEYGEN) return keygen_ws(s, count);
  if (op == PSF_MLKEM_OP_ENCAPS) return encaps_ws(s, count);
  if (op == PSF_MLKEM_OP_DECAPS) return decaps_ws(s, count);
  return Layout{};
}

// a buffer of `len` bytes per instance, packed
Buf buf_of(const void* p, size_t len, bool out) { return Buf{p, len, len, out, false, 0}; }
psf_status launch_segs(bool pack, size_t count, const Seg* segs, int nseg, hipStream_t st) {
  SegArgs a{};
  a.count = count;
  uint32_t most = 0;
  for (int i = 0; i < nseg; ++i) { a.seg[i] = segs[i]; most = segs[i].polys > most ? segs[i].polys : most; }
  const dim3 grid(blocks_of(count * most * 32, 256), (unsigned)nseg);
  if (pack) hipLaunchKernelGGL(k_pack, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_unpack, grid, dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

uint16_t* words_at(void* ws, size_t off) { return reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(ws) + off); }
uint32_t* images_at(void* ws, size_t off) { return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + off); }
uint8_t* bytes_at(void* ws, size_t off) { return static_cast<uint8_t*>(ws) + off; }

// y, e1, e2 = the noise of K-PKE.Encrypt from the coins r (32 bytes per instance, contiguous), mu added to e2; u = A^T y + e1, v = t^T y + e2 + mu;
// c1 || c2 at out + c pitch.  a_hat, t_hat: the images of one instance after the other.
struct EncryptBufs { const uint8_t* r; const uint8_t* m; const uint32_t* a_hat; const uint32_t* t_hat; uint16_t *y, *e1, *e2, *u, *v; uint8_t* out; size_t pitch; };
psf_status encrypt(int device, const Set& s, size_t count, const EncryptBufs& b, hipStream_t st) {
  const size_t k = s.k;
  PSF_TRY(psf_sample_cbd_fips203_dev(device, count, s.eta1, b.r, 32, 0, s.k, b.y, 16, st));
  PSF_TRY(psf_sample_cbd_fips203_dev(device, count, s.eta2, b.r, 32, s.k, s.k, b.e1, 16, st));
  PSF_TRY(psf_sample_cbd_fips203_dev(device, count, s.eta2, b.r, 32, 2 * s.k, 1, b.e2, 16, st));
  hipLaunchKernelGGL(k_add_msg, dim3(blocks_of(count * 32, 256)), dim3(256), 0, st, b.e2, b.m, count * 32);
  HIP_TRY(hipGetLastError());
  PSF_TRY(psf_matpoly_mul_add_hat_dev(device, kQ, kN, count, k, k, 1, b.a_hat, k * k * kN, 1, b.y, b.e1, 1, b.u, 16, st));
  PSF_TRY(psf_matpoly_mul_add_hat_dev(device, kQ, kN, count, 1, k, 1, b.t_hat, k * kN, 1, b.y, b.e2, 1, b.v, 16, st));
  const Seg segs[2] = {{b.out, b.u, b.pitch, s.k, s.du, MODE_MAP}, {b.out + 32 * (size_t)s.du * k, b.v, b.pitch, 1, s.dv, MODE_MAP}};
  return launch_segs(true, count, segs, 2, st);
}

psf_status keygen_run(int device, const Set& s, size_t count, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk, void* ws, const KeygenWs& w, int* fail,
                      hipStream_t st) {
  const size_t k = s.k, polys = count * k;
  uint8_t* sigma = bytes_at(ws, w.sigma);
  uint16_t* a_fips = words_at(ws, w.a_fips);
  uint32_t* a_hat = images_at(ws, w.a_hat);
  uint16_t *e = words_at(ws, w.e), *t = words_at(ws, w.ts), *sv = t + polys * kN, *st_fips = words_at(ws, w.st_fips);
  uint32_t* st_hat = images_at(ws, w.st_hat);
  HIP_TRY(hipSetDevice(device));
  const GArgs g{count, d, 32, d, 32, 0, s.k, 33, ek + 384 * k, s.ek, sigma, 32};        // (rho, sigma) = G(d || k): rho lands in ek
  hipLaunchKernelGGL(k_g, dim3(blocks_of(count, 256)), dim3(256), 0, st, g);
  HIP_TRY(hipGetLastError());
  PSF_TRY(psf_sample_ntt_fips203_dev(device, count, s.k, ek + 384 * k, s.ek, a_fips, fail, 16, st));
  PSF_TRY(psf_ntt_image_from_fips203_dev(device, polys * k, a_fips, 16, a_hat, st));
  PSF_TRY(psf_sample_cbd_fips203_dev(device, count, s.eta1, sigma, 32, 0, s.k, sv, 16, st));
  PSF_TRY(psf_sample_cbd_fips203_dev(device, count, s.eta1, sigma, 32, s.k, s.k, e, 16, st));
  hipLaunchKernelGGL(k_canon, dim3(blocks_of(polys * 32, 256)), dim3(256), 0, st, sv, polys * 32);
  HIP_TRY(hipGetLastError());
  PSF_TRY(psf_matpoly_mul_add_hat_dev(device, kQ, kN, count, k, k, 1, a_hat, k * k * kN, 0, sv, e, 1, t, 16, st));        // t = A s + e
  PSF_TRY(psf_ntt_forward_dev(device, kQ, kN, 2 * polys, t, 16, st_hat, st));
  PSF_TRY(psf_ntt_image_to_fips203_dev(device, 2 * polys, st_hat, st_fips, 16, st));
  const Seg segs[3] = {{ek, st_fips, s.ek, s.k, 12, MODE_RAW}, {dk + 384 * k, st_fips, s.dk, s.k, 12, MODE_RAW}, {dk, st_fips + polys * kN, s.dk, s.k, 12, MODE_RAW}};
  PSF_TRY(launch_segs(true, count, segs, 3, st));
  const KgTailArgs ta{count, s.ek, s.dk, s.k, ek, z, dk};
  hipLaunchKernelGGL(k_keygen_tail, dim3(blocks_of(count, 256)), dim3(256), 0, st, ta);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

psf_status encaps_run(int device, const Set& s, size_t count, const uint8_t* ek, const uint8_t* m, uint8_t* ss, uint8_t* ct, void* ws, const EncapsWs& w, int* fail,
                      hipStream_t st) {
  const size_t k = s.k, polys = count * k;
  uint16_t* fips = words_at(ws, w.fips);
  uint32_t* hat = images_at(ws, w.hat);
  HIP_TRY(hipSetDevice(device));
  const EncHashArgs ha{count, s.ek, ek, m, bytes_at(ws, w.h), ss, bytes_at(ws, w.r)};
  hipLaunchKernelGGL(k_encaps_hash, dim3(blocks_of(count, 256)), dim3(256), 0, st, ha);
  HIP_TRY(hipGetLastError());
  PSF_TRY(psf_sample_ntt_fips203_dev(device, count, s.k, ek + 384 * k, s.ek, fips, fail, 16, st));
  const Seg in[1] = {{ek, fips + polys * k * kN, s.ek, s.k, 12, MODE_RAW}};
  PSF_TRY(launch_segs(false, count, in, 1, st));
  PSF_TRY(psf_ntt_image_from_fips203_dev(device, polys * k + polys, fips, 16, hat, st));
  const EncryptBufs eb{bytes_at(ws, w.r), m, hat, hat + polys * k * kN, words_at(ws, w.y), words_at(ws, w.e1), words_at(ws, w.e2), words_at(ws, w.u),
                       words_at(ws, w.v), ct, s.ct};
  PSF_TRY(encrypt(device, s, count, eb, st));
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

psf_status decaps_run(int device, const Set& s, size_t count, const uint8_t* dk, const uint8_t* ct, uint8_t* ss, void* ws, const DecapsWs& w, int* fail,
                      hipStream_t st) {
  const size_t k = s.k, polys = count * k;
  uint16_t* fips = words_at(ws, w.fips);
  uint16_t *t_fips = fips + polys * k * kN, *s_fips = t_fips + polys * kN;
  uint32_t* hat = images_at(ws, w.hat);
  const uint32_t *t_hat = hat + polys * k * kN, *s_hat = t_hat + polys * kN;
  uint16_t *u2 = words_at(ws, w.u2), *v2 = words_at(ws, w.v2), *wv = words_at(ws, w.w);
  uint8_t *mp = bytes_at(ws, w.mp), *kp = bytes_at(ws, w.kp), *rp = bytes_at(ws, w.rp), *cp = bytes_at(ws, w.cp);
  HIP_TRY(hipSetDevice(device));
  PSF_TRY(psf_sample_ntt_fips203_dev(device, count, s.k, dk + 768 * k, s.dk, fips, fail, 16, st));          // rho of the embedded ek
  const Seg in[4] = {{dk + 384 * k, t_fips, s.dk, s.k, 12, MODE_RAW}, {dk, s_fips, s.dk, s.k, 12, MODE_RAW}, {ct, u2, s.ct, s.k, s.du, MODE_MAP},
                     {ct + 32 * (size_t)s.du * k, v2, s.ct, 1, s.dv, MODE_MAP}};
  PSF_TRY(launch_segs(false, count, in, 4, st));
  PSF_TRY(psf_ntt_image_from_fips203_dev(device, polys * k + 2 * polys, fips, 16, hat, st));
  PSF_TRY(psf_matpoly_mul_add_hat_dev(device, kQ, kN, count, 1, k, 1, s_hat, k * kN, 1, u2, v2, -1, wv, 16, st));     // w = v - s^T u
  const Seg msg[1] = {{mp, wv, 32, 1, 1, MODE_MAP}};                                                                   // m' = ByteEncode_1(Compress_1(w))
  PSF_TRY(launch_segs(true, count, msg, 1, st));
  const GArgs g{count, mp, 32, dk + 768 * k + 32, s.dk, 32, 0, 64, kp, 32, rp, 32};                                    // (K', r') = G(m' || h)
  hipLaunchKernelGGL(k_g, dim3(blocks_of(count, 256)), dim3(256), 0, st, g);
  HIP_TRY(hipGetLastError());
  const EncryptBufs eb{rp, mp, hat, t_hat, words_at(ws, w.y), words_at(ws, w.e1), words_at(ws, w.e2), words_at(ws, w.u), words_at(ws, w.v), cp, s.ct};
  PSF_TRY(encrypt(device, s, count, eb, st));
  const TailArgs ta{count, s.ct, s.dk, s.k, dk, ct, cp, kp, ss};
  hipLaunchKernelGGL(k_decaps_tail, dim3(blocks_of(count, 64)), dim3(256), 0, st, ta);        // 64 instances per workgroup
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

// ---- argument checks of the three operations, for both forms ---------------------------------------------------------------------------------------
// the header's order after `param` and count = 0: NULL pointers, byte counts, the workspace (device forms), overlaps; then the instance limit: every grid of
// this unit has at most one workgroup per instance (k_check_ek: exactly one; k_pack / k_unpack: 128 k threads per instance)
psf_status keygen_check(int param, size_t count, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk, bool dev, const void* ws, size_t ws_bytes, Set* s,
                        KeygenWs* w) {
  if (!set_of(param, s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  Buf b[4] = {buf_of(d, 32, false), buf_of(z, 32, false), buf_of(ek, s->ek, true), buf_of(dk, s->dk, true)};
  *w = keygen_ws(*s, count);
  PSF_TRY(check_null(b, 4));
  PSF_TRY(check_rest(count, b, 4, *w, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}
psf_status encaps_check(int param, size_t count, const uint8_t* ek, const uint8_t* m, uint8_t* ss, uint8_t* ct, bool dev, const void* ws, size_t ws_bytes, Set* s,
                        EncapsWs* w) {
  if (!set_of(param, s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  Buf b[4] = {buf_of(ek, s->ek, false), buf_of(m, 32, false), buf_of(ss, 32, true), buf_of(ct, s->ct, true)};
  *w = encaps_ws(*s, count);
  PSF_TRY(check_null(b, 4));
  PSF_TRY(check_rest(count, b, 4, *w, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}
psf_status decaps_check(int param, size_t count, const uint8_t* dk, const uint8_t* ct, uint8_t* ss, bool dev, const void* ws, size_t ws_bytes, Set* s, DecapsWs* w) {
  if (!set_of(param, s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  Buf b[3] = {buf_of(dk, s->dk, false), buf_of(ct, s->ct, false), buf_of(ss, 32, true)};
  *w = decaps_ws(*s, count);
  PSF_TRY(check_null(b, 3));
  PSF_TRY(check_rest(count, b, 3, *w, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

psf_status check_run(bool dk_form, int device, const Set& s, size_t count, const uint8_t* in, uint8_t* ok, hipStream_t st) {
  if (!grid_fits(count)) return PSF_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(device));
  if (dk_form) hipLaunchKernelGGL(k_check_dk, dim3(blocks_of(count, 256)), dim3(256), 0, st, in, s.dk, s.k, count, ok);
  else hipLaunchKernelGGL(k_check_ek, dim3((unsigned)count), dim3(256), 0, st, in, s.ek, s.k, ok);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status check_call(bool dk_form, bool host, int device, int param, size_t count, const uint8_t* in, uint8_t* ok, hipStream_t st) {
  Set s;
  if (!set_of(param, &s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const size_t len = dk_form ? s.dk : s.ek;
  Buf b[2] = {buf_of(in, len, false), buf_of(ok, 1, true)};
  PSF_TRY(check_null(b, 2));
  PSF_TRY(check_rest(count, b, 2, Layout{}, false, nullptr, 0));
  if (!host) return check_run(dk_form, device, s, count, in, ok, st);
  PSF_TRY(use_device(device));
  HostCall h;
  const uint8_t* din = h.in(in, count, len, len, dk_form ? SECRET : PUBLIC);
  uint8_t* dok = h.out(count);
  PSF_TRY(h.status());
  PSF_TRY(check_run(dk_form, device, s, count, din, dok, nullptr));
  return h.fetch(ok, dok, count);
}

}  // namespace mlkem
}  // namespace psf

using namespace psf;
using namespace psf::mlkem;

extern "C" {

psf_status psf_mlkem_sizes(int param, size_t* ek, size_t* dk, size_t* ct, size_t* ss) {
  Set s;
  if (!set_of(param, &s)) return PSF_ERR_PARAM;
  if (ek) *ek = s.ek;
  if (dk) *dk = s.dk;
  if (ct) *ct = s.ct;
  if (ss) *ss = 32;
  return PSF_OK;
}

psf_status psf_mlkem_workspace_bytes(int param, size_t count, int op, size_t* bytes) {
  Set s;
  if (!set_of(param, &s) || op < PSF_MLKEM_OP_KEYGEN || op > PSF_MLKEM_OP_CHECK || !bytes) return PSF_ERR_PARAM;
  const Layout need = ws_need(s, count, op);
  if (!need.ok) return PSF_ERR_PARAM;
  *bytes = need.total;
  return PSF_OK;
}

psf_status psf_mlkem_keygen_dev(int device, int param, size_t count, const uint8_t* d_d, const uint8_t* d_z, uint8_t* d_ek, uint8_t* d_dk, void* d_ws, size_t ws_bytes,
                                int* d_fail, void* stream) {
  Set s;
  KeygenWs w;
  const psf_status rc = keygen_check(param, count, d_d, d_z, d_ek, d_dk, true, d_ws, ws_bytes, &s, &w);
  if (rc != PSF_OK || count == 0) return rc;
  return keygen_run(device, s, count, d_d, d_z, d_ek, d_dk, d_ws, w, d_fail, (hipStream_t)stream);
}

psf_status psf_mlkem_encaps_dev(int device, int param, size_t count, const uint8_t* d_ek, const uint8_t* d_m, uint8_t* d_ss, uint8_t* d_ct, void* d_ws, size_t ws_bytes,
                                int* d_fail, void* stream) {
  Set s;
  EncapsWs w;
  const psf_status rc = encaps_check(param, count, d_ek, d_m, d_ss, d_ct, true, d_ws, ws_bytes, &s, &w);
  if (rc != PSF_OK || count == 0) return rc;
  return encaps_run(device, s, count, d_ek, d_m, d_ss, d_ct, d_ws, w, d_fail, (hipStream_t)stream);
}

psf_status psf_mlkem_decaps_dev(int device, int param, size_t count, const uint8_t* d_dk, const uint8_t* d_ct, uint8_t* d_ss, void* d_ws, size_t ws_bytes, int* d_fail,
                                void* stream) {
  Set s;
  DecapsWs w;
  const psf_status rc = decaps_check(param, count, d_dk, d_ct, d_ss, true, d_ws, ws_bytes, &s, &w);
  if (rc != PSF_OK || count == 0) return rc;
  return decaps_run(device, s, count, d_dk, d_ct, d_ss, d_ws, w, d_fail, (hipStream_t)stream);
}

psf_status psf_mlkem_check_ek_dev(int device, int param, size_t count, const uint8_t* d_ek, uint8_t* d_ok, void* stream) {
  return check_call(false, false, device, param, count, d_ek, d_ok, (hipStream_t)stream);
}
psf_status psf_mlkem_check_dk_dev(int device, int param, size_t count, const uint8_t* d_dk, uint8_t* d_ok, void* stream) {
  return check_call(true, false, device, param, count, d_dk, d_ok, (hipStream_t)stream);
}
psf_status psf_mlkem_check_ek(int device, int param, size_t count, const uint8_t* ek, uint8_t* ok) {
  return check_call(false, true, device, param, count, ek, ok, nullptr);
}
psf_status psf_mlkem_check_dk(int device, int param, size_t count, const uint8_t* dk, uint8_t* ok) {
  return check_call(true, true, device, param, count, dk, ok, nullptr);
}

psf_status psf_mlkem_keygen(int device, int param, size_t count, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk) {
  Set s;
  KeygenWs w;
  const psf_status rc = keygen_check(param, count, d, z, ek, dk, false, nullptr, 0, &s, &w);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  HostCall h;
  const uint8_t *dd = h.in(d, count, 32, 32, SECRET), *dz = h.in(z, count, 32, 32, SECRET);
  uint8_t *dek = h.out(count * s.ek), *ddk = h.out(count * s.dk, SECRET);
  void* dws = h.workspace(w.total);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(keygen_run(device, s, count, dd, dz, dek, ddk, dws, w, dflag, nullptr));
  PSF_TRY(h.fetch(ek, dek, count * s.ek));
  PSF_TRY(h.fetch(dk, ddk, count * s.dk));
  return h.finish();
}

psf_status psf_mlkem_encaps(int device, int param, size_t count, const uint8_t* ek, const uint8_t* m, uint8_t* ss, uint8_t* ct) {
  Set s;
  EncapsWs w;
  const psf_status rc = encaps_check(param, count, ek, m, ss, ct, false, nullptr, 0, &s, &w);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  HostCall h;
  const uint8_t *dek = h.in(ek, count, s.ek, s.ek), *dm = h.in(m, count, 32, 32, SECRET);
  uint8_t *dss = h.out(count * 32, SECRET), *dct = h.out(count * s.ct);
  void* dws = h.workspace(w.total);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(encaps_run(device, s, count, dek, dm, dss, dct, dws, w, dflag, nullptr));
  PSF_TRY(h.fetch(ss, dss, count * 32));
  PSF_TRY(h.fetch(ct, dct, count * s.ct));
  return h.finish();
}

psf_status psf_mlkem_decaps(int device, int param, size_t count, const uint8_t* dk, const uint8_t* ct, uint8_t* ss) {
  Set s;
  DecapsWs w;
  const psf_status rc = decaps_check(param, count, dk, ct, ss, false, nullptr, 0, &s, &w);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  HostCall h;
  const uint8_t *ddk = h.in(dk, count, s.dk, s.dk, SECRET), *dct = h.in(ct, count, s.ct, s.ct);
  uint8_t* dss = h.out(count * 32, SECRET);
  void* dws = h.workspace(w.total);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(decaps_run(device, s, count, ddk, dct, dss, dws, w, dflag, nullptr));
  PSF_TRY(h.fetch(ss, dss, count * 32));
  return h.finish();
}

}  // extern "C"
