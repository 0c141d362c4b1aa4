// psf_mldsa.hip -- ML-DSA (FIPS 204, August 2024) on the device, batched: KeyGen_internal (Algorithm 6) and Verify_internal (Algorithm 8) for
// ML-DSA-44, -65 and -87, bytes in and bytes out, `count` instances per call, and the stages they are made of as entry points of their own.  The
// sponge is psf_keccak_core.hpp, the products are ntt_matmul_dev / ntt_matfma_dev at (8380417, 256); this unit adds FIPS 204's own part
// (psf_mldsa_core.hpp) and the glue:
//   k_rej_ntt      RejNTTPoly, one polynomial per lane: ExpandA straight into product images (the permutation of image_from in its put), or 64-bit
//                  words in FIPS 204's NTT-domain order for the public stage
//   k_rej_bounded  RejBoundedPoly, one polynomial per lane: ExpandS
//   k_ball         SampleInBall, one instance per lane, the polynomial as bytes in LDS
//   k_image_from   FIPS 204's NTT-domain order -> product images
//   k_seed         (rho, rho', K) = H(xi || k || l, 128)
//   k_tr           tr = H(pk, 64)
//   k_mu           mu = H(tr || M', 64)
//   k_hint         HintBitUnpack, one lane per instance, into a bit mask per polynomial
//   k_unpack       pkDecode / sigDecode fields -> 64-bit words (t1 2^d, z) and the norm check of z
//   k_pack         Power2Round and pkEncode / skEncode fields from 64-bit words
//   k_verify_tail  UseHint, w1Encode and SHAKE256(mu || w1) in one lane per instance, w1 never in memory; the comparison with c~; ok and why
// One lane per unit of work and one Keccak state per lane throughout.  Everything secret of KeyGen lives in the caller's workspace, which the last
// operation of the call clears; verification has no secret (DESIGN.md "ML-DSA").
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_keccak_core.hpp"
#include "psf_mldsa_api.hpp"
#include "psf_mldsa_core.hpp"
#include "psf_ntt_api.hpp"
#include "psf_ntt_core.hpp"

namespace psf {
namespace dsa {

using kc::kDomShake;

// ---- samplers ------------------------------------------------------------------------------------------------------------------------------------
// One polynomial per lane, 64 consecutive polynomials per wave, four waves per workgroup, each wave on its own.  A lane past the end of the batch
// repeats the last polynomial (the wave vote of the parse loop sees 64 live lanes) and writes nothing.
// RejBoundedPoly and SampleInBall have values in [-4, 4]: a lane parks its coefficients as bytes in its wave's part of LDS at [coefficient][lane], at a
// pitch of 68 bytes (17 words between rows: the write of a coefficient by 64 lanes and the read of 64 coefficients of one polynomial are both conflict
// free; 17 KiB per wave), then the wave writes the 64 polynomials out one after the other, word lane + 64 k by lane `lane`.
// RejNTTPoly has 23-bit values: 64 polynomials of them are 64 KiB, more than the 40 KiB a wave of a four-wave workgroup can have, so a lane stores every
// accepted coefficient straight to its word (the 1 KiB or 2 KiB of a polynomial fill up in L2); LDS holds the permutation of the image form only.
constexpr int kPitch8 = 68;

struct RejNttArgs { size_t total, seed_stride; uint32_t k, l; uint8_t word_of[256]; };

// IMG: the output is the product image of the polynomial (32-bit words, word_of[j] the place of FIPS 204 coefficient j); else 64-bit words in order
template <bool IMG> __global__ __launch_bounds__(256) void k_rej_ntt(RejNttArgs a, const uint8_t* __restrict__ seed, void* __restrict__ out, int* __restrict__ fail) {
  __shared__ uint8_t perm[256];
  if constexpr (IMG) {
    perm[threadIdx.x] = a.word_of[threadIdx.x];
    __syncthreads();
  }
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < a.total;
  const size_t p = live ? g : a.total - 1;
  kc::SeedReader rd;
  if (a.k == 0) rd = kc::SeedReader{seed + p * a.seed_stride, 34, 0};
  else {                                                                 // polynomial (c, r, s): rho_c || s || r
    const uint32_t kl = a.k * a.l;
    const size_t c = p / kl;
    const uint32_t e = (uint32_t)(p - c * kl), r = e / a.l, s = e - r * a.l;
    rd = kc::SeedReader{seed + c * a.seed_stride, 32, s | (r << 8)};
  }
  uint64_t st[25];
  zero_state(st);
  kc::absorb<kc::kRateShake128, kc::DevOps>(st, rd, 34, kDomShake);
  const bool f = rej_ntt_parse<kc::DevOps>(st, [&](uint32_t j, uint32_t v) {
    if (!live) return;
    if constexpr (IMG) static_cast<uint32_t*>(out)[p * 256 + perm[j]] = v;
    else static_cast<uint64_t*>(out)[p * 256 + j] = v;
  }, kMaxBlocks);
  if (f && fail) atomicOr(fail, 1);
}

// the 64 polynomials of a wave from bytes in LDS to 64-bit words
__device__ __forceinline__ void emit_bytes(const int8_t* lds, int64_t* __restrict__ out, size_t p0, size_t total, uint32_t lane) {
  const size_t left = p0 < total ? total - p0 : 0;
  const uint32_t np = left < 64 ? (uint32_t)left : 64u;
  for (uint32_t q = 0; q < np; ++q) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t j = lane + 64 * k;
      out[(p0 + q) * 256 + j] = (int64_t)lds[j * kPitch8 + q];
    }
  }
}

struct BoundedArgs { size_t total, seed_stride; uint32_t per_seed, first_nonce; };

template <int ETA> __global__ __launch_bounds__(256) void k_rej_bounded(BoundedArgs a, const uint8_t* __restrict__ seed, int64_t* __restrict__ out, int* __restrict__ fail) {
  __shared__ int8_t lds_all[4 * 256 * kPitch8];
  const uint32_t lane = threadIdx.x & 63;
  int8_t* lds = lds_all + (threadIdx.x >> 6) * (256 * kPitch8);
  const size_t p0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u);
  const size_t p = p0 + lane < a.total ? p0 + lane : a.total - 1;
  const size_t c = p / a.per_seed;
  const uint32_t t = (uint32_t)(p - c * a.per_seed);
  uint64_t st[25];
  zero_state(st);
  kc::absorb<kc::kRateShake256, kc::DevOps>(st, kc::SeedReader{seed + c * a.seed_stride, 64, a.first_nonce + t}, 66, kDomShake);
  const bool f = rej_bounded_parse<ETA, kc::DevOps>(st, [&](uint32_t j, int v) { lds[__umul24(j, kPitch8) + lane] = (int8_t)v; }, kMaxBlocks);
  if (f && fail) atomicOr(fail, 1);
  __syncthreads();
  emit_bytes(lds, out, p0, a.total, lane);
}

struct BallArgs { size_t total, len, stride; uint32_t tau; };

__global__ __launch_bounds__(256) void k_ball(BallArgs a, const uint8_t* __restrict__ ctilde, int64_t* __restrict__ out, int* __restrict__ fail) {
  __shared__ int8_t lds_all[4 * 256 * kPitch8];
  const uint32_t lane = threadIdx.x & 63;
  int8_t* lds = lds_all + (threadIdx.x >> 6) * (256 * kPitch8);
  const size_t p0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u);
  const size_t p = p0 + lane < a.total ? p0 + lane : a.total - 1;
  for (uint32_t j = 0; j < 256; ++j) lds[j * kPitch8 + lane] = 0;       // a lane reads and writes its own column only until the emit
  uint64_t st[25];
  zero_state(st);
  kc::absorb<kc::kRateShake256, kc::DevOps>(st, kc::PtrReader{ctilde + p * a.stride, false}, a.len, kDomShake);
  const bool f = sample_in_ball_parse<kc::DevOps>(
      st, a.tau, [&](uint32_t j) { return (int)lds[__umul24(j, kPitch8) + lane]; }, [&](uint32_t j, int v) { lds[__umul24(j, kPitch8) + lane] = (int8_t)v; },
      kMaxBlocks);
  if (f && fail) atomicOr(fail, 1);
  __syncthreads();
  emit_bytes(lds, out, p0, a.total, lane);
}

// ---- NTT images ----------------------------------------------------------------------------------------------------------------------------------
struct ImgArgs { uint8_t src[256]; };

__global__ __launch_bounds__(256) void k_image_from(ImgArgs m, const uint64_t* __restrict__ fhat, uint32_t* __restrict__ hat, size_t count) {
  const uint32_t w = threadIdx.x, src = m.src[w];
  for (size_t c = blockIdx.x; c < count; c += gridDim.x) hat[c * 256 + w] = (uint32_t)(fhat[c * 256 + src] % kQ);
}

// ---- hashes ----------------------------------------------------------------------------------------------------------------------------------------
// KeyGen: (rho, rho', K) = H(xi_c || k || l, 128): rho to pk_c and sk_c, K to sk_c + 32, rho' to the workspace
struct SeedArgs { size_t count, pk_len, sk_len; uint32_t k, l; const uint8_t* xi; uint8_t* pk; uint8_t* sk; uint8_t* rho_p; };
__global__ __launch_bounds__(256) void k_seed(SeedArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint64_t s[25];
  zero_state(s);
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, kc::SeedReader{a.xi + c * 32, 32, a.k | (a.l << 8)}, 34, kDomShake);
  put_words<0, 4>(s, a.pk + c * a.pk_len);
  put_words<0, 4>(s, a.sk + c * a.sk_len);
  put_words<4, 8>(s, a.rho_p + c * 64);
  put_words<12, 4>(s, a.sk + c * a.sk_len + 32);
}

// tr_c = H(pk_c, 64) to out + c out_pitch
struct TrArgs { size_t count, pk_len, pk_pitch, out_pitch; const uint8_t* pk; uint8_t* out; };
__global__ __launch_bounds__(256) void k_tr(TrArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint64_t s[25];
  zero_state(s);
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, kc::PtrReader{a.pk + c * a.pk_pitch, aligned8(a.pk, a.pk_pitch)}, a.pk_len, kDomShake);
  put_words<0, 8>(s, a.out + c * a.out_pitch);
}

// mu_c = H(tr || M'_c, 64); tr_pitch = 0: one key for all
struct MuArgs { size_t count, tr_pitch, msg_len, msg_pitch; const uint8_t* tr; const uint8_t* msg; uint8_t* mu; };
__global__ __launch_bounds__(256) void k_mu(MuArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint64_t s[25];
  zero_state(s);
  const CatReader rd{a.tr + c * a.tr_pitch, a.msg + c * a.msg_pitch, 64, a.msg_len, aligned8(a.msg, a.msg_pitch)};      // tr is in the workspace: aligned
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, rd, 64 + a.msg_len, kDomShake);
  put_words<0, 8>(s, a.mu + c * 64);
}

// ---- the hint --------------------------------------------------------------------------------------------------------------------------------------
// One lane per instance: the omega + k bytes at hint + c pitch into k masks of 256 bits at h + c 32 k; flags[c] = 0, or PSF_MLDSA_WHY_HINT
struct HintArgs { size_t count, pitch; uint32_t k, omega; const uint8_t* hint; uint8_t* h; uint32_t* flags; };
__global__ __launch_bounds__(256) void k_hint(HintArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* y = a.hint + c * a.pitch;
  uint8_t* h = a.h + c * 32 * a.k;
  for (uint32_t i = 0; i < 4 * a.k; ++i) reinterpret_cast<uint64_t*>(h)[i] = 0;
  const bool ok = hint_bit_unpack([&](uint32_t pos) { return (uint32_t)y[pos]; }, a.k, a.omega,
                                  [&](uint32_t i, uint32_t j) { h[32 * i + (j >> 3)] |= (uint8_t)(1u << (j & 7)); });
  a.flags[c] = ok ? 0u : (uint32_t)PSF_MLDSA_WHY_HINT;
}

// ---- the polynomial glue ---------------------------------------------------------------------------------------------------------------------------
struct SegArgs { Seg seg[4]; uint32_t* flags; int32_t bound; };

__global__ __launch_bounds__(256) void k_unpack(SegArgs a) {
  const Seg sg = a.seg[blockIdx.y];
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)sg.polys * 32;
  if (g >= sg.count * per) return;
  const size_t inst = g / per;
  const uint8_t* src = sg.bytes + inst * sg.pitch + (g - inst * per) * (size_t)sg.bits;
  uint32_t f[8];
  for_bits(sg.bits, [&](auto b) { unpack8<decltype(b)::value>(src, f); });
  int64_t v[8];
  bool big = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int32_t x = field_to_value(sg.top, f[j]);
    big |= (x < 0 ? -x : x) >= a.bound;
    v[j] = sg.map == MAP_T1_SHIFT ? (int64_t)x << kD : (int64_t)x;
  }
  v4u* dst = reinterpret_cast<v4u*>(sg.words + g * 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v4u r;
    r[0] = (uint32_t)v[2 * j]; r[1] = (uint32_t)((uint64_t)v[2 * j] >> 32); r[2] = (uint32_t)v[2 * j + 1]; r[3] = (uint32_t)((uint64_t)v[2 * j + 1] >> 32);
    dst[j] = r;
  }
  if (sg.map == MAP_NORM && big) atomicOr(a.flags + inst, (uint32_t)PSF_MLDSA_WHY_NORM);
}

__global__ __launch_bounds__(256) void k_pack(SegArgs a) {
  const Seg sg = a.seg[blockIdx.y];
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)sg.polys * 32;
  if (g >= sg.count * per) return;
  const size_t inst = g / per;
  uint8_t* dst = const_cast<uint8_t*>(sg.bytes) + inst * sg.pitch + (g - inst * per) * (size_t)sg.bits;
  const v4u* src = reinterpret_cast<const v4u*>(sg.words + g * 8);
  uint32_t f[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const v4u r = src[j];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t lo = r[2 * e];                                      // T1 / T0: a residue in [0, q); PLAIN: a small signed value
      int32_t x = (int32_t)lo;
      if (sg.map == MAP_T1 || sg.map == MAP_T0) {
        uint32_t r1;
        int32_t r0;
        power2round(lo, r1, r0);
        x = sg.map == MAP_T1 ? (int32_t)r1 : r0;
      }
      f[2 * j + e] = value_to_field(sg.top, x);
    }
  }
  for_bits(sg.bits, [&](auto b) { pack8<decltype(b)::value>(dst, f); });
}

// ---- the verification tail -------------------------------------------------------------------------------------------------------------------------
// W1Reader (psf_mldsa_api.hpp) feeds mu || w1Encode(UseHint(h, w')) to the sponge.
struct TailArgs {
  size_t count, sig_len, mu_pitch;
  uint32_t k, cb;
  const uint8_t* mu; const uint64_t* w; const uint8_t* h; const uint8_t* sig; const uint32_t* flags;
  uint8_t* ok; uint8_t* why;
};
template <uint32_t G2> __global__ __launch_bounds__(256) void k_verify_tail(TailArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint32_t why = a.flags[c];
  if (why & PSF_MLDSA_WHY_HINT) why |= PSF_MLDSA_WHY_HASH;              // no w1' from a malformed hint
  else {
    const size_t fields = (size_t)a.k * 256;
    const uint8_t* mu = a.mu + c * a.mu_pitch;
    const W1Reader<G2> rd{mu, (uintptr_t)mu % 8 == 0, a.w + c * fields, a.h + c * 32 * a.k, fields};
    uint64_t s[25];
    zero_state(s);
    kc::absorb<kc::kRateShake256, kc::DevOps>(s, rd, 64 + fields * W1Reader<G2>::BITS / 8, kDomShake);
    const kc::PtrReader ct{a.sig + c * a.sig_len, false};
    uint64_t d = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
      if (i < a.cb / 8) d |= s[i] ^ ct.le64(8 * i);
    if (d != 0) why |= PSF_MLDSA_WHY_HASH;
  }
  a.ok[c] = why == 0 ? 1 : 0;
  if (a.why) a.why[c] = (uint8_t)why;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
bool set_of(int param, Set* s) {
  switch (param) {
    case PSF_MLDSA_44: *s = {4, 4, 2, 39, 32, 80, 1 << 17, (int32_t)kGamma2Low, 78, 18, 0, 0, 0}; break;
    case PSF_MLDSA_65: *s = {6, 5, 4, 49, 48, 55, 1 << 19, (int32_t)kGamma2High, 196, 20, 0, 0, 0}; break;
    case PSF_MLDSA_87: *s = {8, 7, 2, 60, 64, 75, 1 << 19, (int32_t)kGamma2High, 120, 20, 0, 0, 0}; break;
    default: return false;
  }
  const size_t eb = s->eta == 2 ? 3 : 4;
  s->pk = 32 + 320 * (size_t)s->k;
  s->sk = 128 + 32 * ((size_t)(s->k + s->l) * eb + 13 * (size_t)s->k);
  s->sig = s->cb + 32 * (size_t)s->zbits * s->l + s->omega + s->k;
  return true;
}

const ImageMap& image_map() {
  static const ImageMap m = [] {
    using S = ntt::Sched<8>;
    ImageMap im;
    const NttPlan pl = make_ntt_plan(kQ, 256);
    const NttTables tb = make_ntt_tables(pl);
    if (!pl.ok || pl.L != 8 || pl.d != 1 || !tb.wave || tb.qb != 0) return im;
    auto powmod = [](uint64_t b, uint32_t e) {
      uint64_t r = 1;
      for (; e; e >>= 1, b = b * b % kQ)
        if (e & 1) r = r * b % kQ;
      return r;
    };
    uint64_t point[256];                                                  // Algorithm 41 leaves f(+-1753^BitRev8(128 + floor(i / 2))) at position i
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t m7 = 128 + (i >> 1), br = 0;
      for (uint32_t b = 0; b < 8; ++b)
        if (m7 & (1u << b)) br |= 1u << (7 - b);
      const uint64_t z = powmod(1753, br);
      point[i] = (i & 1) ? kQ - z : z;
    }
    bool seen[256] = {};
    for (uint32_t p = 0; p < 256; ++p) {                                  // position p of the plan's order: +-zetas[128 + floor(p / 2)]
      const uint64_t z = pl.zetas[128 + (p >> 1)] % kQ, pt = (p & 1) ? kQ - z : z;
      uint32_t i = 0;
      while (i < 256 && point[i] != pt) ++i;
      if (i == 256 || seen[i]) return im;
      seen[i] = true;
      const uint32_t word = (uint32_t)S::reg_of_nat((int)(p & 3)) * 64 + (p >> 2);
      im.word_of[i] = (uint8_t)word;
      im.fips_of[word] = (uint8_t)i;
    }
    im.ok = true;
    return im;
  }();
  return m;
}

// the workspaces: sections in a fixed order (Layout).  A polynomial of 64-bit words takes 2048 bytes, an image 1024 bytes.
struct KeygenWs : Layout { size_t rho_p, a_hat, s1, s2, t; };
struct VerifyWs : Layout { size_t tr, mu, flags, h, a_hat, z, t1, c, w; };
KeygenWs keygen_ws(const Set& s, size_t count) {
  KeygenWs w;
  const u128 c = count, k = s.k, el = s.l;
  w.rho_p = w.take(c * 64);
  w.a_hat = w.take(c * k * el * 1024);
  w.s1 = w.take(c * el * 2048);
  w.s2 = w.take(c * k * 2048);
  w.t = w.take(c * k * 2048);
  return w;
}
// sized for one key per instance; with one key for all, the sections of tr, the images and t1 are used for one instance only
VerifyWs verify_ws(const Set& s, size_t count) {
  VerifyWs w;
  const u128 c = count, k = s.k, el = s.l;
  w.tr = w.take(c * 64);
  w.mu = w.take(c * 64);
  w.flags = w.take(c * 4);
  w.h = w.take(c * k * 32);
  w.a_hat = w.take(c * k * el * 1024);
  w.z = w.take(c * el * 2048);
  w.t1 = w.take(c * k * 2048);
  w.c = w.take(c * 2048);
  w.w = w.take(c * k * 2048);
  return w;
}
Layout ws_need(const Set& s, size_t count, int op) {
  if (op == PSF_MLDSA_OP_KEYGEN) return keygen_ws(s, count);
  return verify_ws(s, count);
}

// ---- launches of the stages (arguments checked by the caller; `device` is current) ------------------------------------------------------------------
psf_status rej_ntt_launch(size_t total, uint32_t k, uint32_t l, const uint8_t* d_seed, size_t seed_stride, void* d_out, bool img, int* d_fail, hipStream_t st) {
  const size_t blocks = (total + 255) / 256;
  if (blocks > kMaxGrid) return PSF_ERR_UNSUPPORTED;
  RejNttArgs a{};
  a.total = total; a.seed_stride = seed_stride; a.k = k; a.l = l;
  if (img) {
    const ImageMap& m = image_map();
    if (!m.ok) return PSF_ERR_UNSUPPORTED;
    for (int i = 0; i < 256; ++i) a.word_of[i] = m.word_of[i];
    hipLaunchKernelGGL(k_rej_ntt<true>, dim3((unsigned)blocks), dim3(256), 0, st, a, d_seed, d_out, d_fail);
  } else {
    hipLaunchKernelGGL(k_rej_ntt<false>, dim3((unsigned)blocks), dim3(256), 0, st, a, d_seed, d_out, d_fail);
  }
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status rej_bounded_launch(size_t total, uint32_t eta, const uint8_t* d_seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed, int64_t* d_out,
                              int* d_fail, hipStream_t st) {
  const size_t blocks = (total + 255) / 256;
  if (blocks > kMaxGrid) return PSF_ERR_UNSUPPORTED;
  const BoundedArgs a{total, seed_stride, per_seed, first_nonce};
  if (eta == 2) hipLaunchKernelGGL(k_rej_bounded<2>, dim3((unsigned)blocks), dim3(256), 0, st, a, d_seed, d_out, d_fail);
  else hipLaunchKernelGGL(k_rej_bounded<4>, dim3((unsigned)blocks), dim3(256), 0, st, a, d_seed, d_out, d_fail);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status ball_launch(size_t total, uint32_t tau, const uint8_t* d_ct, size_t len, size_t stride, int64_t* d_out, int* d_fail, hipStream_t st) {
  const size_t blocks = (total + 255) / 256;
  if (blocks > kMaxGrid) return PSF_ERR_UNSUPPORTED;
  const BallArgs a{total, len, stride, tau};
  hipLaunchKernelGGL(k_ball, dim3((unsigned)blocks), dim3(256), 0, st, a, d_ct, d_out, d_fail);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status image_launch(int device, size_t count, const uint64_t* d_fhat, uint32_t* d_hat, hipStream_t st) {
  const ImageMap& m = image_map();
  if (!m.ok) return PSF_ERR_UNSUPPORTED;
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const unsigned blocks = (unsigned)(count < (size_t)cus * 8 ? count : (size_t)cus * 8);
  ImgArgs a;
  for (int i = 0; i < 256; ++i) a.src[i] = m.fips_of[i];
  hipLaunchKernelGGL(k_image_from, dim3(blocks), dim3(256), 0, st, a, d_fhat, d_hat, count);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status launch_segs(bool pack, const Seg* segs, int nseg, uint32_t* flags, int32_t bound, hipStream_t st) {
  SegArgs a{};
  size_t most = 0;
  for (int i = 0; i < nseg; ++i) {
    a.seg[i] = segs[i];
    const size_t items = segs[i].count * segs[i].polys * 32;
    most = items > most ? items : most;
  }
  a.flags = flags;
  a.bound = bound;
  const dim3 grid(blocks_of(most, 256), (unsigned)nseg);
  if (pack) hipLaunchKernelGGL(k_pack, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_unpack, grid, dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
// ---- the two algorithms ----------------------------------------------------------------------------------------------------------------------------
psf_status keygen_run(int device, const Set& s, size_t count, const uint8_t* xi, uint8_t* pk, uint8_t* sk, void* ws, const KeygenWs& w, int* fail, hipStream_t st) {
  const size_t k = s.k, l = s.l, eb = s.eta == 2 ? 3 : 4;
  uint8_t* rho_p = at<uint8_t>(ws, w.rho_p);
  uint32_t* a_hat = at<uint32_t>(ws, w.a_hat);
  int64_t *s1 = at<int64_t>(ws, w.s1), *s2 = at<int64_t>(ws, w.s2), *t = at<int64_t>(ws, w.t);
  PSF_TRY(use_device(device));
  const SeedArgs sa{count, s.pk, s.sk, s.k, s.l, xi, pk, sk, rho_p};
  hipLaunchKernelGGL(k_seed, dim3(blocks_of(count, 256)), dim3(256), 0, st, sa);
  HIP_TRY(hipGetLastError());
  PSF_TRY(rej_ntt_launch(count * k * l, s.k, s.l, pk, s.pk, a_hat, true, fail, st));                    // A_hat = ExpandA(rho), as images
  PSF_TRY(rej_bounded_launch(count * l, s.eta, rho_p, 64, 0, s.l, s1, fail, st));                       // (s1, s2) = ExpandS(rho')
  PSF_TRY(rej_bounded_launch(count * k, s.eta, rho_p, 64, s.l, s.k, s2, fail, st));
  const NttMatShape shape{count, k, l, 1, 0};
  PSF_TRY(ntt_matfma_dev(device, kQ, kN, shape, a_hat, k * l * kN, true, s1, s2, 1, t, 64, st));        // t = A s1 + s2
  const Packing pe = s.eta == 2 ? kPackEta2 : kPackEta4;
  const Seg segs[4] = {seg_of(pk + 32, t, s.pk, count, s.k, kPackT1, MAP_T1), seg_of(sk + 128 + 32 * eb * (k + l), t, s.sk, count, s.k, kPackT0, MAP_T0),
                       seg_of(sk + 128, s1, s.sk, count, s.l, pe, MAP_PLAIN), seg_of(sk + 128 + 32 * eb * l, s2, s.sk, count, s.k, pe, MAP_PLAIN)};
  PSF_TRY(launch_segs(true, segs, 4, nullptr, 0, st));
  const TrArgs ta{count, s.pk, s.pk, s.sk, pk, sk + 64};                                                  // tr = H(pk, 64), into sk
  hipLaunchKernelGGL(k_tr, dim3(blocks_of(count, 256)), dim3(256), 0, st, ta);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

struct VerifyIn { const uint8_t* pk; size_t pk_stride; const uint8_t* msg; size_t msg_len, msg_stride; int msg_kind; const uint8_t* sig; };
psf_status verify_run(int device, const Set& s, size_t count, const VerifyIn& in, uint8_t* ok, uint8_t* why, void* ws, const VerifyWs& w, int* fail, hipStream_t st) {
  const size_t k = s.k, l = s.l, keys = in.pk_stride ? count : 1;
  uint8_t *tr = at<uint8_t>(ws, w.tr), *mu = at<uint8_t>(ws, w.mu), *h = at<uint8_t>(ws, w.h);
  uint32_t *flags = at<uint32_t>(ws, w.flags), *a_hat = at<uint32_t>(ws, w.a_hat);
  int64_t *z = at<int64_t>(ws, w.z), *t1 = at<int64_t>(ws, w.t1), *c = at<int64_t>(ws, w.c), *wp = at<int64_t>(ws, w.w);
  PSF_TRY(use_device(device));
  PSF_TRY(rej_ntt_launch(keys * k * l, s.k, s.l, in.pk, in.pk_stride, a_hat, true, fail, st));
  const bool hashed = in.msg_kind == PSF_MLDSA_MSG_BYTES;
  if (hashed) {
    const TrArgs ta{keys, s.pk, in.pk_stride, 64, in.pk, tr};
    hipLaunchKernelGGL(k_tr, dim3(blocks_of(keys, 256)), dim3(256), 0, st, ta);
    HIP_TRY(hipGetLastError());
    const MuArgs ma{count, in.pk_stride ? (size_t)64 : 0, in.msg_len, in.msg_stride, tr, in.msg, mu};
    hipLaunchKernelGGL(k_mu, dim3(blocks_of(count, 256)), dim3(256), 0, st, ma);
    HIP_TRY(hipGetLastError());
  }
  PSF_TRY(ball_launch(count, s.tau, in.sig, s.cb, s.sig, c, fail, st));                                  // c = SampleInBall(c~)
  const HintArgs ha{count, s.sig, s.k, s.omega, in.sig + s.cb + 32 * (size_t)s.zbits * l, h, flags};
  hipLaunchKernelGGL(k_hint, dim3(blocks_of(count, 256)), dim3(256), 0, st, ha);                         // writes every flag: before the norm check
  HIP_TRY(hipGetLastError());
  const Seg segs[2] = {seg_of(in.sig + s.cb, z, s.sig, count, s.l, s.zbits == 18 ? kPackZ17 : kPackZ19, MAP_NORM),
                       seg_of(in.pk + 32, t1, in.pk_stride, keys, s.k, kPackT1, MAP_T1_SHIFT)};
  PSF_TRY(launch_segs(false, segs, 2, flags, s.gamma1 - s.beta, st));
  const NttMatShape az{count, k, l, 1, 0}, ct{count, k, 1, 1, 0};
  PSF_TRY(ntt_matmul_dev(device, kQ, kN, az, a_hat, in.pk_stride ? k * l * kN : 0, true, z, wp, 64, st));              // w = A z
  PSF_TRY(ntt_matfma_dev(device, kQ, kN, ct, t1, in.pk_stride ? k : 0, false, c, wp, -1, wp, 64, st));                // w' = w - (t1 2^d) c
  const TailArgs ta{count, s.sig, hashed ? (size_t)64 : in.msg_stride, s.k, s.cb, hashed ? mu : in.msg, reinterpret_cast<const uint64_t*>(wp), h, in.sig, flags, ok, why};
  if (s.gamma2 == (int32_t)kGamma2Low) hipLaunchKernelGGL(k_verify_tail<kGamma2Low>, dim3(blocks_of(count, 256)), dim3(256), 0, st, ta);
  else hipLaunchKernelGGL(k_verify_tail<kGamma2High>, dim3(blocks_of(count, 256)), dim3(256), 0, st, ta);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// ---- argument checks of the entry points -----------------------------------------------------------------------------------------------------------
struct Checked { Set s; Layout need; };
psf_status keygen_check(int param, size_t count, const uint8_t* xi, uint8_t* pk, uint8_t* sk, bool dev, const void* ws, size_t ws_bytes, Checked* kc_) {
  if (!set_of(param, &kc_->s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  Buf b[3] = {{xi, 32, 32, false, false, 0}, {pk, kc_->s.pk, kc_->s.pk, true, false, 0}, {sk, kc_->s.sk, kc_->s.sk, true, false, 0}};
  PSF_TRY(check_null(b, 3));
  kc_->need = ws_need(kc_->s, count, PSF_MLDSA_OP_KEYGEN);
  PSF_TRY(check_rest(count, b, 3, kc_->need, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}
psf_status verify_check(int param, size_t count, const VerifyIn& in, uint8_t* ok, uint8_t* why, bool dev, const void* ws, size_t ws_bytes, Checked* kc_) {
  if (!set_of(param, &kc_->s) || (in.msg_kind != PSF_MLDSA_MSG_BYTES && in.msg_kind != PSF_MLDSA_MSG_MU)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const Set& s = kc_->s;
  Buf b[5] = {{in.pk, s.pk, in.pk_stride, false, false, 0}, {in.msg, in.msg_len, in.msg_stride, false, in.msg_len == 0, 0}, {in.sig, s.sig, s.sig, false, false, 0},
              {ok, 1, 1, true, false, 0}, {why, 1, 1, true, true, 0}};
  PSF_TRY(check_null(b, 5));
  if ((in.pk_stride != 0 && in.pk_stride < s.pk) || in.msg_stride < in.msg_len) return PSF_ERR_PARAM;
  if (in.msg_kind == PSF_MLDSA_MSG_MU && in.msg_len != 64) return PSF_ERR_PARAM;
  if (in.msg_len > SIZE_MAX - 64) return PSF_ERR_PARAM;
  kc_->need = ws_need(s, count, PSF_MLDSA_OP_VERIFY);
  PSF_TRY(check_rest(count, b, 5, kc_->need, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

// the checks every stage shares: pointers, strides, sizes, overlap of the seeds with the output
psf_status stage_check(size_t count, const void* seed, size_t seed_len, size_t seed_stride, const void* out, size_t polys_per_seed, size_t word_bytes, size_t* total) {
  if (seed_stride < seed_len) return PSF_ERR_PARAM;
  if (count && (!out || (!seed && seed_len))) return PSF_ERR_PARAM;
  const size_t poly = (size_t)kN * word_bytes;
  if (polys_per_seed && count > SIZE_MAX / polys_per_seed / poly) return PSF_ERR_PARAM;
  *total = count * polys_per_seed;
  size_t in_span = 0, out_span = 0;
  if (!span_of(seed, count, seed_len, seed_stride, &in_span) || !span_of(out, *total, poly, poly, &out_span)) return PSF_ERR_PARAM;
  if (overlap(seed, in_span, out, out_span)) return PSF_ERR_PARAM;
  return PSF_OK;
}
psf_status check_sample_ntt(size_t count, uint32_t k, uint32_t l, const uint8_t* seed, size_t seed_stride, const void* out, size_t* total) {
  if (k > 255 || l > 255 || (k == 0) != (l == 0)) return PSF_ERR_PARAM;
  return stage_check(count, seed, k ? 32 : 34, seed_stride, out, k ? (size_t)k * l : 1, 8, total);
}
psf_status check_sample_bounded(size_t count, uint32_t eta, const uint8_t* seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed, const void* out,
                                size_t* total) {
  if (eta == 0) return PSF_ERR_PARAM;
  if (first_nonce > 65536 || per_seed > 65536 - first_nonce) return PSF_ERR_PARAM;
  PSF_TRY(stage_check(count, seed, 64, seed_stride, out, per_seed, 8, total));
  return eta == 2 || eta == 4 ? PSF_OK : PSF_ERR_UNSUPPORTED;
}
psf_status check_sample_in_ball(size_t count, uint32_t tau, const uint8_t* ct, size_t len, size_t stride, const void* out, size_t* total) {
  if (tau < 1 || tau > 64) return PSF_ERR_PARAM;
  return stage_check(count, ct, len, stride, out, 1, 8, total);
}
psf_status check_image(size_t count, const uint64_t* fhat, const uint32_t* hat) {
  if (count && (!fhat || !hat)) return PSF_ERR_PARAM;
  if (count > SIZE_MAX / (kN * 8)) return PSF_ERR_PARAM;
  if (overlap(fhat, count * kN * 8, hat, count * kN * 4)) return PSF_ERR_PARAM;
  return image_map().ok ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

// a stage on host buffers: packed device copies of the seeds, the output, the flag
template <class Launch> psf_status stage_host(int device, size_t count, const void* seed, size_t seed_len, size_t seed_stride, void* out, size_t out_bytes, Launch&& launch) {
  PSF_TRY(use_device(device));
  HostCall h;
  const uint8_t* dseed = h.in(seed, count, seed_len, seed_stride);                  // stage_check: seed_stride >= seed_len
  uint8_t* dout = h.out(out_bytes);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(launch(dseed, dout, dflag));
  PSF_TRY(h.fetch(out, dout, out_bytes));
  return h.finish();
}

}  // namespace dsa
}  // namespace psf

using namespace psf;
using namespace psf::dsa;

extern "C" {

psf_status psf_mldsa_sizes(int param, size_t* pk, size_t* sk, size_t* sig) {
  Set s;
  if (!set_of(param, &s)) return PSF_ERR_PARAM;
  if (pk) *pk = s.pk;
  if (sk) *sk = s.sk;
  if (sig) *sig = s.sig;
  return PSF_OK;
}

psf_status psf_mldsa_workspace_bytes(int param, size_t count, int op, size_t* bytes) {
  Set s;
  if (!set_of(param, &s) || (op != PSF_MLDSA_OP_KEYGEN && op != PSF_MLDSA_OP_VERIFY) || !bytes) return PSF_ERR_PARAM;
  const Layout need = ws_need(s, count, op);
  if (!need.ok) return PSF_ERR_PARAM;
  *bytes = need.total;
  return PSF_OK;
}

psf_status psf_mldsa_keygen_dev(int device, int param, size_t count, const uint8_t* d_xi, uint8_t* d_pk, uint8_t* d_sk, void* d_ws, size_t ws_bytes, int* d_fail,
                                void* stream) {
  Checked kc_{};
  const psf_status rc = keygen_check(param, count, d_xi, d_pk, d_sk, true, d_ws, ws_bytes, &kc_);
  if (rc != PSF_OK || count == 0) return rc;
  return keygen_run(device, kc_.s, count, d_xi, d_pk, d_sk, d_ws, keygen_ws(kc_.s, count), d_fail, (hipStream_t)stream);
}

psf_status psf_mldsa_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                                int msg_kind, const uint8_t* d_sig, uint8_t* d_ok, uint8_t* d_why, void* d_ws, size_t ws_bytes, int* d_fail, void* stream) {
  Checked kc_{};
  const VerifyIn in{d_pk, pk_stride, d_msg, msg_len, msg_stride, msg_kind, d_sig};
  const psf_status rc = verify_check(param, count, in, d_ok, d_why, true, d_ws, ws_bytes, &kc_);
  if (rc != PSF_OK || count == 0) return rc;
  return verify_run(device, kc_.s, count, in, d_ok, d_why, d_ws, verify_ws(kc_.s, count), d_fail, (hipStream_t)stream);
}

psf_status psf_mldsa_keygen(int device, int param, size_t count, const uint8_t* xi, uint8_t* pk, uint8_t* sk) {
  Checked kc_{};
  const psf_status rc = keygen_check(param, count, xi, pk, sk, false, nullptr, 0, &kc_);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  const Set& s = kc_.s;
  HostCall h;
  const uint8_t* dxi = h.in(xi, count, 32, 32, SECRET);
  uint8_t *dpk = h.out(count * s.pk), *dsk = h.out(count * s.sk, SECRET);
  void* dws = h.workspace(kc_.need.total);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(keygen_run(device, s, count, dxi, dpk, dsk, dws, keygen_ws(s, count), dflag, nullptr));
  PSF_TRY(h.fetch(pk, dpk, count * s.pk));
  PSF_TRY(h.fetch(sk, dsk, count * s.sk));
  return h.finish();
}

psf_status psf_mldsa_verify(int device, int param, size_t count, const uint8_t* pk, size_t pk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                            int msg_kind, const uint8_t* sig, uint8_t* ok, uint8_t* why) {
  Checked kc_{};
  const VerifyIn in{pk, pk_stride, msg, msg_len, msg_stride, msg_kind, sig};
  const psf_status rc = verify_check(param, count, in, ok, why, false, nullptr, 0, &kc_);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  const Set& s = kc_.s;
  HostCall h;
  const VerifyIn din{h.in(pk, count, s.pk, pk_stride), pk_stride ? s.pk : 0, h.in(msg, count, msg_len, msg_stride), msg_len, msg_len, msg_kind, h.in(sig, count, s.sig, s.sig)};
  uint8_t *dok = h.out(count), *dwhy = h.out(count);
  void* dws = h.workspace(kc_.need.total);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(verify_run(device, s, count, din, dok, dwhy, dws, verify_ws(s, count), dflag, nullptr));
  PSF_TRY(h.fetch(ok, dok, count));
  PSF_TRY(h.fetch(why, dwhy, count));
  return h.finish();
}

// ---- the stages ------------------------------------------------------------------------------------------------------------------------------------
psf_status psf_sample_ntt_fips204_dev(int device, size_t count, uint32_t k, uint32_t l, const uint8_t* d_seed, size_t seed_stride, uint64_t* d_out, int* d_fail,
                                      void* stream) {
  size_t total = 0;
  const psf_status rc = check_sample_ntt(count, k, l, d_seed, seed_stride, d_out, &total);
  if (rc != PSF_OK || total == 0) return rc;
  PSF_TRY(use_device(device));
  return rej_ntt_launch(total, k, l, d_seed, seed_stride, d_out, false, d_fail, (hipStream_t)stream);
}
psf_status psf_sample_ntt_fips204(int device, size_t count, uint32_t k, uint32_t l, const uint8_t* seed, size_t seed_stride, uint64_t* out) {
  size_t total = 0;
  const psf_status rc = check_sample_ntt(count, k, l, seed, seed_stride, out, &total);
  if (rc != PSF_OK || total == 0) return rc;
  const size_t len = k ? 32 : 34;
  return stage_host(device, count, seed, len, seed_stride, out, total * kN * 8,
                    [&](const uint8_t* ds, void* dout, int* df) { return rej_ntt_launch(total, k, l, ds, len, dout, false, df, nullptr); });
}

psf_status psf_sample_bounded_fips204_dev(int device, size_t count, uint32_t eta, const uint8_t* d_seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed,
                                          int64_t* d_out, int* d_fail, void* stream) {
  size_t total = 0;
  const psf_status rc = check_sample_bounded(count, eta, d_seed, seed_stride, first_nonce, per_seed, d_out, &total);
  if (rc != PSF_OK || total == 0) return rc;
  PSF_TRY(use_device(device));
  return rej_bounded_launch(total, eta, d_seed, seed_stride, first_nonce, per_seed, d_out, d_fail, (hipStream_t)stream);
}
psf_status psf_sample_bounded_fips204(int device, size_t count, uint32_t eta, const uint8_t* seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed,
                                      int64_t* out) {
  size_t total = 0;
  const psf_status rc = check_sample_bounded(count, eta, seed, seed_stride, first_nonce, per_seed, out, &total);
  if (rc != PSF_OK || total == 0) return rc;
  return stage_host(device, count, seed, 64, seed_stride, out, total * kN * 8, [&](const uint8_t* ds, void* dout, int* df) {
    return rej_bounded_launch(total, eta, ds, 64, first_nonce, per_seed, static_cast<int64_t*>(dout), df, nullptr);
  });
}

psf_status psf_sample_in_ball_fips204_dev(int device, size_t count, uint32_t tau, const uint8_t* d_ctilde, size_t ctilde_len, size_t ctilde_stride, int64_t* d_out,
                                          int* d_fail, void* stream) {
  size_t total = 0;
  const psf_status rc = check_sample_in_ball(count, tau, d_ctilde, ctilde_len, ctilde_stride, d_out, &total);
  if (rc != PSF_OK || total == 0) return rc;
  PSF_TRY(use_device(device));
  return ball_launch(total, tau, d_ctilde, ctilde_len, ctilde_stride, d_out, d_fail, (hipStream_t)stream);
}
psf_status psf_sample_in_ball_fips204(int device, size_t count, uint32_t tau, const uint8_t* ctilde, size_t ctilde_len, size_t ctilde_stride, int64_t* out) {
  size_t total = 0;
  const psf_status rc = check_sample_in_ball(count, tau, ctilde, ctilde_len, ctilde_stride, out, &total);
  if (rc != PSF_OK || total == 0) return rc;
  return stage_host(device, count, ctilde, ctilde_len, ctilde_stride, out, total * kN * 8, [&](const uint8_t* ds, void* dout, int* df) {
    return ball_launch(total, tau, ds, ctilde_len, ctilde_len, static_cast<int64_t*>(dout), df, nullptr);
  });
}

psf_status psf_ntt_image_from_fips204_dev(int device, size_t count, const uint64_t* d_fhat, uint32_t* d_hat, void* stream) {
  const psf_status rc = check_image(count, d_fhat, d_hat);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  return image_launch(device, count, d_fhat, d_hat, (hipStream_t)stream);
}
psf_status psf_ntt_image_from_fips204(int device, size_t count, const uint64_t* fhat, uint32_t* hat) {
  const psf_status rc = check_image(count, fhat, hat);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  DevBuf df, dh;
  HIP_TRY(df.alloc(count * kN * 8));
  HIP_TRY(dh.alloc(count * kN * 4));
  HIP_TRY(df.upload(fhat, count * kN * 8));
  PSF_TRY(image_launch(device, count, df.as<uint64_t>(), dh.as<uint32_t>(), nullptr));
  HIP_TRY(dh.download(hat, count * kN * 4));
  return PSF_OK;
}

}  // extern "C"
