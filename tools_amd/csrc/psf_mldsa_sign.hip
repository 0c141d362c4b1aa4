// psf_mldsa_sign.hip -- ML-DSA.Sign_internal (FIPS 204 Algorithm 7) on the device, batched, for ML-DSA-44, -65 and -87: begin / round / end over a
// dense prefix of live slots (include/psf_mi355x.h, DESIGN.md "ML-DSA signing").  A slot holds what one unsigned instance needs for its next attempt
// (mu, rho'', kappa, its index, and with one key per instance the images of A_hat, s1_hat, s2_hat and t0_hat); a round makes one attempt for the
// first min(active, *d_live) slots, writes the signatures of the accepted ones, and moves live slots from beyond the new prefix into its holes.
// The sponge, ExpandA, SampleInBall and the products are those of KeyGen / Verify (psf_mldsa_api.hpp, psf_ntt_api.hpp); this unit adds
//   k_sign_unpack   s1, s2, t0 of skDecode as residues in [0, q), a thread per 8 coefficients
//   k_sign_seed     mu = H(tr || M', 64) (or mu given) and rho'' = H(K || rnd || mu, 64), one instance per lane; kappa = 0, index = c, *d_live = count
//   k_expand_mask   ExpandMask, one polynomial per lane: SHAKE256(rho'' || le16(kappa + r)) squeezed over five blocks straight into y
//   k_sign_ctilde   c~ = H(mu || w1Encode(HighBits(w)), lambda / 4), one slot per lane, w1 never in memory
//   k_sign_check    the four tests of Algorithm 7 and MakeHint over all coefficients of a slot by one workgroup; then, on the accept bit alone,
//                   sigEncode of the accepted instance
//   k_sign_match    pairs the holes of the new prefix with the live slots beyond it
//   k_sign_move     copies the state of each such slot into its hole
//   k_sign_commit   *d_live = new_live
// No kernel here branches or addresses on s1, s2, t0, y or a value of a rejected attempt; the accept bit of a whole attempt is the one exception.
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_keccak_core.hpp"
#include "psf_mldsa_api.hpp"
#include "psf_mldsa_core.hpp"
#include "psf_ntt_api.hpp"

namespace psf {
namespace dsa {

using kc::kDomShake;

// ctl words of the workspace: slots that left the live set in this round, holes and sources matched so far
enum { CTL_DONE = 0, CTL_HOLES = 1, CTL_SRCS = 2, CTL_WORDS = 4 };

__device__ __forceinline__ size_t live_prefix(size_t active, const uint32_t* live) {
  const size_t lv = *live;
  return active < lv ? active : lv;
}

// ---- begin -----------------------------------------------------------------------------------------------------------------------------------------
// out: the s1 of every key (keys * l polynomials), then every s2, then every t0, as 64-bit residues for ntt_forward_dev
struct SkArgs { size_t keys, sk_stride; uint32_t k, l, eta; const uint8_t* sk; uint64_t* out; };
__global__ __launch_bounds__(256) void k_sign_unpack(SkArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)(a.l + 2 * a.k) * 32;
  if (g >= a.keys * per) return;
  const size_t key = g / per;
  const uint32_t e = (uint32_t)(g - key * per), poly = e >> 5, t = e & 31, ebits = a.eta == 2 ? 3 : 4;
  const uint8_t* sk = a.sk + key * a.sk_stride + 128;
  uint32_t f[8];
  int32_t top;
  size_t o;
  if (poly < a.l + a.k) {
    const uint8_t* src = sk + (size_t)poly * 32 * ebits + t * ebits;
    if (ebits == 3) unpack8<3>(src, f);
    else unpack8<4>(src, f);
    top = (int32_t)a.eta;
    o = poly < a.l ? key * a.l + poly : a.keys * a.l + key * a.k + (poly - a.l);
  } else {
    const uint32_t r = poly - a.l - a.k;
    unpack8<13>(sk + (size_t)(a.l + a.k) * 32 * ebits + (size_t)r * 416 + t * 13, f);
    top = 1 << (kD - 1);
    o = a.keys * (a.l + a.k) + key * a.k + r;
  }
  v4u* dst = reinterpret_cast<v4u*>(a.out + o * 256 + t * 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v4u r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int32_t x = field_to_value(top, f[2 * j + h]);
      r[2 * h] = (uint32_t)(x + (int32_t)(kQ & (uint32_t)(x >> 31)));      // x < 0: x + q
      r[2 * h + 1] = 0;
    }
    dst[j] = r;
  }
}

// K (32 bytes), rnd (32 bytes, or zeros), mu (8 words in registers)
struct KRndMuReader {
  const uint8_t* key;
  const uint8_t* rnd;
  const uint64_t (&mu)[8];
  PSF_KC_FN uint8_t byte(size_t pos) const {
    if (pos < 32) return key[pos];
    if (pos < 64) return rnd ? rnd[pos - 32] : (uint8_t)0;
    return (uint8_t)(mu[(pos - 64) >> 3] >> (8 * (pos & 7)));
  }
  PSF_KC_FN uint64_t le64(size_t pos) const {
    if (pos >= 64) return mu[(pos - 64) >> 3];
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte(pos + k) << (8 * k);
    return w;
  }
};

struct SeedArgs {
  size_t count, sk_stride, msg_len, msg_stride;
  int msg_kind;
  const uint8_t* sk; const uint8_t* msg; const uint8_t* rnd;
  uint64_t* mu; uint64_t* rho; uint32_t* kappa; uint32_t* index; uint32_t* ctl; uint32_t* live;
};
__global__ __launch_bounds__(256) void k_sign_seed(SeedArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c == 0) {
    *a.live = (uint32_t)a.count;
    for (int i = 0; i < CTL_WORDS; ++i) a.ctl[i] = 0;
  }
  if (c >= a.count) return;
  const uint8_t* sk = a.sk + c * a.sk_stride;
  const uint8_t* msg = a.msg + c * a.msg_stride;
  uint64_t m[8], s[25];
  if (a.msg_kind == PSF_MLDSA_MSG_MU) {
    const kc::PtrReader rd{msg, aligned8(a.msg, a.msg_stride)};
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = rd.le64(8 * i);
  } else {
    zero_state(s);
    const CatReader rd{sk + 64, msg, 64, a.msg_len, aligned8(a.sk, a.sk_stride) && aligned8(a.msg, a.msg_stride)};
    kc::absorb<kc::kRateShake256, kc::DevOps>(s, rd, 64 + a.msg_len, kDomShake);
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = s[i];
  }
  zero_state(s);
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, KRndMuReader{sk + 32, a.rnd ? a.rnd + c * 32 : nullptr, m}, 128, kDomShake);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a.mu[c * 8 + i] = m[i];
    a.rho[c * 8 + i] = s[i];
  }
  a.kappa[c] = 0;
  a.index[c] = (uint32_t)c;
}

// ---- a round ---------------------------------------------------------------------------------------------------------------------------------------
// polynomial r of slot j: lane j l + r.  y[(j l + r) 256 + i] = gamma1 - field i of the stream
struct MaskArgs { size_t active; uint32_t l; const uint32_t* live; const uint8_t* rho; const uint32_t* kappa; int64_t* y; };
template <int BITS> __global__ __launch_bounds__(256) void k_expand_mask(MaskArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= live_prefix(a.active, a.live) * a.l) return;
  const size_t slot = g / a.l;
  const uint32_t r = (uint32_t)(g - slot * a.l);
  uint64_t s[25];
  zero_state(s);
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, kc::SeedReader{a.rho + slot * 64, 64, a.kappa[slot] + r}, 66, kDomShake);
  int64_t* y = a.y + g * 256;
  expand_mask_parse<BITS, kc::DevOps>(s, [&](uint32_t i, int32_t v) { y[i] = (int64_t)v; });
}

struct CtArgs { size_t active; uint32_t k; const uint32_t* live; const uint8_t* mu; const uint64_t* w; uint8_t* ct; };
template <uint32_t G2> __global__ __launch_bounds__(256) void k_sign_ctilde(CtArgs a) {
  const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= live_prefix(a.active, a.live)) return;
  const size_t fields = (size_t)a.k * 256;
  const W1Reader<G2, false> rd{a.mu + slot * 64, true, a.w + slot * fields, nullptr, fields};
  uint64_t s[25];
  zero_state(s);
  kc::absorb<kc::kRateShake256, kc::DevOps>(s, rd, 64 + fields * W1Reader<G2, false>::BITS / 8, kDomShake);
  put_words<0, 8>(s, a.ct + slot * 64);                                  // lambda / 4 <= 64 bytes are c~; the section has 64 per slot
}

// One workgroup per slot.  Every thread takes groups of 8 coefficients: of z (l polynomials), then of r = w - c s2 and c t0 together (k polynomials);
// the three norm bits are OR-ed and the hint bits counted in LDS by every thread whatever its values, and the 8 hint bits of a group are one byte of
// the mask in LDS.  Then the workgroup knows the accept bit, and only an accepted slot goes on to write its signature.
enum { FIRED_Z = 1, FIRED_R0 = 2, FIRED_CT0 = 4 };
struct CheckArgs {
  size_t active, sig_len;
  uint32_t k, l, cb, omega, zbound, rbound;
  const uint32_t* live;
  const uint64_t* z; const uint64_t* r; const uint64_t* ct0; const uint8_t* ct;
  uint32_t* kappa; const uint32_t* index; uint32_t* flags; uint32_t* ctl;
  uint8_t* sig; uint32_t* rounds; int* fail;
};
__device__ __forceinline__ void load8(const uint64_t* p, uint32_t (&v)[8]) {
  const v4u* src = reinterpret_cast<const v4u*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const v4u r = src[j];
    v[2 * j] = r[0];
    v[2 * j + 1] = r[2];
  }
}
template <uint32_t G2> __global__ __launch_bounds__(256) void k_sign_check(CheckArgs a) {
  constexpr int ZBITS = G2 == kGamma2Low ? 18 : 20;
  __shared__ uint32_t sh_bits, sh_cnt;
  __shared__ uint8_t hmask[8 * 32];
  const size_t slot = blockIdx.x;
  if (slot >= live_prefix(a.active, a.live)) return;
  const uint32_t tid = threadIdx.x, zitems = a.l * 32, items = (a.l + a.k) * 32;
  if (tid == 0) { sh_bits = 0; sh_cnt = 0; }
  __syncthreads();
  uint32_t bits = 0, cnt = 0;
  for (uint32_t item = tid; item < items; item += 256) {
    if (item < zitems) {
      uint32_t v[8];
      load8(a.z + (slot * a.l * 256 + (size_t)item * 8), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) bits |= norm_reaches(v[j], a.zbound) * FIRED_Z;
    } else {
      const uint32_t it = item - zitems;
      uint32_t rr[8], cc[8], hb = 0;
      load8(a.r + (slot * a.k * 256 + (size_t)it * 8), rr);
      load8(a.ct0 + (slot * a.k * 256 + (size_t)it * 8), cc);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bits |= low_reaches(low_bits<G2>(rr[j]), a.rbound) * FIRED_R0;
        bits |= norm_reaches(cc[j], G2) * FIRED_CT0;
        uint32_t sum = rr[j] + cc[j];
        sum -= kQ & (0u - (uint32_t)(sum >= kQ));
        const uint32_t h = make_hint<G2>(rr[j], sum);                     // MakeHint(-c t0, r + c t0)
        hb |= h << j;
        cnt += h;
      }
      hmask[it] = (uint8_t)hb;
    }
  }
  atomicOr(&sh_bits, bits);
  atomicAdd(&sh_cnt, cnt);
  __syncthreads();
  const bool accept = sh_bits == 0 && sh_cnt <= a.omega;
  const uint32_t idx = a.index[slot];
  if (tid == 0) {
    const uint32_t kap = a.kappa[slot] + a.l;
    a.kappa[slot] = kap;
    const bool retired = !accept && kappa_exhausted(kap, a.l);
    a.flags[slot] = accept || retired ? 1u : 0u;
    if (accept || retired) atomicAdd(a.ctl + CTL_DONE, 1u);
    if (retired && a.fail) atomicOr(a.fail, 2);
    if (accept && a.rounds) a.rounds[idx] = kap / a.l;
  }
  if (!accept) return;
  uint8_t* out = a.sig + (size_t)idx * a.sig_len;
  if (tid < a.cb) out[tid] = a.ct[slot * 64 + tid];
  for (uint32_t item = tid; item < zitems; item += 256) {
    uint32_t v[8], f[8];
    load8(a.z + (slot * a.l * 256 + (size_t)item * 8), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = value_to_field(1 << (ZBITS - 1), centered(v[j]));
    pack8<ZBITS>(out + a.cb + (size_t)item * ZBITS, f);
  }
  if (tid == 0) {
    uint8_t* y = out + a.cb + (size_t)zitems * ZBITS;
    hint_bit_pack([&](uint32_t i, uint32_t b) { return (uint32_t)hmask[i * 32 + b]; }, a.k, a.omega, [&](uint32_t pos, uint32_t v) { y[pos] = (uint8_t)v; });
  }
}

// After the attempt: the live set is [0, live) without the slots whose flag is set (only slots below min(active, live) were attempted).  A hole is such
// a slot below new_live = live - done; a source is a live slot at or beyond new_live; there are as many of one as of the other.
struct MatchArgs { size_t active; const uint32_t* live; const uint32_t* flags; uint32_t* ctl; uint32_t* holes; uint32_t* srcs; };
__global__ __launch_bounds__(256) void k_sign_match(MatchArgs a) {
  const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x, lv = *a.live;
  if (slot >= lv) return;
  const size_t m = a.active < lv ? a.active : lv, new_live = lv - a.ctl[CTL_DONE];
  const bool done = slot < m && a.flags[slot] != 0;
  if (slot < new_live && done) a.holes[atomicAdd(a.ctl + CTL_HOLES, 1u)] = (uint32_t)slot;
  if (slot >= new_live && !done) a.srcs[atomicAdd(a.ctl + CTL_SRCS, 1u)] = (uint32_t)slot;
}

struct MoveArgs {
  uint32_t kl, k, l, per_key;
  const uint32_t* ctl; const uint32_t* holes; const uint32_t* srcs;
  v4u* a_hat; v4u* s1; v4u* s2; v4u* t0;
  uint64_t* mu; uint64_t* rho; uint32_t* kappa; uint32_t* index;
};
__device__ __forceinline__ void move_rows(v4u* base, size_t vecs, size_t dst, size_t src, uint32_t tid) {
  for (size_t i = tid; i < vecs; i += 256) base[dst * vecs + i] = base[src * vecs + i];
}
__global__ __launch_bounds__(256) void k_sign_move(MoveArgs a) {
  const uint32_t i = blockIdx.x, tid = threadIdx.x;
  if (i >= a.ctl[CTL_HOLES]) return;
  const size_t src = a.srcs[i], dst = a.holes[i];
  if (tid < 8) a.mu[dst * 8 + tid] = a.mu[src * 8 + tid];
  else if (tid < 16) a.rho[dst * 8 + tid - 8] = a.rho[src * 8 + tid - 8];
  else if (tid == 16) a.kappa[dst] = a.kappa[src];
  else if (tid == 17) a.index[dst] = a.index[src];
  if (!a.per_key) return;
  move_rows(a.a_hat, (size_t)a.kl * 64, dst, src, tid);                   // an image is 1024 bytes: 64 vectors
  move_rows(a.s1, (size_t)a.l * 64, dst, src, tid);
  move_rows(a.s2, (size_t)a.k * 64, dst, src, tid);
  move_rows(a.t0, (size_t)a.k * 64, dst, src, tid);
}

__global__ __launch_bounds__(256) void k_sign_commit(uint32_t* live, uint32_t* ctl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *live -= ctl[CTL_DONE];
    for (int i = 0; i < CTL_WORDS; ++i) ctl[i] = 0;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
// sk_stride = 0: the four image sections hold one key.  During begin the unpacked s1, s2, t0 (keys (l + 2 k) polynomials of 64-bit words) lie at y and
// run on into w, c, z, ct0, which follow without a gap: count (2 l + 2 k + 1) polynomials.
struct SignWs : Layout { size_t a_hat, s1, s2, t0, mu, rho, kappa, index, ctl, y, w, c, z, ct0, ct, flags, holes, srcs; };
SignWs sign_ws(const Set& s, size_t count, bool per_key) {
  SignWs w;
  const u128 c = count, keys = per_key ? count : (count ? 1 : 0), k = s.k, el = s.l;
  w.a_hat = w.take(keys * k * el * 1024);
  w.s1 = w.take(keys * el * 1024);
  w.s2 = w.take(keys * k * 1024);
  w.t0 = w.take(keys * k * 1024);
  w.mu = w.take(c * 64);
  w.rho = w.take(c * 64);
  w.kappa = w.take(c * 4);
  w.index = w.take(c * 4);
  w.ctl = w.take(count ? CTL_WORDS * 4 : 0);
  w.y = w.take(c * el * 2048);
  w.w = w.take(c * k * 2048);
  w.c = w.take(c * 2048);
  w.z = w.take(c * el * 2048);
  w.ct0 = w.take(c * k * 2048);
  w.ct = w.take(c * 64);
  w.flags = w.take(c * 4);
  w.holes = w.take(c * 4);
  w.srcs = w.take(c * 4);
  return w;
}

struct SignIn { const uint8_t* sk; size_t sk_stride; const uint8_t* msg; size_t msg_len, msg_stride; int msg_kind; const uint8_t* rnd; };

psf_status begin_run(int device, const Set& s, size_t count, const SignIn& in, void* ws, const SignWs& w, uint32_t* live, int* fail, hipStream_t st) {
  const size_t k = s.k, l = s.l, keys = in.sk_stride ? count : 1;
  PSF_TRY(use_device(device));
  uint64_t* words = at<uint64_t>(ws, w.y);
  const SkArgs ua{keys, in.sk_stride, s.k, s.l, s.eta, in.sk, words};
  hipLaunchKernelGGL(k_sign_unpack, dim3(blocks_of(keys * (l + 2 * k) * 32, 256)), dim3(256), 0, st, ua);
  HIP_TRY(hipGetLastError());
  PSF_TRY(ntt_forward_dev(device, kQ, kN, keys * l, words, 64, at<uint32_t>(ws, w.s1), st));
  PSF_TRY(ntt_forward_dev(device, kQ, kN, keys * k, words + keys * l * kN, 64, at<uint32_t>(ws, w.s2), st));
  PSF_TRY(ntt_forward_dev(device, kQ, kN, keys * k, words + keys * (l + k) * kN, 64, at<uint32_t>(ws, w.t0), st));
  PSF_TRY(rej_ntt_launch(keys * k * l, s.k, s.l, in.sk, in.sk_stride, at<uint32_t>(ws, w.a_hat), true, fail, st));      // A_hat = ExpandA(rho), as images
  const SeedArgs sa{count, in.sk_stride, in.msg_len, in.msg_stride, in.msg_kind, in.sk, in.msg, in.rnd, at<uint64_t>(ws, w.mu), at<uint64_t>(ws, w.rho),
                    at<uint32_t>(ws, w.kappa), at<uint32_t>(ws, w.index), at<uint32_t>(ws, w.ctl), live};
  hipLaunchKernelGGL(k_sign_seed, dim3(blocks_of(count, 256)), dim3(256), 0, st, sa);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

psf_status round_run(int device, const Set& s, size_t count, bool per_key, size_t active, uint8_t* sig, uint32_t* rounds, void* ws, const SignWs& w,
                     uint32_t* live, int* fail, hipStream_t st) {
  const size_t k = s.k, l = s.l;
  PSF_TRY(use_device(device));
  if (active == 0) return PSF_OK;
  uint32_t *a_hat = at<uint32_t>(ws, w.a_hat), *s1 = at<uint32_t>(ws, w.s1), *s2 = at<uint32_t>(ws, w.s2), *t0 = at<uint32_t>(ws, w.t0);
  uint32_t *kappa = at<uint32_t>(ws, w.kappa), *index = at<uint32_t>(ws, w.index), *ctl = at<uint32_t>(ws, w.ctl), *flags = at<uint32_t>(ws, w.flags);
  uint32_t *holes = at<uint32_t>(ws, w.holes), *srcs = at<uint32_t>(ws, w.srcs);
  int64_t *y = at<int64_t>(ws, w.y), *wv = at<int64_t>(ws, w.w), *c = at<int64_t>(ws, w.c), *z = at<int64_t>(ws, w.z), *ct0 = at<int64_t>(ws, w.ct0);
  uint8_t *mu = at<uint8_t>(ws, w.mu), *rho = at<uint8_t>(ws, w.rho), *ct = at<uint8_t>(ws, w.ct);
  const bool low = s.gamma2 == (int32_t)kGamma2Low;

  const MaskArgs ma{active, s.l, live, rho, kappa, y};                                                       // y = ExpandMask(rho'', kappa)
  if (s.zbits == 18) hipLaunchKernelGGL(k_expand_mask<18>, dim3(blocks_of(active * l, 256)), dim3(256), 0, st, ma);
  else hipLaunchKernelGGL(k_expand_mask<20>, dim3(blocks_of(active * l, 256)), dim3(256), 0, st, ma);
  HIP_TRY(hipGetLastError());
  const NttMatShape ay{active, k, l, 1, 0}, cs1{active, l, 1, 1, 0}, ck{active, k, 1, 1, 0};
  PSF_TRY(ntt_matmul_dev(device, kQ, kN, ay, a_hat, per_key ? k * l * kN : 0, true, y, wv, 64, st));                 // w = A y
  const CtArgs ca{active, s.k, live, mu, reinterpret_cast<const uint64_t*>(wv), ct};                          // c~ = H(mu || w1Encode(HighBits(w)))
  if (low) hipLaunchKernelGGL(k_sign_ctilde<kGamma2Low>, dim3(blocks_of(active, 256)), dim3(256), 0, st, ca);
  else hipLaunchKernelGGL(k_sign_ctilde<kGamma2High>, dim3(blocks_of(active, 256)), dim3(256), 0, st, ca);
  HIP_TRY(hipGetLastError());
  PSF_TRY(ball_launch(active, s.tau, ct, s.cb, 64, c, fail, st));                                           // c = SampleInBall(c~)
  PSF_TRY(ntt_matfma_dev(device, kQ, kN, cs1, s1, per_key ? l * kN : 0, true, c, y, 1, z, 64, st));                  // z = y + c s1
  PSF_TRY(ntt_matfma_dev(device, kQ, kN, ck, s2, per_key ? k * kN : 0, true, c, wv, -1, wv, 64, st));                // r = w - c s2, over w
  PSF_TRY(ntt_matmul_dev(device, kQ, kN, ck, t0, per_key ? k * kN : 0, true, c, ct0, 64, st));                       // c t0
  const CheckArgs ka{active, s.sig, s.k, s.l, s.cb, s.omega, (uint32_t)(s.gamma1 - s.beta), (uint32_t)(s.gamma2 - s.beta), live,
                     reinterpret_cast<const uint64_t*>(z), reinterpret_cast<const uint64_t*>(wv), reinterpret_cast<const uint64_t*>(ct0), ct,
                     kappa, index, flags, ctl, sig, rounds, fail};
  if (low) hipLaunchKernelGGL(k_sign_check<kGamma2Low>, dim3((unsigned)active), dim3(256), 0, st, ka);
  else hipLaunchKernelGGL(k_sign_check<kGamma2High>, dim3((unsigned)active), dim3(256), 0, st, ka);
  HIP_TRY(hipGetLastError());
  const MatchArgs ta{active, live, flags, ctl, holes, srcs};
  hipLaunchKernelGGL(k_sign_match, dim3(blocks_of(count, 256)), dim3(256), 0, st, ta);
  HIP_TRY(hipGetLastError());
  const MoveArgs va{s.k * s.l, s.k, s.l, per_key ? 1u : 0u, ctl, holes, srcs, reinterpret_cast<v4u*>(a_hat), reinterpret_cast<v4u*>(s1), reinterpret_cast<v4u*>(s2),
                    reinterpret_cast<v4u*>(t0), reinterpret_cast<uint64_t*>(mu), reinterpret_cast<uint64_t*>(rho), kappa, index};
  hipLaunchKernelGGL(k_sign_move, dim3((unsigned)active), dim3(256), 0, st, va);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sign_commit, dim3(1), dim3(256), 0, st, live, ctl);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// ---- argument checks -------------------------------------------------------------------------------------------------------------------------------
struct SignChecked { Set s; SignWs w; };
bool kind_ok(int kind) { return kind == PSF_MLDSA_MSG_BYTES || kind == PSF_MLDSA_MSG_MU; }
bool stride_ok(const Set& s, size_t sk_stride) { return sk_stride == 0 || sk_stride >= s.sk; }

// the inputs of begin and, for the host form, sig and rounds; for the device form, d_live
psf_status begin_check(int param, size_t count, const SignIn& in, bool dev, const void* live, uint8_t* sig, uint32_t* rounds, const void* ws, size_t ws_bytes,
                       SignChecked* ck) {
  if (!set_of(param, &ck->s) || !kind_ok(in.msg_kind)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const Set& s = ck->s;
  Buf b[5] = {{in.sk, s.sk, in.sk_stride, false, false, 0}, {in.msg, in.msg_len, in.msg_stride, false, in.msg_len == 0, 0}, {in.rnd, 32, 32, false, true, 0},
              {dev ? live : sig, dev ? (size_t)4 : s.sig, dev ? (size_t)0 : s.sig, true, false, 0}, {rounds, 4, 4, true, true, 0}};
  const int nb = dev ? 4 : 5;
  PSF_TRY(check_null(b, nb));
  if (!stride_ok(s, in.sk_stride) || in.msg_stride < in.msg_len) return PSF_ERR_PARAM;
  if (in.msg_kind == PSF_MLDSA_MSG_MU && in.msg_len != 64) return PSF_ERR_PARAM;
  if (in.msg_len > SIZE_MAX - 64) return PSF_ERR_PARAM;
  ck->w = sign_ws(s, count, in.sk_stride != 0);
  PSF_TRY(check_rest(count, b, nb, ck->w, dev, ws, ws_bytes));
  if (dev && (uintptr_t)live % 4 != 0) return PSF_ERR_PARAM;
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

psf_status round_check(int param, size_t count, size_t sk_stride, size_t active, uint8_t* sig, uint32_t* rounds, const void* ws, size_t ws_bytes, const void* live,
                       SignChecked* ck) {
  if (!set_of(param, &ck->s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const Set& s = ck->s;
  Buf b[3] = {{sig, s.sig, s.sig, true, false, 0}, {rounds, 4, 4, true, true, 0}, {live, 4, 0, true, false, 0}};
  PSF_TRY(check_null(b, 3));
  if (!stride_ok(s, sk_stride) || active > count) return PSF_ERR_PARAM;
  ck->w = sign_ws(s, count, sk_stride != 0);
  PSF_TRY(check_rest(count, b, 3, ck->w, true, ws, ws_bytes));
  if ((uintptr_t)live % 4 != 0 || (uintptr_t)rounds % 4 != 0) return PSF_ERR_PARAM;
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

}  // namespace dsa
}  // namespace psf

using namespace psf;
using namespace psf::dsa;

extern "C" {

psf_status psf_mldsa_sign_workspace_bytes(int param, size_t count, size_t sk_stride, size_t* bytes) {
  Set s;
  if (!set_of(param, &s) || !bytes || !stride_ok(s, sk_stride)) return PSF_ERR_PARAM;
  const SignWs w = sign_ws(s, count, sk_stride != 0);
  if (!w.ok) return PSF_ERR_PARAM;
  *bytes = w.total;
  return PSF_OK;
}

psf_status psf_mldsa_sign_begin_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len,
                                    size_t msg_stride, int msg_kind, const uint8_t* d_rnd, void* d_ws, size_t ws_bytes, uint32_t* d_live, int* d_fail, void* stream) {
  SignChecked ck{};
  const SignIn in{d_sk, sk_stride, d_msg, msg_len, msg_stride, msg_kind, d_rnd};
  const psf_status rc = begin_check(param, count, in, true, d_live, nullptr, nullptr, d_ws, ws_bytes, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  return begin_run(device, ck.s, count, in, d_ws, ck.w, d_live, d_fail, (hipStream_t)stream);
}

psf_status psf_mldsa_sign_round_dev(int device, int param, size_t count, size_t sk_stride, size_t active, uint8_t* d_sig, uint32_t* d_rounds, void* d_ws,
                                    size_t ws_bytes, uint32_t* d_live, int* d_fail, void* stream) {
  SignChecked ck{};
  const psf_status rc = round_check(param, count, sk_stride, active, d_sig, d_rounds, d_ws, ws_bytes, d_live, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  return round_run(device, ck.s, count, sk_stride != 0, active, d_sig, d_rounds, d_ws, ck.w, d_live, d_fail, (hipStream_t)stream);
}

psf_status psf_mldsa_sign_end_dev(int device, int param, size_t count, size_t sk_stride, void* d_ws, size_t ws_bytes, void* stream) {
  Set s;
  if (!set_of(param, &s)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  if (!stride_ok(s, sk_stride)) return PSF_ERR_PARAM;
  const SignWs w = sign_ws(s, count, sk_stride != 0);
  if (!w.ok) return PSF_ERR_PARAM;
  PSF_TRY(check_ws(true, d_ws, ws_bytes, w.total));
  PSF_TRY(use_device(device));
  HIP_TRY(hipMemsetAsync(d_ws, 0, w.total, (hipStream_t)stream));
  return PSF_OK;
}

psf_status psf_mldsa_sign(int device, int param, size_t count, const uint8_t* sk, size_t sk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                          int msg_kind, const uint8_t* rnd, uint8_t* sig, uint32_t max_rounds, uint32_t* rounds) {
  SignChecked ck{};
  const SignIn in{sk, sk_stride, msg, msg_len, msg_stride, msg_kind, rnd};
  if (set_of(param, &ck.s) && kind_ok(msg_kind) && (max_rounds < 1 || (uint64_t)max_rounds * ck.s.l > 65536)) return PSF_ERR_PARAM;
  const psf_status rc = begin_check(param, count, in, false, nullptr, sig, rounds, nullptr, 0, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  const Set& s = ck.s;
  HostCall h;
  // the packed device copies change the layout only through sk_stride != 0, which din keeps
  const SignIn din{h.in(sk, count, s.sk, sk_stride, SECRET), sk_stride ? s.sk : 0, h.in(msg, count, msg_len, msg_stride), msg_len, msg_len, msg_kind,
                   h.in(rnd, count, 32, 32, SECRET)};
  uint8_t* dsig = h.out(count * s.sig, PUBLIC, true);
  uint32_t *drounds = reinterpret_cast<uint32_t*>(h.out(count * 4, PUBLIC, true)), *dlive = reinterpret_cast<uint32_t*>(h.out(4));
  void* dws = h.workspace(ck.w.total);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  psf_status run = begin_run(device, s, count, din, dws, ck.w, dlive, dflag, nullptr);
  uint32_t live = (uint32_t)count;
  for (uint32_t r = 0; run == PSF_OK && r < max_rounds && live != 0; ++r) {
    run = round_run(device, s, count, sk_stride != 0, live, dsig, drounds, dws, ck.w, dlive, dflag, nullptr);
    if (run == PSF_OK) run = h.fetch(&live, dlive, 4);
  }
  HIP_TRY(hipMemsetAsync(dws, 0, ck.w.total, nullptr));                   // everything in the workspace but A_hat is secret: cleared on every path
  PSF_TRY(run);
  PSF_TRY(h.fetch(sig, dsig, count * s.sig));
  PSF_TRY(h.fetch(rounds, drounds, count * 4));
  PSF_TRY(h.finish());
  return live != 0 ? PSF_ERR_SAMPLER : PSF_OK;
}

}  // extern "C"
