// psf_sample.hip -- free fills of device buffers with samples: uniform on [0, q), centred binomial, discrete Gaussian
//   (sample_uniform / sample_binomial / sample_discrete_gauss of MatZq, PolynomialRingZq, MatPolynomialRingZq and MatZ in qfall-math;
//   mp_perturbation.rs:222, trapdoor_distribution.rs, gadget_ring.rs).
// `count` polynomials of n coefficients, row-major, polynomial first_index + c at offset c n.  Every value is a pure function of
// (seed, tag, global polynomial index, coefficient) through the randomness contract of psf_rng.hpp (DESIGN.md "Randomness contract"), so a
// fill of [0, 8) is the fill of [0, 3) followed by the fill of [3, 8).  No division by a runtime value on the device: the host passes
// multipliers (div_u64 / div_u32 below), the Lemire thresholds and the constants of SampleZ.
#include <cmath>
#include <cstdlib>
#include "psf_hip_util.hpp"
#include "psf_stream_host.hpp"
#include "psf_rng.hpp"

namespace psf {
namespace smp {

// floor(s / d) without a division: m = floor((2^W - 1) / d) gives floor(s m / 2^W) in {floor(s/d) - 1, floor(s/d)} for every s < 2^W
// (s/d - s m/2^W = s (2^W - m d) / (d 2^W) <= s / 2^W < 1), and one comparison settles it.
__device__ __forceinline__ uint64_t div_u64(uint64_t s, uint64_t d, uint64_t m) {
  const uint64_t t = __umul64hi(s, m);
  return t + ((t + 1) * d <= s);                                        // (t + 1) d <= s + d: no overflow for s + d < 2^64 (s < 2^63 here)
}
__device__ __forceinline__ uint32_t div_u32(uint32_t s, uint32_t d, uint32_t m) {
  const uint32_t t = __umulhi(s, m);
  return t + ((uint64_t)(t + 1) * d <= s);
}

// where a flat offset lies: polynomial c = floor(e / n), coefficient i = e mod n
struct Shape { uint64_t n, mn; };                                       // mn = floor((2^64 - 1) / n)
__device__ __forceinline__ void locate(const Shape sh, uint64_t e, uint64_t* c, uint32_t* i) {
  const uint64_t cc = div_u64(e, sh.n, sh.mn);
  *c = cc;
  *i = (uint32_t)(e - cc * sh.n);
}

template <int IO> struct Word { typedef int16_t type; };
template <> struct Word<64> { typedef int64_t type; };

__device__ __forceinline__ int lane_rank(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// ---- uniform on [0, q) ---------------------------------------------------------------------------------------------------------------------
// uniform_mod of psf_rng.hpp with its threshold 2^64 mod q supplied by the host (the contract's own form divides by q)
__device__ __forceinline__ uint64_t uniform_thr(uint64_t seed, uint32_t tw, uint32_t c0, uint32_t c1, uint64_t q, uint64_t thr) {
  for (uint32_t t = 0;; ++t) {
    const U4 w = philox(seed, c0, c1, t, tw);
    const uint64_t x = ((uint64_t)w.y << 32) | w.x;
    if (x * q >= thr || t == 63) return __umul64hi(x, q);
  }
}

struct FillArgs { uint64_t seed, first_index; uint32_t tag; Shape sh; };

// elements [0, head) and [head + EPV nvec, total) word by word, the nvec 16-byte vectors between them (16-byte aligned in `out`) by a
// grid-stride loop: one coefficient per lane per Philox block, the redraws inside the lane, one coalesced non-temporal store per vector
template <int IO>
__global__ __launch_bounds__(256) void k_fill_uniform(FillArgs a, uint64_t q, uint64_t thr, void* __restrict__ out, size_t total, size_t head, size_t nvec) {
  constexpr size_t EPV = IO == 16 ? 8 : 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  v4u* vout = reinterpret_cast<v4u*>(static_cast<char*>(out) + head * (IO / 8));
  for (size_t v = gid; v < nvec; v += stride) {
    uint64_t c;
    uint32_t i;
    locate(a.sh, head + v * EPV, &c, &i);
    uint64_t val[EPV];
#pragma unroll
    for (size_t j = 0; j < EPV; ++j) {
      const uint64_t idx = a.first_index + c;
      val[j] = uniform_thr(a.seed, tag_word(a.tag, idx), i, (uint32_t)idx, q, thr);
      if (++i == (uint32_t)a.sh.n) { i = 0; ++c; }                      // (n < 2^32; n = 2^32 - 1 wraps at the same place)
    }
    v4u r;
    if constexpr (IO == 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = (uint32_t)val[2 * j] | ((uint32_t)val[2 * j + 1] << 16);
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) { r[2 * j] = (uint32_t)val[j]; r[2 * j + 1] = (uint32_t)(val[j] >> 32); }
    }
    __builtin_nontemporal_store(r, vout + v);
  }
  const size_t body = nvec * EPV, rest = total - head - body;
  for (size_t g = gid; g < head + rest; g += stride) {
    const size_t e = g < head ? g : g + body;
    uint64_t c;
    uint32_t i;
    locate(a.sh, e, &c, &i);
    const uint64_t idx = a.first_index + c;
    const uint64_t x = uniform_thr(a.seed, tag_word(a.tag, idx), i, (uint32_t)idx, q, thr);
    if constexpr (IO == 16) static_cast<uint16_t*>(out)[e] = (uint16_t)x;
    else static_cast<uint64_t*>(out)[e] = x;
  }
}

// ---- centred binomial ------------------------------------------------------------------------------------------------------------------------
// s_w = floor(16 / eta) slots of 2 eta bits per 32-bit word, bw = 4 s_w coefficients per Philox block (c0 = block, c1 = index, c2 = 0);
// coefficient i: block floor(i / bw), word floor(i / s_w) mod 4, slot i mod s_w, value popcount(low eta bits) - popcount(high eta bits).
struct CbdArgs {
  uint32_t eta, sw, bw, sh2;   // sh2 = 2 eta
  uint32_t fmask, lomask;      // 2^(2 eta) - 1, 2^eta - 1
  uint32_t mbw, msw;           // floor((2^32 - 1) / bw), ... / sw
  uint64_t nblk, mnblk;        // blocks per polynomial ceil(n / bw) and floor((2^64 - 1) / nblk)
};

__device__ __forceinline__ int cbd_field(const CbdArgs& b, uint32_t f) {
  return __popc(f & b.lomask) - __popc(f >> b.eta);
}

constexpr int kTileVec = 1024;                                          // 16-byte vectors per tile: 4 per lane of a 256-lane workgroup, 16 KiB

// Whole tiles of 8192 16-bit or 2048 64-bit values (16-byte aligned in `out`): a lane owns whole Philox blocks -- block k, k + 256, ... of those
// that meet the tile -- and parks their values in LDS; the tile leaves as 4 coalesced 16-byte non-temporal stores per lane.  A block that
// straddles a tile edge is drawn by both tiles (each keeps its own part), so a tile needs nothing from its neighbours.  Everything outside
// whole tiles -- the head before the first 16-byte boundary and the ragged end -- runs value by value, one block per value.
template <int IO>
__global__ __launch_bounds__(256) void k_fill_cbd(FillArgs a, CbdArgs b, void* __restrict__ out, size_t total, size_t head, size_t ntiles) {
  typedef typename Word<IO>::type word_t;
  constexpr uint32_t EPV = IO == 16 ? 8 : 2, TV = kTileVec * EPV;
  __shared__ v4u s_val[kTileVec];
  word_t* sv = reinterpret_cast<word_t*>(s_val);
  const uint32_t tid = threadIdx.x;
  auto block_of = [&](uint64_t e) -> uint64_t {                          // the global block (polynomial * nblk + block) of flat offset e
    uint64_t c;
    uint32_t i;
    locate(a.sh, e, &c, &i);
    return c * b.nblk + div_u32(i, b.bw, b.mbw);
  };
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t e0 = head + t * (uint64_t)TV;
    const uint64_t gb0 = block_of(e0);
    const uint32_t nb = (uint32_t)(block_of(e0 + TV - 1) - gb0) + 1;    // at most TV blocks (n = 1)
    for (uint32_t k = tid; k < nb; k += 256) {
      const uint64_t gb = gb0 + k;
      const uint64_t c = div_u64(gb, b.nblk, b.mnblk);
      const uint32_t blk = (uint32_t)(gb - c * b.nblk);
      const uint64_t idx = a.first_index + c;
      const U4 w = philox(a.seed, blk, (uint32_t)idx, 0, tag_word(a.tag, idx));
      const uint32_t word[4] = {w.x, w.y, w.z, w.w};
      const uint64_t i0 = (uint64_t)blk * b.bw;
      const uint64_t left = a.sh.n - i0;                                 // coefficients from this block to the end of the polynomial: >= 1
      const uint32_t lim = left < b.bw ? (uint32_t)left : b.bw;
      const int64_t pos0 = (int64_t)(c * a.sh.n + i0) - (int64_t)e0;
      uint32_t j = 0;
#pragma unroll
      for (int wd = 0; wd < 4; ++wd) {
        uint64_t bits = word[wd];
#pragma clang loop unroll(disable)
        for (uint32_t s = 0; s < b.sw; ++s, ++j) {
          const int v = cbd_field(b, (uint32_t)bits & b.fmask);
          bits >>= b.sh2;
          const uint64_t p = (uint64_t)(pos0 + (int64_t)j);
          if (j < lim && p < TV) sv[p] = (word_t)v;
        }
      }
    }
    __syncthreads();
    v4u* vout = reinterpret_cast<v4u*>(static_cast<char*>(out) + e0 * (IO / 8));
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(s_val[tid + 256 * u], vout + tid + 256 * u);
    __syncthreads();
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t body = ntiles * (size_t)TV, rest = total - head - body;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + tid; g < head + rest; g += stride) {
    const size_t e = g < head ? g : g + body;
    uint64_t c;
    uint32_t i;
    locate(a.sh, e, &c, &i);
    const uint32_t blk = div_u32(i, b.bw, b.mbw), j = i - blk * b.bw;
    const uint32_t wd = div_u32(j, b.sw, b.msw), s = j - wd * b.sw;
    const uint64_t idx = a.first_index + c;
    const U4 w = philox(a.seed, blk, (uint32_t)idx, 0, tag_word(a.tag, idx));
    const uint32_t word = (wd & 2) ? ((wd & 1) ? w.w : w.z) : ((wd & 1) ? w.y : w.x);
    const int v = cbd_field(b, (word >> (b.sh2 * s)) & b.fmask);        // 2 eta s <= 32 - 2 eta
    static_cast<word_t*>(out)[e] = (word_t)v;
  }
}

// ---- discrete Gaussian -------------------------------------------------------------------------------------------------------------------------
// Both kernels cut the fill into segments of `seg` samples (a multiple of 64), one per wave, and run the compacted rejection loop of
// k_perturb_round_lean: a lane that accepts takes the next undone sample of its wave's segment, so no lane waits for the slowest of 64.  The
// value of a sample is the first accepted attempt of its own Philox stream, whichever lane evaluates it.  Segments are laid so that every
// segment but the first starts on a 16-byte boundary of `out`: the flat offset of sample `off` of wave w is w seg + off - pad, and wave 0
// starts at off = pad (pad = seg - head when the buffer starts `head` words before a boundary, else 0).
struct SegArgs { uint32_t seg, pad; };

// Shared centre, narrow words: one (c, s) for the whole fill, so the acceptance threshold of every candidate is a constant of the call.  The
// prologue tabulates, per candidate x = lo + k, ru = floor(rho 2^16) and the tie word floor((rho 2^16 - ru) 2^32) with the exact rule of
// sz_decide; after the barrier an attempt is a 24-bit multiply, Lemire's test, one LDS word and a compare -- no exponential and no f64.  A tie
// (wb == ru) draws the side block 0x80000000 | t.  The accepted candidate indices are parked in the wave's LDS strip (0xffff: the attempt cap)
// and leave as coalesced 16-byte non-temporal vectors when the segment is done.
struct TabArgs {
  long long lo;            // first candidate ceil(c) - ceil(6 s)
  long long cap_value;     // floor(c + 1/2): the value of a draw that ends at the attempt cap
  double center, inv_s;
  uint32_t N, thr;         // candidates (<= 4096) and 2^16 mod N
};

template <int IO>
__global__ __launch_bounds__(256) void k_fill_gauss_tab(FillArgs a, TabArgs tb, SegArgs sg, void* __restrict__ out, int* __restrict__ fail, size_t total) {
  typedef typename Word<IO>::type word_t;
  constexpr uint32_t EPV = IO == 16 ? 8 : 2;
  extern __shared__ uint32_t s_dyn[];
  uint32_t* s_ru = s_dyn;                                               // [N]
  uint32_t* s_tie = s_dyn + tb.N;                                       // [N]
  uint16_t* strip = reinterpret_cast<uint16_t*>(s_dyn + 2 * tb.N) + (threadIdx.x >> 6) * sg.seg;   // [seg] per wave
  for (uint32_t k = threadIdx.x; k < tb.N; k += 256) {
    const double d = ((double)(tb.lo + (long long)k) - tb.center) * tb.inv_s;
    const double rs = det_exp(-3.14159265358979323846 * (d * d)) * 65536.0;
    const double rf = floor(rs);
    s_ru[k] = (uint32_t)(uint64_t)rf;                                   // up to 2^16 (rho = 1): every wb accepts
    s_tie[k] = (uint32_t)(uint64_t)floor((rs - rf) * 4294967296.0);
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wv = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t v0 = wv * sg.seg;                                      // the wave's first sample, in offsets shifted by pad
  if (v0 >= total + sg.pad) return;                                     // (no workgroup barrier below: a wave may leave alone)
  const uint32_t off_lo = wv == 0 ? sg.pad : 0;
  const uint64_t room = total + sg.pad - v0;
  const uint32_t off_hi = room < sg.seg ? (uint32_t)room : sg.seg;
  uint32_t my = off_lo + lane, next_free = off_lo + 64;
  bool active = my < off_hi;
  uint32_t coord = 0, idx_lo = 0, tw = 0, t = 0;
  auto take = [&](uint32_t off) {
    uint64_t c;
    locate(a.sh, v0 + off - sg.pad, &c, &coord);
    const uint64_t idx = a.first_index + c;
    idx_lo = (uint32_t)idx;
    tw = tag_word(a.tag, idx);
    t = 0;
  };
  if (active) take(my);
  int f = 0;
  while (__ballot(active)) {
    bool accept = false;
    uint32_t xi = 0;
    if (active) {
      const U4 w = philox(a.seed, coord, idx_lo, t, tw);
      const uint32_t word[4] = {w.x, w.y, w.z, w.w};
      uint32_t ci[4], ru[4];
      bool maybe[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t prod = __umul24(word[j] >> 16, tb.N);
        ci[j] = prod >> 16;
        ru[j] = s_ru[ci[j]];
        maybe[j] = (prod & 0xffffu) >= tb.thr && (word[j] & 0xffffu) <= ru[j];      // Lemire: void below the threshold
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!accept && maybe[j]) {
          bool ok = (word[j] & 0xffffu) < ru[j];
          if (!ok) ok = philox(a.seed, coord, idx_lo, 0x80000000u | (4 * t + (uint32_t)j), tw).x < s_tie[ci[j]];   // the tie
          if (ok) { accept = true; xi = ci[j]; }
        }
      if (!accept && ++t >= kMaxAttempts / 4) { accept = true; f = 1; xi = 0xffffu; }
      if (accept) strip[my] = (uint16_t)xi;
    }
    const uint64_t mask = __ballot(accept);
    if (mask) {
      const uint32_t nid = next_free + (uint32_t)lane_rank(mask);
      next_free += (uint32_t)__popcll(mask);
      if (accept) {
        my = nid;
        active = nid < off_hi;
        if (active) take(nid);
      }
    }
  }
  if (f && fail) atomicOr(fail, 1);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  auto value = [&](uint32_t off) -> long long {
    const uint32_t k = strip[off];
    return k == 0xffffu ? tb.cap_value : tb.lo + (long long)k;
  };
  char* base = static_cast<char*>(out) + ((int64_t)v0 - (int64_t)sg.pad) * (IO / 8);    // wave 0 with a pad: only offsets >= pad are touched
  for (uint32_t o = lane * EPV; o < off_hi; o += 64 * EPV) {
    if (o >= off_lo && o + EPV <= off_hi) {
      v4u r;
      if constexpr (IO == 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = ((uint32_t)value(o + 2 * j) & 0xffffu) | ((uint32_t)value(o + 2 * j + 1) << 16);
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint64_t x = (uint64_t)value(o + j);
          r[2 * j] = (uint32_t)x;
          r[2 * j + 1] = (uint32_t)(x >> 32);
        }
      }
      __builtin_nontemporal_store(r, reinterpret_cast<v4u*>(base + (size_t)o * (IO / 8)));
    } else {
      for (uint32_t j = 0; j < EPV; ++j)
        if (o + j >= off_lo && o + j < off_hi) reinterpret_cast<word_t*>(base)[o + j] = (word_t)value(o + j);
    }
  }
}

// Every other case -- per-element centres, wide s: the same compacted loop over sz_group4 / sz_group4_narrow with the fp32 screen of the
// contract; the exact decisions are sz_decide's, so the values are sample_z's bit for bit.  A centre at or beyond 2^62 writes 0 and raises the flag.
template <int IO>
__global__ __launch_bounds__(256) void k_fill_gauss(FillArgs a, SampleZParams sp, double center, const double* __restrict__ centers, SegArgs sg,
                                                    void* __restrict__ out, int* __restrict__ fail, size_t total) {
  typedef typename Word<IO>::type word_t;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wv = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t v0 = wv * sg.seg;
  if (v0 >= total + sg.pad) return;
  const uint32_t off_lo = wv == 0 ? sg.pad : 0;
  const uint64_t room = total + sg.pad - v0;
  const uint32_t off_hi = room < sg.seg ? (uint32_t)room : sg.seg;
  word_t* base = reinterpret_cast<word_t*>(static_cast<char*>(out) + ((int64_t)v0 - (int64_t)sg.pad) * (IO / 8));
  uint32_t my = off_lo + lane, next_free = off_lo + 64;
  bool active = my < off_hi;
  const float inv_s_f = (float)sp.inv_s;
  double c = 0.0;
  float c_rel = 0.f;
  uint32_t coord = 0, idx_lo = 0, tw = 0, t = 0;
  SzRange rg{0, 1, 0, 16};
  bool generic = false, dead = false;
  auto take = [&](uint32_t off) {
    const uint64_t e = v0 + off - sg.pad;
    uint64_t pc;
    locate(a.sh, e, &pc, &coord);
    const uint64_t idx = a.first_index + pc;
    idx_lo = (uint32_t)idx;
    tw = tag_word(a.tag, idx);
    c = centers ? centers[e] : center;
    dead = !(fabs(c) < 0x1.0p62);                                       // no room for the candidates in 64-bit integers: 0, reported
    const double cs = dead ? 0.0 : c;
    rg = sz_range(cs, sp);
    c_rel = (float)((double)rg.lo - cs);
    generic = sp.sh != 16 || !(fabs(cs) < 0x1.0p40);
    t = 0;
  };
  if (active) take(my);
  int f = 0;
  while (__ballot(active)) {
    bool accept = false;
    long long x = 0;
    if (active) {
      if (dead) { accept = true; f = 1; }
      else {
        accept = generic ? sz_group4(a.seed, coord, idx_lo, tw, t, rg, c, sp.inv_s, &x)
                         : sz_group4_narrow(a.seed, coord, idx_lo, tw, t, rg, c, sp.inv_s, c_rel, inv_s_f, &x);
        if (!accept && ++t >= kMaxAttempts / 4) { accept = true; f = 1; x = (long long)floor(c + 0.5); }
      }
      if (accept) base[my] = (word_t)x;
    }
    const uint64_t mask = __ballot(accept);
    if (mask) {
      const uint32_t nid = next_free + (uint32_t)lane_rank(mask);
      next_free += (uint32_t)__popcll(mask);
      if (accept) {
        my = nid;
        active = nid < off_hi;
        if (active) take(nid);
      }
    }
  }
  if (f && fail) atomicOr(fail, 1);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------

// the checks every fill shares, in the order of the header; *total = count n
psf_status check_fill(uint32_t tag, int io_bits, uint64_t first_index, size_t count, size_t n, const void* out, size_t* total) {
  if (tag < 64 || tag > 255) return PSF_ERR_PARAM;
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  if (n == 0 || (uint64_t)n >= (1ull << 32)) return PSF_ERR_PARAM;
  const uint64_t cap = 1ull << 56;
  if (first_index > cap || (uint64_t)count > cap - first_index) return PSF_ERR_PARAM;
  if (count > SIZE_MAX / n || count * n > SIZE_MAX / 16) return PSF_ERR_PARAM;      // 8 bytes per word and 8 per centre
  if (count && !out) return PSF_ERR_PARAM;
  *total = count * n;
  return PSF_OK;
}

FillArgs fill_args(uint64_t seed, uint32_t tag, uint64_t first_index, size_t n) {
  return FillArgs{seed, first_index, tag, Shape{(uint64_t)n, ~0ull / (uint64_t)n}};
}

psf_status uniform_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t n, size_t total, uint64_t q, void* out, int io_bits, hipStream_t st) {
  if (total == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const size_t wb = (size_t)io_bits / 8, epv = 16 / wb;
  const StreamSplit sp = split_stream((uintptr_t)out, wb, total, epv);
  const size_t head = sp.head, nvec = sp.nvec, swork = total - nvec * epv;
  const dim3 grid(grid_blocks(nvec > swork ? nvec : swork, 0, cus, 8));      // 8 workgroups of 256 lanes per CU: 8 waves per SIMD
  const FillArgs a = fill_args(seed, tag, first_index, n);
  const uint64_t thr = (0 - q) % q;
  for_int<16, 64>(io_bits, [&](auto io) {
    hipLaunchKernelGGL((k_fill_uniform<decltype(io)::value>), grid, dim3(256), 0, st, a, q, thr, out, total, head, nvec);
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

psf_status cbd_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t n, size_t total, uint32_t eta, void* out, int io_bits, hipStream_t st) {
  if (total == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const size_t wb = (size_t)io_bits / 8, tv = (size_t)kTileVec * (16 / wb);
  const StreamSplit sp = split_stream((uintptr_t)out, wb, total, tv);      // head words first, then whole tiles
  const size_t head = sp.head, ntiles = sp.nvec;
  const dim3 grid(grid_blocks(total - ntiles * tv, ntiles, cus, 8));      // 16 KiB of LDS per workgroup of 4 waves
  CbdArgs b{};
  b.eta = eta;
  b.sw = 16 / eta;
  b.bw = 4 * b.sw;
  b.sh2 = 2 * eta;
  b.fmask = (uint32_t)((1ull << (2 * eta)) - 1);
  b.lomask = (1u << eta) - 1;
  b.mbw = 0xffffffffu / b.bw;
  b.msw = 0xffffffffu / b.sw;
  b.nblk = ((uint64_t)n + b.bw - 1) / b.bw;
  b.mnblk = ~0ull / b.nblk;
  const FillArgs a = fill_args(seed, tag, first_index, n);
  for_int<16, 64>(io_bits, [&](auto io) {
    hipLaunchKernelGGL((k_fill_cbd<decltype(io)::value>), grid, dim3(256), 0, st, a, b, out, total, head, ntiles);
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// samples per wave: about 16 waves per CU for small fills, up to 2048 samples as the fill grows (a wave's last samples run with most lanes
// idle, so long segments waste least; the table kernel parks 2 bytes per sample in LDS)
uint32_t gauss_segment(size_t total, int cus) {
  size_t seg = (total / ((size_t)cus * 16) + 63) / 64 * 64;
  if (seg < 64) seg = 64;
  return (uint32_t)(seg > 2048 ? 2048 : seg);
}

// (experiments build: PSF_SAMPLE_GENERAL=1 sends a shared narrow centre to the general kernel too -- tools/time_sample_fill.py times the two side by side)
psf_status gauss_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t n, size_t total, double center, const double* centers, double s,
                     void* out, int* fail, int io_bits, hipStream_t st) {
  if (total == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const size_t wb = (size_t)io_bits / 8;
  const SampleZParams sp = make_sample_z_params(s);
  SegArgs sg;
  sg.seg = gauss_segment(total, cus);
  const size_t head = head_words((uintptr_t)out, wb, total);
  sg.pad = head ? sg.seg - (uint32_t)head : 0;
  const size_t waves = (total + sg.pad + sg.seg - 1) / sg.seg;
  const dim3 grid((unsigned)((waves + 3) / 4));
  const FillArgs a = fill_args(seed, tag, first_index, n);
  bool table = !centers && sp.sh == 16 && fabs(center) < 0x1.0p62;
#if defined(PSF_EXPERIMENTS)
  if (const char* e = getenv("PSF_SAMPLE_GENERAL")) table = table && e[0] != '1';
#endif
  if (table) {
    const SzRange rg = sz_range(center, sp);
    TabArgs tb;
    tb.lo = rg.lo;
    tb.cap_value = (long long)floor(center + 0.5);
    tb.center = center;
    tb.inv_s = sp.inv_s;
    tb.N = rg.N;
    tb.thr = rg.thr;
    const size_t lds = (size_t)2 * tb.N * sizeof(uint32_t) + (size_t)4 * sg.seg * sizeof(uint16_t);      // at most 32 + 16 KiB
    for_int<16, 64>(io_bits, [&](auto io) {
      hipLaunchKernelGGL((k_fill_gauss_tab<decltype(io)::value>), grid, dim3(256), lds, st, a, tb, sg, out, fail, total);
    });
  } else {
    for_int<16, 64>(io_bits, [&](auto io) {
      hipLaunchKernelGGL((k_fill_gauss<decltype(io)::value>), grid, dim3(256), 0, st, a, sp, center, centers, sg, out, fail, total);
    });
  }
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

psf_status check_uniform(uint64_t q, int io_bits) {
  if (q >= (1ull << 62)) return PSF_ERR_UNSUPPORTED;
  if (io_bits == 16 && q > (1ull << 16)) return PSF_ERR_UNSUPPORTED;
  return PSF_OK;
}
psf_status check_gauss_param(double center, const double* centers, double s) {
  if (!std::isfinite(s) || !(s > 0.0)) return PSF_ERR_PARAM;
  if (!centers && !std::isfinite(center)) return PSF_ERR_PARAM;
  return PSF_OK;
}
psf_status check_gauss_support(double center, const double* centers, double s, int io_bits) {
  if (s > 0x1.0p28) return PSF_ERR_UNSUPPORTED;                         // the candidate count must fit the contract's 32-bit N
  if (io_bits == 16 && (centers || !(fabs(center) + 6.0 * s + 1.0 < 32768.0))) return PSF_ERR_UNSUPPORTED;
  return PSF_OK;
}

// The three fills behind their entry points: the checks in the header's order (every PSF_ERR_PARAM before every PSF_ERR_UNSUPPORTED), then the
// device form in `st`, or (host) the host-pointer form: allocate, run on the device (64-bit words), copy out.  No CPU fallback.
enum { K_UNIFORM = 0, K_CBD = 1, K_GAUSS = 2 };
struct FillSpec { int kind; uint64_t q; uint32_t eta; double center; const double* centers; double s; };

psf_status fill_dev(const FillSpec& f, int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t n, size_t total, void* out, int* fail, int io_bits,
                    hipStream_t st) {
  if (f.kind == K_UNIFORM) return uniform_dev(device, seed, tag, first_index, n, total, f.q, out, io_bits, st);
  if (f.kind == K_CBD) return cbd_dev(device, seed, tag, first_index, n, total, f.eta, out, io_bits, st);
  return gauss_dev(device, seed, tag, first_index, n, total, f.center, f.centers, f.s, out, fail, io_bits, st);
}

psf_status fill_host(FillSpec f, int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t n, size_t total, void* out) {
  if (total == 0) return PSF_OK;
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  const size_t bytes = total * sizeof(uint64_t);
  DevBuf dout, dcen, dflag;
  HIP_TRY(dout.alloc(bytes));
  if (f.kind == K_GAUSS) {
    HIP_TRY(dflag.alloc(sizeof(int)));
    HIP_TRY(dflag.zero(sizeof(int)));
    if (f.centers) {
      HIP_TRY(dcen.alloc(bytes));
      HIP_TRY(dcen.upload(f.centers, bytes));
      f.centers = dcen.as<double>();
    }
  }
  const psf_status rc = fill_dev(f, device, seed, tag, first_index, n, total, dout.as<void>(), dflag.as<int>(), 64, nullptr);
  if (rc != PSF_OK) return rc;
  HIP_TRY(dout.download(out, bytes));
  if (f.kind == K_GAUSS) {
    int fl = 0;
    HIP_TRY(dflag.download(&fl, sizeof(int)));
    if (fl) return PSF_ERR_SAMPLER;
  }
  return PSF_OK;
}

psf_status fill_call(const FillSpec& f, int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, void* out, int* fail, int io_bits,
                     void* st, bool host = false) {
  size_t total = 0;
  psf_status rc = check_fill(tag, io_bits, first_index, count, n, out, &total);
  if (rc == PSF_OK && f.kind == K_UNIFORM) rc = f.q < 2 ? PSF_ERR_PARAM : check_uniform(f.q, io_bits);
  if (rc == PSF_OK && f.kind == K_CBD) rc = f.eta == 0 ? PSF_ERR_PARAM : f.eta > 16 ? PSF_ERR_UNSUPPORTED : PSF_OK;
  if (rc == PSF_OK && f.kind == K_GAUSS) rc = check_gauss_param(f.center, f.centers, f.s);
  if (rc == PSF_OK && f.kind == K_GAUSS) rc = check_gauss_support(f.center, f.centers, f.s, io_bits);
  if (rc != PSF_OK) return rc;
  return host ? fill_host(f, device, seed, tag, first_index, n, total, out)
              : fill_dev(f, device, seed, tag, first_index, n, total, out, fail, io_bits, (hipStream_t)st);
}

}  // namespace smp
}  // namespace psf

using namespace psf::smp;

extern "C" {

psf_status psf_sample_uniform_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint64_t q, void* d_out, int io_bits,
                                  void* stream) {
  return fill_call({K_UNIFORM, q, 0, 0.0, nullptr, 0.0}, device, seed, tag, first_index, count, n, d_out, nullptr, io_bits, stream);
}
psf_status psf_sample_cbd_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint32_t eta, void* d_out, int io_bits,
                              void* stream) {
  return fill_call({K_CBD, 0, eta, 0.0, nullptr, 0.0}, device, seed, tag, first_index, count, n, d_out, nullptr, io_bits, stream);
}
psf_status psf_sample_discrete_gauss_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, double center,
                                         const double* d_centers, double s, void* d_out, int* d_fail, int io_bits, void* stream) {
  return fill_call({K_GAUSS, 0, 0, center, d_centers, s}, device, seed, tag, first_index, count, n, d_out, d_fail, io_bits, stream);
}
psf_status psf_sample_uniform(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint64_t q, uint64_t* out) {
  return fill_call({K_UNIFORM, q, 0, 0.0, nullptr, 0.0}, device, seed, tag, first_index, count, n, out, nullptr, 64, nullptr, true);
}
psf_status psf_sample_cbd(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint32_t eta, int64_t* out) {
  return fill_call({K_CBD, 0, eta, 0.0, nullptr, 0.0}, device, seed, tag, first_index, count, n, out, nullptr, 64, nullptr, true);
}
psf_status psf_sample_discrete_gauss(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, double center,
                                     const double* centers, double s, int64_t* out) {
  return fill_call({K_GAUSS, 0, 0, center, centers, s}, device, seed, tag, first_index, count, n, out, nullptr, 64, nullptr, true);
}

}  // extern "C"
