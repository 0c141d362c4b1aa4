// psf_ntt.hip -- NTT products over R_q = Z_q[X]/(X^n + 1) and Z_q[X]/(X^n - 1): plan cache, shape dispatch and launches (psf_ntt_api.hpp).
// PolynomialRingZq multiplication under gadget_ring.rs:78 and gpv_ring.rs:243-247; the kernels are in psf_ntt_kernels.hpp / psf_ntt_core.hpp.  They read
// the ring from the table of zetas alone (NttDev::zetas), so the cyclic ring takes the same instantiations with the table of make_ntt_plan_cyclic.
// The list of wave shapes is psf_ntt_shapes.hpp; the launch skeleton of every wave kernel and the launch of the matrix products are psf_ntt_launch.hpp,
// which psf_ntt_fma.hip instantiates a second time for the fused products C = E +- op(A) B (k_matpoly_fma), through the plan access of psf_ntt_api.hpp.
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include "psf_host.hpp"
#include "psf_ntt_launch.hpp"

using namespace psf;
using namespace psf::ntt;

namespace {

// ---- generic form: any power-of-two n <= 8192, any plan (leaf degree d = n >> L of any size), 32-bit Montgomery arithmetic, data in LDS ------------
// One product per workgroup at a time; the n/2 butterflies of a and of b of one level run side by side (n threads busy), leaves by schoolbook.
__global__ __launch_bounds__(256) void k_ntt_polymul_lds(NttDev p, uint32_t n, uint32_t L, uint32_t d, const uint64_t* __restrict__ A, const int64_t* __restrict__ Bp,
                                                         uint64_t* __restrict__ out, size_t count) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_smem[];   // zetas fwd [2^L] | inv [2^L] | a[n] | b[n] | c[n]
  const Mod32<DevWave> md = make_policy<0>(p, 0);
  uint32_t* zf = lds_smem;
  uint32_t* zi = zf + (1u << L);
  uint32_t* sa = zi + (1u << L);
  uint32_t* sb = sa + n;
  uint32_t* sc = sb + n;
  for (uint32_t i = threadIdx.x; i < (2u << L); i += 256) zf[i] = p.zetas[i];
  for (size_t pr = blockIdx.x; pr < count; pr += gridDim.x) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
      sa[i] = (uint32_t)(A[pr * n + i] % p.q);
      const int64_t v = Bp[pr * n + i] % (int64_t)p.q;
      sb[i] = (uint32_t)(v < 0 ? v + (int64_t)p.q : v);
    }
    __syncthreads();
    uint32_t len = n >> 1;
    for (uint32_t l = 0; l < L; ++l, len >>= 1) {                        // Cooley-Tukey, block b of level l uses zetas[2^l + b]
      for (uint32_t e = threadIdx.x; e < n; e += 256) {
        uint32_t* s = e < n / 2 ? sa : sb;
        const uint32_t bf = e < n / 2 ? e : e - n / 2, blk = bf / len, j = bf - blk * len, lo = blk * 2 * len + j, hi = lo + len;
        const uint32_t t = md.mul(zf[(1u << l) + blk], s[hi]), u = s[lo];
        s[hi] = md.sub(u, t);
        s[lo] = md.add(u, t);
      }
      __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < n; e += 256) {                    // leaf e / d: Z_q[X]/(X^d - gamma), gamma = +-zeta of the last level
      const uint32_t leaf = e / d, c = e - leaf * d;
      const uint32_t z = zf[(1u << (L - 1)) + (leaf >> 1)], gamma = (leaf & 1) ? md.neg(z) : z;
      const uint32_t* pa = sa + leaf * d;
      const uint32_t* pb = sb + leaf * d;
      uint32_t lo = 0, hi = 0;
      for (uint32_t i = 0; i < d; ++i) {
        if (i <= c) lo = md.add(lo, md.mul(pa[i], pb[c - i]));
        else hi = md.add(hi, md.mul(pa[i], pb[d + c - i]));
      }
      sc[e] = md.add(lo, md.mul(gamma, hi));                             // every term times R^-1 (gamma is in Montgomery form)
    }
    __syncthreads();
    len = d;
    for (int l = (int)L - 1; l >= 0; --l, len <<= 1) {                   // Gentleman-Sande
      for (uint32_t e = threadIdx.x; e < n / 2; e += 256) {
        const uint32_t blk = e / len, j = e - blk * len, lo = blk * 2 * len + j, hi = lo + len;
        const uint32_t u = sc[lo], v = sc[hi];
        sc[lo] = md.add(u, v);
        sc[hi] = md.mul(zi[(1u << l) + blk], md.sub(u, v));
      }
      __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) out[pr * n + i] = md.mul(p.fin, sc[i]);
  }
}

struct Plan {
  NttPlan pl;
  NttTables tb;
  uint32_t* d_zetas = nullptr;
  int route = 0;
};
std::mutex g_mu;
std::map<std::tuple<int, uint64_t, size_t, int>, Plan*> g_plans;

// the plan of (device, q, n, ring), built once; nullptr: no NTT for this (q, n)
Plan* plan_for(int device, uint64_t q, size_t n, psf_status* st, NttRing ring = kNegacyclic) {
  *st = PSF_OK;
  std::lock_guard<std::mutex> lk(g_mu);
  const auto key = std::make_tuple(device, q, n, (int)ring);
  auto it = g_plans.find(key);
  if (it != g_plans.end()) return it->second->route ? it->second : nullptr;
  Plan* P = new Plan();
  if (q < (1ull << 31) && n >= 2 && n <= 8192) P->pl = ring == kCyclic ? make_ntt_plan_cyclic(q, (uint32_t)n) : make_ntt_plan(q, (uint32_t)n);
  if (P->pl.ok) {
    P->tb = make_ntt_tables(P->pl);
    P->route = P->tb.wave ? 2 : 1;
    if (device >= 0) {
      if (hipSetDevice(device) != hipSuccess || hipMalloc(&P->d_zetas, P->tb.zetas.size() * sizeof(uint32_t)) != hipSuccess ||
          hipMemcpy(P->d_zetas, P->tb.zetas.data(), P->tb.zetas.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        delete P;
        *st = PSF_ERR_HIP;
        return nullptr;
      }
    }
  }
  g_plans[key] = P;
  return P->route ? P : nullptr;
}

NttDev dev_args(const Plan* P, int e, int e_fa) {
  NttDev a;
  a.q = P->tb.q; a.qinv16 = P->tb.qinv16; a.nqinv32 = P->tb.nqinv32; a.r2 = P->tb.r2;
  a.fin = ntt_final_scale(P->tb, P->pl, e);
  a.fin_fa = ntt_final_scale(P->tb, P->pl, e_fa);
  a.zetas = P->d_zetas;
  return a;
}
NttWavePlan wave_of(const Plan* P) {                                     // a route-2 plan as the launches see it
  return NttWavePlan{P, P->tb.logn, P->tb.ld, P->tb.qb, P->tb.q, (size_t)((P->tb.qb == 12 ? 4u : 2u) << P->pl.L)};
}
unsigned wave_grid(size_t count) {                                       // four products per workgroup at a time, at most 8 workgroups per CU
  static const size_t cap = [] { const char* e = psf_exp_env("PSF_NTT_GRID"); const long v = e ? std::atol(e) : 0; return (size_t)(v > 0 ? v : 2048); }();
  const size_t g = (count + 3) / 4;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace


namespace psf {

psf_status ntt_wave_plan(int device, uint64_t q, size_t n, NttRing ring, int io_bits, NttWavePlan* out) {
  psf_status rc;
  Plan* P = plan_for(device, q, n, &rc, ring);
  if (!P) return rc != PSF_OK ? rc : PSF_ERR_UNSUPPORTED;
  if (P->route != 2 || (io_bits == 16 && P->tb.qb == 0)) return PSF_ERR_UNSUPPORTED;
  *out = wave_of(P);
  return PSF_OK;
}
void ntt_dev_args(const NttWavePlan& w, int e, int e_fa, ntt::NttDev* out) { *out = dev_args(static_cast<const Plan*>(w.plan), e, e_fa); }
unsigned ntt_wave_grid(size_t items) { return wave_grid(items); }

int ntt_route(uint64_t q, size_t n, NttRing ring) {
  psf_status st;
  Plan* P = plan_for(-1, q, n, &st, ring);
  return P ? P->route : 0;
}

psf_status ntt_polymul_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, hipStream_t st,
                           NttRing ring) {
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  if (count && (!d_a || !d_b || !d_out)) return PSF_ERR_PARAM;
  psf_status rc;
  Plan* P = plan_for(device, q, n, &rc, ring);
  if (!P) return rc != PSF_OK ? rc : PSF_ERR_UNSUPPORTED;
  if (count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  if (P->route == 1) {
    if (io_bits != 64) return PSF_ERR_UNSUPPORTED;
    const NttDev a = dev_args(P, 1, 1);
    const size_t smem = ((2u << P->pl.L) + 3 * n) * sizeof(uint32_t);
    if (smem > 160 * 1024) return PSF_ERR_UNSUPPORTED;                   // gfx950: 160 KiB of LDS per workgroup (n = 8192 with a fully splitting prime needs 160 KiB exactly)
    const psf_status rl = raise_lds_once(reinterpret_cast<const void*>(k_ntt_polymul_lds), device, smem);
    if (rl != PSF_OK) return rl;
    hipLaunchKernelGGL(k_ntt_polymul_lds, dim3((unsigned)(count > 4096 ? 4096 : count)), dim3(256), smem, st, a, (uint32_t)n, P->pl.L, P->pl.d,
                       (const uint64_t*)d_a, (const int64_t*)d_b, (uint64_t*)d_out, count);
    HIP_TRY(hipGetLastError());
    return PSF_OK;
  }
  if (io_bits == 16 && P->tb.qb == 0) return PSF_ERR_UNSUPPORTED;
  const NttWavePlan w = wave_of(P);
  return ntt_launch_wave(w, io_bits, [&](auto ln, auto ldv, auto qbv, auto io) {
    hipLaunchKernelGGL((k_ntt_polymul<ln(), ldv(), qbv(), io()>), dim3(wave_grid(count)), dim3(256), 0, st, ntt_product_args<ln(), ldv(), qbv()>(w), d_a, d_b, d_out, count);
  });
}

psf_status ntt_forward_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, int io_bits, uint32_t* d_hat, hipStream_t st, NttRing ring) {
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  if (count && (!d_a || !d_hat)) return PSF_ERR_PARAM;
  NttWavePlan w;
  const psf_status rc = ntt_wave_plan(device, q, n, ring, io_bits, &w);
  if (rc != PSF_OK) return rc;
  if (count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  return ntt_launch_wave(w, io_bits, [&](auto ln, auto ldv, auto qbv, auto io) {
    hipLaunchKernelGGL((k_ntt_forward<ln(), ldv(), qbv(), io(), false>), dim3(wave_grid(count)), dim3(256), 0, st, dev_args(static_cast<const Plan*>(w.plan), 1, 1), d_a, d_hat, count);
  });
}

psf_status ntt_mul_hat_dev(int device, uint64_t q, size_t n, size_t count, const uint32_t* d_hat, size_t hat_stride, const void* d_b, void* d_out, int io_bits, hipStream_t st,
                           NttRing ring) {
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  if (count && (!d_hat || !d_b || !d_out)) return PSF_ERR_PARAM;
  NttWavePlan w;
  const psf_status rc = ntt_wave_plan(device, q, n, ring, io_bits, &w);
  if (rc != PSF_OK) return rc;
  if (count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  return ntt_launch_wave(w, io_bits, [&](auto ln, auto ldv, auto qbv, auto io) {
    hipLaunchKernelGGL((k_ntt_mul_hat<ln(), ldv(), qbv(), io()>), dim3(wave_grid(count)), dim3(256), 0, st, ntt_product_args<ln(), ldv(), qbv()>(w), d_hat, hat_stride, d_b, d_out, count);
  });
}

psf_status ntt_ring_fa_dev(int device, uint64_t q, size_t n, uint32_t K, const uint32_t* d_hat, const int64_t* d_sigma, uint64_t* d_u, size_t B, hipStream_t st) {
  if (B && (!d_hat || !d_sigma || !d_u)) return PSF_ERR_PARAM;
  NttWavePlan w;
  const psf_status rc = ntt_wave_plan(device, q, n, kNegacyclic, 64, &w);
  if (rc != PSF_OK) return rc;
  const size_t smem = (w.zeta_words + (size_t)K * n) * sizeof(uint32_t);
  if (smem > 64 * 1024) return PSF_ERR_UNSUPPORTED;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  return ntt_launch_wave(w, 64, [&](auto ln, auto ldv, auto qbv, auto) {     // 64-bit words only
    hipLaunchKernelGGL((k_ring_fa<ln(), ldv(), qbv()>), dim3(wave_grid(B)), dim3(256), smem, st, ntt_product_args<ln(), ldv(), qbv()>(w), d_hat, K, d_sigma, d_u, B);
  });
}

psf_status ntt_matmul_dev(int device, uint64_t q, size_t n, const NttMatShape& s, const void* d_a, size_t a_stride, bool hat, const void* d_b, void* d_c,
                          int io_bits, hipStream_t st, NttRing ring) {
  return ntt_matpoly_launch<false>(device, q, n, s, d_a, a_stride, hat, d_b, nullptr, 0, d_c, io_bits, st, ring);
}

}  // namespace psf
