// psf_ntt_launch.hpp -- how a unit of wave kernels (psf_ntt.hip, psf_ntt_fma.hip) launches them: the dispatch of a plan's shape and of the call's word
// width to template arguments, and on top of it the launch of the R_q matrix products, written once for k_matpoly_mul and k_matpoly_fma.  Each unit
// instantiates only its own kernels from here.
#pragma once
#include "psf_hip_util.hpp"
#include "psf_ntt_api.hpp"
#include "psf_ntt_kernels.hpp"
#include "psf_ntt_shapes.hpp"

namespace psf {

// launch(ic<LN>, ic<LDV>, ic<QBV>, ic<IO>) for the shape of the plan and the words of the call (16 bits only where the shape has a 16-bit Montgomery form;
// ntt_wave_plan has refused the others), then the status of the launch
template <class F> psf_status ntt_launch_wave(const NttWavePlan& w, int io_bits, F&& launch) {
  const bool ok = for_shape(w.logn, w.ld, w.qb, [&](auto ln, auto ldv, auto qbv) {
    if constexpr (decltype(qbv)::value != 0) {
      if (io_bits == 16) { launch(ln, ldv, qbv, ic<16>{}); return; }
    }
    launch(ln, ldv, qbv, ic<64>{});
  });
  if (!ok) return PSF_ERR_UNSUPPORTED;                      // a wave plan without an instantiated shape: nothing was launched
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
// the kernel argument of the plan for the products of shape (LN, LDV, QBV)
template <int LN, int LDV, int QBV> ntt::NttDev ntt_product_args(const NttWavePlan& w) {
  ntt::NttDev a;
  ntt_dev_args(w, ntt::Kern<LN, LDV, QBV>::E, ntt::Kern<LN, LDV, QBV>::E + 1, &a);
  return a;
}

// ntt_matmul_dev (FUSED = false: k_matpoly_mul; d_e and sign unused) and ntt_matfma_dev (FUSED = true: k_matpoly_fma)
template <bool FUSED>
psf_status ntt_matpoly_launch(int device, uint64_t q, size_t n, const NttMatShape& s, const void* d_a, size_t a_stride, bool hat, const void* d_b, const void* d_e,
                              int sign, void* d_c, int io_bits, hipStream_t st, NttRing ring) {
  NttWavePlan w;
  const psf_status rc = ntt_wave_plan(device, q, n, ring, io_bits, &w);
  if (rc != PSF_OK) return rc;
  const bool stage = hat && a_stride == 0 && (w.zeta_words + s.rows * s.inner * n) * sizeof(uint32_t) <= 64 * 1024;   // one A for all: its images in LDS
  if (s.count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  return ntt_launch_wave(w, io_bits, [&](auto ln, auto ldv, auto qbv, auto io) {
    constexpr int LN = decltype(ln)::value, LDV = decltype(ldv)::value, QBV = decltype(qbv)::value, IO = decltype(io)::value;
    const ntt::NttDev a = ntt_product_args<LN, LDV, QBV>(w);
    const ntt::MatArgs m = ntt::make_mat_args(s.count, s.rows, s.inner, s.cols, s.trans_a, a_stride, ntt::MatTile<LN>::RT, w.q);
    const size_t smem = (w.zeta_words + (stage ? s.rows * s.inner * n : 0)) * sizeof(uint32_t);
    const dim3 grid(ntt_wave_grid(m.items));
    auto go = [&](auto form) {                              // A as polynomials, as images in global memory, as images in LDS
      constexpr int HAT = decltype(form)::value;
      if constexpr (FUSED) hipLaunchKernelGGL((ntt::k_matpoly_fma<LN, LDV, QBV, IO, HAT>), grid, dim3(256), smem, st, a, m, d_a, d_b, d_e, sign, d_c);
      else hipLaunchKernelGGL((ntt::k_matpoly_mul<LN, LDV, QBV, IO, HAT>), grid, dim3(256), smem, st, a, m, d_a, d_b, d_c);
    };
    if (!hat) go(ic<0>{});
    else if (!stage) go(ic<1>{});
    else go(ic<2>{});
  });
}

}  // namespace psf
