// psf_ntt_fma.hip -- the fused R_q matrix products C[c] = E[c] +- op(A[c]) B[c] (psf_matpoly_mul_add_*_dev): the instantiations of k_matpoly_fma
// (psf_ntt_kernels.hpp) and their launch, in a translation unit of their own so that they compile beside psf_ntt.hip.  The plan cache, the tables on
// the device and the launch conventions stay in psf_ntt.hip (psf_ntt_api.hpp); the list of wave shapes is for_shape of psf_ntt.hip, included here
// without the rest of that file.  The cyclic ring comes through the table of zetas, as for every wave kernel.
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_ntt_api.hpp"
#include "psf_ntt_kernels.hpp"
#define PSF_NTT_SHAPES_ONLY
#include "psf_ntt.hip"
#undef PSF_NTT_SHAPES_ONLY

namespace psf {

psf_status ntt_matfma_dev(int device, uint64_t q, size_t n, const NttMatShape& s, const void* d_a, size_t a_stride, bool hat, const void* d_b, const void* d_e,
                          int sign, void* d_c, int io_bits, hipStream_t st, NttRing ring) {
  NttWavePlan w;
  const psf_status rc = ntt_wave_plan(device, q, n, ring, io_bits, &w);
  if (rc != PSF_OK) return rc;
  const bool stage = hat && a_stride == 0 && (w.zeta_words + s.rows * s.inner * n) * sizeof(uint32_t) <= 64 * 1024;   // one A for all: its images in LDS
  if (s.count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const bool ok = for_shape(w.logn, w.ld, w.qb, [&](auto ln, auto ldv, auto qbv) {
    constexpr int LN = decltype(ln)::value, LDV = decltype(ldv)::value, QBV = decltype(qbv)::value;
    NttDev a;
    ntt_dev_args(w, Kern<LN, LDV, QBV>::E, Kern<LN, LDV, QBV>::E + 1, &a);
    const MatArgs m = make_mat_args(s.count, s.rows, s.inner, s.cols, s.trans_a, a_stride, MatTile<LN>::RT, w.q);
    const size_t smem = (w.zeta_words + (stage ? s.rows * s.inner * n : 0)) * sizeof(uint32_t);
    const dim3 grid(ntt_wave_grid(m.items));
    auto go = [&](auto io) {
      constexpr int IO = decltype(io)::value;
      if (!hat) hipLaunchKernelGGL((k_matpoly_fma<LN, LDV, QBV, IO, 0>), grid, dim3(256), smem, st, a, m, d_a, d_b, d_e, sign, d_c);
      else if (!stage) hipLaunchKernelGGL((k_matpoly_fma<LN, LDV, QBV, IO, 1>), grid, dim3(256), smem, st, a, m, d_a, d_b, d_e, sign, d_c);
      else hipLaunchKernelGGL((k_matpoly_fma<LN, LDV, QBV, IO, 2>), grid, dim3(256), smem, st, a, m, d_a, d_b, d_e, sign, d_c);
    };
    if constexpr (QBV != 0) {
      if (io_bits == 16) { go(ic<16>{}); return; }
    }
    go(ic<64>{});
  });
  if (!ok) return PSF_ERR_UNSUPPORTED;                      // a wave plan without an instantiated shape: nothing was launched
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

}  // namespace psf
