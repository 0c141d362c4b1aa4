// psf_ntt_fma.hip -- the fused R_q matrix products C[c] = E[c] +- op(A[c]) B[c] (psf_matpoly_mul_add_*_dev): the instantiations of k_matpoly_fma
// (psf_ntt_kernels.hpp), in a translation unit of their own so that they compile beside psf_ntt.hip.  The plan cache and the tables on the device stay
// in psf_ntt.hip (psf_ntt_api.hpp); the list of wave shapes (psf_ntt_shapes.hpp) and the launch (psf_ntt_launch.hpp) are the ones of the plain products.
// The cyclic ring comes through the table of zetas, as for every wave kernel.
#include "psf_ntt_launch.hpp"

namespace psf {

psf_status ntt_matfma_dev(int device, uint64_t q, size_t n, const NttMatShape& s, const void* d_a, size_t a_stride, bool hat, const void* d_b, const void* d_e,
                          int sign, void* d_c, int io_bits, hipStream_t st, NttRing ring) {
  return ntt_matpoly_launch<true>(device, q, n, s, d_a, a_stride, hat, d_b, d_e, sign, d_c, io_bits, st, ring);
}

}  // namespace psf
