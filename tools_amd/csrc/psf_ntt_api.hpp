// psf_ntt_api.hpp -- what psf_ntt.hip and psf_ntt_fma.hip (the translation units of the NTT kernels) offer the rest of the library: psf_rq.hip (the
// C ABI of the R_q products) and the ring PSF of psfgpv_impl.hpp.  Device pointers, the caller's stream, no allocation per call: the tables of a
// (device, q, n) are built at first use and kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/psf_mi355x.h"

namespace psf {

// The ring of a product: Z_q[X]/(X^n + 1) (common_moduli.rs:41-48) or Z_q[X]/(X^n - 1) (:72-79).  Both run the same kernels: only the table of zetas
// differs (make_ntt_plan / make_ntt_plan_cyclic, psf_host.hpp), and a (q, n) has a plan, a route and a shape in one ring exactly when it has them in the other.
enum NttRing : int { kNegacyclic = 0, kCyclic = 1 };

// 0: (q, n) has no negacyclic NTT (q not a prime with 4 | q - 1, q >= 2^31, n not a power of two); 1: the generic LDS kernel; 2: one transform per wave
int ntt_route(uint64_t q, size_t n, NttRing ring = kNegacyclic);
// out = a * b mod (X^n + 1, q), `count` products.  io_bits 64: a uint64 (any value), b int64 (any value), out uint64 in [0, q) -- the layout of
// psf_poly_mul_negacyclic; io_bits 16 (route 2, q < 2^14): a uint16 in [0, q), b int16 in (-q, q), out uint16.
psf_status ntt_polymul_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, hipStream_t st,
                           NttRing ring = kNegacyclic);
// route 2 only.  hat: count * n words, the register image of the leaf residues (opaque: only ntt_mul_hat_dev / ntt_ring_fa_dev / ntt_matmul_dev of the
// same ring read it)
psf_status ntt_forward_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, int io_bits, uint32_t* d_hat, hipStream_t st,
                           NttRing ring = kNegacyclic);
// out = a * b with a given by its image; hat_stride in words between the images of consecutive products (0: one image for all)
psf_status ntt_mul_hat_dev(int device, uint64_t q, size_t n, size_t count, const uint32_t* d_hat, size_t hat_stride, const void* d_b, void* d_out, int io_bits, hipStream_t st,
                           NttRing ring = kNegacyclic);
// u_b = sum_{j < K} a_j * sigma_{b,j}: sigma B rows of K*n int64, u B rows of n uint64 (PSFGPVRing::f_a, gpv_ring.rs:243-247); X^n + 1 only
psf_status ntt_ring_fa_dev(int device, uint64_t q, size_t n, uint32_t K, const uint32_t* d_hat, const int64_t* d_sigma, uint64_t* d_u, size_t B, hipStream_t st);

// C[c] = op(A[c]) B[c] over R_q for `count` batches of matrices of polynomials (psf_matpoly_mul_*_dev; arguments checked by the caller), route 2 only:
// hat = false: A as polynomials in the io_bits layout of a, a_stride in polynomials; hat = true: A as images, a_stride in words.  0: one A for all.
struct NttMatShape { size_t count, rows, inner, cols; int trans_a; };
psf_status ntt_matmul_dev(int device, uint64_t q, size_t n, const NttMatShape& s, const void* d_a, size_t a_stride, bool hat, const void* d_b, void* d_c,
                          int io_bits, hipStream_t st, NttRing ring = kNegacyclic);

// C[c] = E[c] + sign * op(A[c]) B[c] (psf_matpoly_mul_add_*_dev; arguments checked by the caller, sign = +1 or -1): ntt_matmul_dev with the epilogue of
// k_matpoly_fma.  E in the io_bits layout and value contract of B; d_e == d_c is the one overlap allowed.  Defined in psf_ntt_fma.hip.
psf_status ntt_matfma_dev(int device, uint64_t q, size_t n, const NttMatShape& s, const void* d_a, size_t a_stride, bool hat, const void* d_b, const void* d_e,
                          int sign, void* d_c, int io_bits, hipStream_t st, NttRing ring = kNegacyclic);

// ---- what another translation unit of wave kernels needs from psf_ntt.hip: the cached plan of (device, q, n, ring) and the launch conventions ----------
namespace ntt { struct NttDev; }
struct NttWavePlan {
  const void* plan;          // the cache entry (owned by psf_ntt.hip)
  int logn, ld, qb;          // the wave shape (for_shape, psf_ntt_shapes.hpp)
  uint32_t q;
  size_t zeta_words;         // words of LDS the zetas of this shape take in front of anything else
};
// PSF_ERR_UNSUPPORTED unless (q, n) has a wave kernel that reads io_bits words; PSF_ERR_HIP when the tables cannot be placed on the device
psf_status ntt_wave_plan(int device, uint64_t q, size_t n, NttRing ring, int io_bits, NttWavePlan* out);
// the kernel argument of the plan for a product that carries e (e_fa: one more) factors R^-1 (Kern::E)
void ntt_dev_args(const NttWavePlan& w, int e, int e_fa, ntt::NttDev* out);
// workgroups of 256 threads for `items` wave-sized work items
unsigned ntt_wave_grid(size_t items);

}  // namespace psf
