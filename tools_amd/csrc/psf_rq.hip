// psf_rq.hip -- the R_q products behind the C ABI of include/psf_mi355x.h: psf_poly_mul_*, psf_ntt_forward_*, psf_matpoly_mul* over Z_q[X]/(X^n + 1) and
// Z_q[X]/(X^n - 1).  Argument checks, the host-buffer forms and the choice of route: the NTT kernels of psf_ntt.hip / psf_ntt_fma.hip (psf_ntt_api.hpp)
// when (q, n) has them, the exact schoolbook kernels of psf_rq_kernels.hpp otherwise.  No handle: the PSF types reach these products through
// psf_ntt_api.hpp or the public entries.
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_ntt_api.hpp"
#include "psf_rq_kernels.hpp"

using namespace psf;

// one R_q product kernel launch on device buffers: the NTT when (q, n) has one, the exact schoolbook kernel otherwise (64-bit layout only)
// method: 0 = schoolbook kernel, 1 = NTT (PSF_ERR_UNSUPPORTED without a plan), -1 = NTT when there is one
static psf_status polymul_dev_any(int device, uint64_t q, size_t n, size_t count, const void* da, const void* db, void* dout, int io_bits, int method, hipStream_t st,
                                  NttRing ring) {
  if (method != 0) {
    const psf_status rc = ntt_polymul_dev(device, q, n, count, da, db, dout, io_bits, st, ring);
    if (rc != PSF_ERR_UNSUPPORTED || method == 1) return rc;
  }
  if (io_bits != 64) return PSF_ERR_UNSUPPORTED;
  if (count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const uint64_t two64 = (uint64_t)((((u128)1) << 64) % q);
  const size_t smem = 2 * n * sizeof(uint64_t);                          // n > 4096: above the default LDS limit
  const psf_status rl = raise_lds_once(ring == kCyclic ? reinterpret_cast<const void*>(k_polymul_cyclic) : reinterpret_cast<const void*>(k_polymul_negacyclic), device, smem);
  if (rl != PSF_OK) return rl;
  if (ring == kCyclic)
    hipLaunchKernelGGL(k_polymul_cyclic, dim3((unsigned)(count < 65536 ? count : 65536)), dim3(256), smem, st, q, two64, (uint32_t)n, count, (const uint64_t*)da,
                       (const int64_t*)db, (uint64_t*)dout);
  else
    hipLaunchKernelGGL(k_polymul_negacyclic, dim3((unsigned)count), dim3(256), smem, st, q, two64, (uint32_t)n, (const uint64_t*)da, n, (const int64_t*)db, n,
                       (uint64_t*)dout, n);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// the pair products on device buffers: every argument checked before the first HIP call
static psf_status poly_mul_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, void* stream, NttRing ring) {
  if (q <= 1 || q >= (1ull << 62) || n < 1 || n > 8192 || (io_bits != 16 && io_bits != 64) || (count && (!d_a || !d_b || !d_out))) return PSF_ERR_PARAM;
  return polymul_dev_any(device, q, n, count, d_a, d_b, d_out, io_bits, -1, (hipStream_t)stream, ring);
}

static psf_status poly_mul_host(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out, int method, NttRing ring) {
  if (q <= 1 || q >= (1ull << 62) || n < 1 || n > 8192 || (count && (!a || !b || !out))) return PSF_ERR_PARAM;
  if (method == 1 && ntt_route(q, n, ring) == 0) return PSF_ERR_UNSUPPORTED;
  if (count == 0) return PSF_OK;
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  const size_t bytes = count * n * sizeof(uint64_t);                 // of a, of b and of the product alike
  DevBuf da, db, dout;
  HIP_TRY(da.alloc(bytes));
  HIP_TRY(db.alloc(bytes));
  HIP_TRY(dout.alloc(bytes));
  HIP_TRY(da.upload(a, bytes));
  HIP_TRY(db.upload(b, bytes));
  const psf_status rc = polymul_dev_any(device, q, n, count, da.as<void>(), db.as<void>(), dout.as<void>(), 64, method, nullptr, ring);
  if (rc != PSF_OK) return rc;
  HIP_TRY(dout.download(out, bytes));
  return PSF_OK;
}

// ---- R_q matrix products (MatPolynomialRingZq * MatPolynomialRingZq: gpv_ring.rs:245, gadget_ring.rs:78 and :190-202, short_basis_ring.rs:183-198) ----
// Every argument is checked here, before the first HIP call (the plan cache of psf_ntt.hip allocates on the device, so it comes after).  hat: A given
// by its images.
static constexpr size_t kMatpolyMaxInner = (size_t)1 << 20;
// The addend E of the fused forms C = E + sign * op(A) B (psf_matpoly_mul_add_*): laid out like C, in B's word type; sign is +1 or -1.
struct MatAddend { const void* d_e; int sign; };
// add = nullptr: a plain product.  Otherwise E is checked with the rest: not NULL, and either E == C exactly (in place) or no byte in common with C.
static psf_status matpoly_check(uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride, bool hat,
                                int trans_a, const void* d_b, const void* d_c, int io_bits, NttRing ring, const MatAddend* add) {
  if (q <= 1 || q >= (1ull << 62) || n < 1 || n > 8192) return PSF_ERR_PARAM;
  if (rows == 0 || inner == 0 || cols == 0 || (trans_a != 0 && trans_a != 1) || (io_bits != 16 && io_bits != 64)) return PSF_ERR_PARAM;
  if (add && add->sign != 1 && add->sign != -1) return PSF_ERR_PARAM;
  if (count && (!d_a || !d_b || !d_c || (add && !add->d_e))) return PSF_ERR_PARAM;
  // byte ranges of A (all batches), B and C; any product that overflows size_t is a malformed call
  const size_t w = io_bits / 8, wa = hat ? sizeof(uint32_t) : w;
  size_t ri, ic, rc, a_one, a_all = 0, b_all, c_all;
  if (__builtin_mul_overflow(rows, inner, &ri) || __builtin_mul_overflow(inner, cols, &ic) || __builtin_mul_overflow(rows, cols, &rc) ||
      __builtin_mul_overflow(ri, n, &a_one) || __builtin_mul_overflow(ic, n, &ic) || __builtin_mul_overflow(rc, n, &rc) ||
      __builtin_mul_overflow(ic, count, &b_all) || __builtin_mul_overflow(b_all, w, &b_all) || __builtin_mul_overflow(rc, count, &c_all) ||
      __builtin_mul_overflow(c_all, w, &c_all) || __builtin_mul_overflow(a_one, wa, &a_one))
    return PSF_ERR_PARAM;
  if (count) {                                              // A: the last batch starts (count - 1) * a_stride polynomials (hat: words) in
    size_t off;
    if (__builtin_mul_overflow(count - 1, a_stride, &off) || __builtin_mul_overflow(off, hat ? sizeof(uint32_t) : w * n, &off) ||
        __builtin_add_overflow(off, a_one, &a_all))
      return PSF_ERR_PARAM;
    const uintptr_t a0 = (uintptr_t)d_a, b0 = (uintptr_t)d_b, c0 = (uintptr_t)d_c;
    if (a0 + a_all < a0 || b0 + b_all < b0 || c0 + c_all < c0) return PSF_ERR_PARAM;
    if ((c0 < a0 + a_all && a0 < c0 + c_all) || (c0 < b0 + b_all && b0 < c0 + c_all)) return PSF_ERR_PARAM;   // the output overlaps an input
    if (add) {                                              // E: c_all bytes; on top of C exactly, or apart from it
      const uintptr_t e0 = (uintptr_t)add->d_e;
      if (e0 + c_all < e0) return PSF_ERR_PARAM;
      if (e0 != c0 && c0 < e0 + c_all && e0 < c0 + c_all) return PSF_ERR_PARAM;
    }
  }
  if (inner > kMatpolyMaxInner) return PSF_ERR_UNSUPPORTED;
  const int route = ntt_route(q, n, ring);                  // host tables only (device -1): no HIP call
  if ((hat || io_bits == 16) && route != 2) return PSF_ERR_UNSUPPORTED;
  if (io_bits == 16 && q >= (1ull << 14)) return PSF_ERR_UNSUPPORTED;     // 16-bit words: the wave kernels of q < 2^14
  return PSF_OK;
}

// C[c] = op(A[c]) B[c], or with an addend C[c] = E[c] + sign * op(A[c]) B[c], on device buffers: the wave kernels of psf_ntt.hip / psf_ntt_fma.hip when
// (q, n) has them, the schoolbook kernels (with the same epilogue) for every other q < 2^62 at 64-bit words
static psf_status matpoly_dev_any(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                  bool hat, int trans_a, const void* d_b, const MatAddend* add, void* d_c, int io_bits, hipStream_t st, NttRing ring) {
  const psf_status chk = matpoly_check(q, n, count, rows, inner, cols, d_a, a_stride, hat, trans_a, d_b, d_c, io_bits, ring, add);
  if (chk != PSF_OK || count == 0) return chk;
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  if (ntt_route(q, n, ring) == 2) {
    const NttMatShape s{count, rows, inner, cols, trans_a};
    return add ? ntt_matfma_dev(device, q, n, s, d_a, a_stride, hat, d_b, add->d_e, add->sign, d_c, io_bits, st, ring)
               : ntt_matmul_dev(device, q, n, s, d_a, a_stride, hat, d_b, d_c, io_bits, st, ring);
  }
  const uint64_t two64 = (uint64_t)((((u128)1) << 64) % q);
  const size_t outs = count * rows * cols, smem = 2 * n * sizeof(uint64_t);
  const dim3 grid((unsigned)(outs < 16384 ? outs : 16384));
  auto launch = [&](auto kern, auto... addend) -> psf_status {    // the kernel's own arguments for E and sign, if any, sit in front of the output
    const psf_status rl = raise_lds_once(reinterpret_cast<const void*>(kern), device, smem);      // n > 4096: above the default LDS limit
    if (rl != PSF_OK) return rl;
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, st, q, two64, (uint32_t)n, count, rows, inner, cols, (const uint64_t*)d_a, a_stride, trans_a,
                       (const int64_t*)d_b, addend..., (uint64_t*)d_c);
    HIP_TRY(hipGetLastError());
    return PSF_OK;
  };
  if (add) return launch(ring == kCyclic ? k_matpoly_fma_cyclic : k_matpoly_fma_negacyclic, (const int64_t*)add->d_e, add->sign);
  return launch(ring == kCyclic ? k_matpoly_cyclic : k_matpoly_negacyclic);
}

// host buffers, one batch: the same checks on them, then device copies.  With an addend c = e + sign * a b, and c == e (in place) is allowed like
// d_e == d_c: E goes into C's buffer and the device call runs in place.
static psf_status matpoly_host(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, const MatAddend* add,
                               uint64_t* c, NttRing ring) {
  const psf_status chk = matpoly_check(q, n, 1, rows, inner, cols, a, 0, false, 0, b, c, 64, ring, add);
  if (chk != PSF_OK) return chk;
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  const size_t na = rows * inner * n * sizeof(uint64_t), nb = inner * cols * n * sizeof(int64_t), nc = rows * cols * n * sizeof(uint64_t);
  DevBuf da, db, dc;
  HIP_TRY(da.alloc(na));
  HIP_TRY(db.alloc(nb));
  HIP_TRY(dc.alloc(nc));
  HIP_TRY(da.upload(a, na));
  HIP_TRY(db.upload(b, nb));
  if (add) HIP_TRY(dc.upload(add->d_e, nc));
  const MatAddend in_place{dc.as<void>(), add ? add->sign : 0};
  const psf_status rc = matpoly_dev_any(device, q, n, 1, rows, inner, cols, da.as<void>(), 0, false, 0, db.as<void>(), add ? &in_place : nullptr, dc.as<void>(), 64,
                                        nullptr, ring);
  if (rc != PSF_OK) return rc;
  HIP_TRY(dc.download(c, nc));
  return PSF_OK;
}

extern "C" {

psf_status psf_poly_mul_negacyclic_method(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out, int method) {
  return poly_mul_host(device, q, n, count, a, b, out, method, kNegacyclic);
}
psf_status psf_poly_mul_negacyclic(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out) {
  return poly_mul_host(device, q, n, count, a, b, out, -1, kNegacyclic);
}
psf_status psf_poly_mul_negacyclic_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, void* stream) {
  return poly_mul_dev(device, q, n, count, d_a, d_b, d_out, io_bits, stream, kNegacyclic);
}
psf_status psf_ntt_forward_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, int io_bits, uint32_t* d_hat, void* stream) {
  return ntt_forward_dev(device, q, n, count, d_a, io_bits, d_hat, (hipStream_t)stream);
}
psf_status psf_poly_mul_hat_dev(int device, uint64_t q, size_t n, size_t count, const uint32_t* d_hat, size_t hat_stride, const void* d_b, void* d_out, int io_bits,
                                void* stream) {
  return ntt_mul_hat_dev(device, q, n, count, d_hat, hat_stride, d_b, d_out, io_bits, (hipStream_t)stream);
}

// the cyclic ring Z_q[X]/(X^n - 1) (common_moduli.rs:72-79): the same checks, codes and routes with the cyclic tables or the cyclic schoolbook kernel
psf_status psf_poly_mul_cyclic_method(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out, int method) {
  return poly_mul_host(device, q, n, count, a, b, out, method, kCyclic);
}
psf_status psf_poly_mul_cyclic(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out) {
  return poly_mul_host(device, q, n, count, a, b, out, -1, kCyclic);
}
psf_status psf_poly_mul_cyclic_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, void* stream) {
  return poly_mul_dev(device, q, n, count, d_a, d_b, d_out, io_bits, stream, kCyclic);
}
psf_status psf_ntt_forward_cyclic_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, int io_bits, uint32_t* d_hat, void* stream) {
  return ntt_forward_dev(device, q, n, count, d_a, io_bits, d_hat, (hipStream_t)stream, kCyclic);
}
psf_status psf_poly_mul_hat_cyclic_dev(int device, uint64_t q, size_t n, size_t count, const uint32_t* d_hat, size_t hat_stride, const void* d_b, void* d_out,
                                       int io_bits, void* stream) {
  return ntt_mul_hat_dev(device, q, n, count, d_hat, hat_stride, d_b, d_out, io_bits, (hipStream_t)stream, kCyclic);
}

psf_status psf_matpoly_mul_negacyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                          int trans_a, const void* d_b, void* d_c, int io_bits, void* stream) {
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_a, a_stride, false, trans_a, d_b, nullptr, d_c, io_bits, (hipStream_t)stream, kNegacyclic);
}
psf_status psf_matpoly_mul_hat_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat, size_t hat_stride,
                                   int trans_a, const void* d_b, void* d_c, int io_bits, void* stream) {
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_hat, hat_stride, true, trans_a, d_b, nullptr, d_c, io_bits, (hipStream_t)stream, kNegacyclic);
}
psf_status psf_matpoly_mul_negacyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, uint64_t* c) {
  return matpoly_host(device, q, n, rows, inner, cols, a, b, nullptr, c, kNegacyclic);
}
psf_status psf_matpoly_mul_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                      int trans_a, const void* d_b, void* d_c, int io_bits, void* stream) {
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_a, a_stride, false, trans_a, d_b, nullptr, d_c, io_bits, (hipStream_t)stream, kCyclic);
}
psf_status psf_matpoly_mul_hat_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat,
                                          size_t hat_stride, int trans_a, const void* d_b, void* d_c, int io_bits, void* stream) {
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_hat, hat_stride, true, trans_a, d_b, nullptr, d_c, io_bits, (hipStream_t)stream, kCyclic);
}
psf_status psf_matpoly_mul_cyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, uint64_t* c) {
  return matpoly_host(device, q, n, rows, inner, cols, a, b, nullptr, c, kCyclic);
}

// the fused forms C = E + sign * op(A) B
psf_status psf_matpoly_mul_add_negacyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                              int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream) {
  const MatAddend add{d_e, sign};
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_a, a_stride, false, trans_a, d_b, &add, d_c, io_bits, (hipStream_t)stream, kNegacyclic);
}
psf_status psf_matpoly_mul_add_hat_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat, size_t hat_stride,
                                       int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream) {
  const MatAddend add{d_e, sign};
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_hat, hat_stride, true, trans_a, d_b, &add, d_c, io_bits, (hipStream_t)stream, kNegacyclic);
}
psf_status psf_matpoly_mul_add_negacyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, const int64_t* e,
                                          int sign, uint64_t* c) {
  const MatAddend add{e, sign};
  return matpoly_host(device, q, n, rows, inner, cols, a, b, &add, c, kNegacyclic);
}
psf_status psf_matpoly_mul_add_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                          int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream) {
  const MatAddend add{d_e, sign};
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_a, a_stride, false, trans_a, d_b, &add, d_c, io_bits, (hipStream_t)stream, kCyclic);
}
psf_status psf_matpoly_mul_add_hat_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat,
                                              size_t hat_stride, int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream) {
  const MatAddend add{d_e, sign};
  return matpoly_dev_any(device, q, n, count, rows, inner, cols, d_hat, hat_stride, true, trans_a, d_b, &add, d_c, io_bits, (hipStream_t)stream, kCyclic);
}
psf_status psf_matpoly_mul_add_cyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, const int64_t* e,
                                      int sign, uint64_t* c) {
  const MatAddend add{e, sign};
  return matpoly_host(device, q, n, rows, inner, cols, a, b, &add, c, kCyclic);
}

}  // extern "C"
