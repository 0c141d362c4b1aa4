// psf_gpv_kernels.hpp -- HIP kernels of PSFGPV / PSFGPVRing (gpv.rs, gpv_ring.rs): short-basis assembly and Gram-Schmidt.
// The batched randomized nearest plane itself is in psf_np_kernels.hpp; the R_q products of the ring variant are a unit of
// their own (psf_rq.hip, psf_rq_kernels.hpp).
//
// Layout: the short basis and its Gram-Schmidt vectors are stored TRANSPOSED -- row i is basis vector i (column i of the
// reference's matrices).
#pragma once
#include "psf_kernels.hpp"

namespace psf {

// ---- [0 I; S' W] transposed: row c = column c of the bottom block [S' | W] (short_basis_classical.rs:77-110) ----------
// rows 0..w-1: columns of S' = I_n (x) S_k, column order reversed iff base^k == q (:80-82)
// rows w..m-1: columns of W, W[jk+t][c] = t-th digit of -A[j][c] mod q (:105-110, tag = identity)
__global__ void k_gpv_bottom_t(const uint64_t* __restrict__ A, size_t lda, uint32_t n, uint32_t k, size_t mbar, size_t w, uint64_t q,
                               uint64_t base, const int32_t* __restrict__ Sk, int reversed, int8_t* __restrict__ BT, size_t ldw) {
  const size_t m = mbar + w, total = m * ldw;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g / ldw, t = g % ldw;
    int32_t v = 0;
    if (t < w) {
      const uint32_t blk = (uint32_t)(t / k), tt = (uint32_t)(t % k);
      if (i < w) {
        const size_t src = reversed ? (w - 1 - i) : i;
        if (src / k == blk) v = Sk[tt * k + (uint32_t)(src % k)];
      } else {
        const uint64_t a = A[(size_t)blk * lda + (i - w)] % q;
        uint64_t x = a ? q - a : 0;
        for (uint32_t d = 0; d < tt; ++d) x /= base;
        v = (int32_t)(x % base);
      }
    }
    BT[g] = (int8_t)v;
  }
}

// S_A^t = [ (R S')^t ; (I + R W)^t | bottom^t ]:  St[i][r] = sum_t BT[i][t] R[r][t] + [i >= w and i - w == r]  (r < mbar),
// St[i][mbar + t] = BT[i][t].  64 x 64 tiles, four coordinates per v_dot4_i32_i8.
__global__ __launch_bounds__(256) void k_gpv_basis_t(const int8_t* __restrict__ BT, size_t ldw, const int8_t* __restrict__ R, size_t ldr,
                                                     size_t m, size_t mbar, size_t w, int32_t* __restrict__ St) {
  __shared__ uint32_t sB[64][17];
  __shared__ uint32_t sR[64][17];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const size_t i0 = (size_t)blockIdx.y * 64, r0 = (size_t)blockIdx.x * 64;
  int32_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0;
  const uint32_t* B32 = reinterpret_cast<const uint32_t*>(BT);
  const uint32_t* R32 = reinterpret_cast<const uint32_t*>(R);
  const size_t w4 = (w + 3) / 4;
  for (size_t q0 = 0; q0 < w4; q0 += 16) {
    for (int e = tid; e < 64 * 16; e += 256) {
      const int rr = e >> 4, qq = e & 15;
      uint32_t vb = 0, vr = 0;
      if (q0 + qq < w4) {
        if (i0 + rr < m) vb = B32[(i0 + rr) * (ldw / 4) + q0 + qq];
        if (r0 + rr < mbar) vr = R32[(r0 + rr) * (ldr / 4) + q0 + qq];
      }
      sB[rr][qq] = vb; sR[rr][qq] = vr;
    }
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < 16; ++qq) {
      uint32_t rv[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) rv[b] = sR[tx * 4 + b][qq];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const uint32_t bv = sB[ty * 4 + a][qq];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_sdot4((int)bv, (int)rv[b], acc[a][b], false);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const size_t i = i0 + ty * 4 + a, r = r0 + tx * 4 + b;
      if (i < m && r < mbar) St[i * m + r] = acc[a][b] + ((i >= w && i - w == r) ? 1 : 0);
    }
}
__global__ void k_gpv_basis_t_tail(const int8_t* __restrict__ BT, size_t ldw, size_t m, size_t mbar, size_t w, int32_t* __restrict__ St) {
  const size_t total = m * w;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g / w, t = g % w;
    St[i * m + mbar + t] = BT[i * ldw + t];
  }
}

// ---- Gram-Schmidt (MatQ::gso, gpv.rs:91) on the rows of St: the blocked, re-orthogonalised form lives in psf_gemm_kernels.hpp (gso_blocked);
// here only the conversion of the basis to doubles and the contract's norms.
__global__ void k_i32_to_f64(const int32_t* __restrict__ s, double* __restrict__ d, size_t total) {
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) d[g] = (double)s[g];
}
// ||b~_i||^2 as the contract's ascending fma chain (one thread per row; setup only)
__global__ void k_row_norm2_chain(const double* __restrict__ Gt, size_t m, double* __restrict__ norm2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double acc = 0.0;
  for (size_t j = 0; j < m; ++j) acc = fma(Gt[i * m + j], Gt[i * m + j], acc);
  norm2[i] = acc;
}

}  // namespace psf
