// psf_gpv_kernels.hpp -- HIP kernels of PSFGPV / PSFGPVRing (gpv.rs, gpv_ring.rs): short-basis assembly, Gram-Schmidt,
// and the R_q products of the ring variant.  The batched randomized nearest plane itself is in psf_np_kernels.hpp.
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

// ---- modular product shared by the polynomial kernels below ------------------------------------------------------------------
__device__ inline uint64_t mulmod_dev(uint64_t a, uint64_t b, uint64_t q) {
  if (q <= 0xffffffffull) return (a * b) % q;
  uint64_t r = 0;
  while (b) {
    if (b & 1) { r += a; if (r >= q) r -= q; }
    a += a; if (a >= q) a -= q;
    b >>= 1;
  }
  return r;
}

// ---- R_q = Z_q[X]/(X^n + 1): negacyclic product (PolynomialRingZq multiplication under gadget_ring.rs:78 and gpv_ring.rs:245-246) ----
// One workgroup per pair; both operands in LDS; thread t owns coefficients t, t+256, ...  out[c] = sum_{i<=c} a_i b_{c-i} - sum_{i>c} a_i b_{n+c-i}.
// Exact: positive and negative parts are accumulated in 128 bits (q < 2^31) or reduced term by term (larger q).
__global__ __launch_bounds__(256) void k_polymul_negacyclic(uint64_t q, uint64_t two64, uint32_t n, const uint64_t* __restrict__ A, size_t a_stride,
                                                            const int64_t* __restrict__ Bp, size_t b_stride, uint64_t* __restrict__ out, size_t o_stride) {
  extern __shared__ __attribute__((aligned(16))) uint64_t pm_smem[];   // a[n] | b[n]
  uint64_t* sa = pm_smem;
  uint64_t* sb = pm_smem + n;
  const size_t pair = blockIdx.x;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    sa[i] = A[pair * a_stride + i] % q;
    const int64_t v = Bp[pair * b_stride + i] % (int64_t)q;
    sb[i] = (uint64_t)(v < 0 ? v + (int64_t)q : v);
  }
  __syncthreads();
  const bool small = q <= 0x7fffffffull;
  for (uint32_t c = threadIdx.x; c < n; c += 256) {
    uint64_t pos = 0, neg = 0;
    if (small) {
      Acc128 P{0, 0}, N{0, 0};
      for (uint32_t i = 0; i <= c; ++i) acc128_add(P, (int64_t)(sa[i] * sb[c - i]));
      for (uint32_t i = c + 1; i < n; ++i) acc128_add(N, (int64_t)(sa[i] * sb[n + c - i]));
      pos = acc128_mod(P, q, two64);
      neg = acc128_mod(N, q, two64);
    } else {
      for (uint32_t i = 0; i <= c; ++i) { pos += mulmod_dev(sa[i], sb[c - i], q); if (pos >= q) pos -= q; }
      for (uint32_t i = c + 1; i < n; ++i) { neg += mulmod_dev(sa[i], sb[n + c - i], q); if (neg >= q) neg -= q; }
    }
    out[pair * o_stride + c] = pos >= neg ? pos - neg : pos + q - neg;
  }
}

// ---- R_q matrix product C[c] = op(A[c]) B[c] (MatPolynomialRingZq * MatPolynomialRingZq) for every q < 2^62 without a wave NTT ---------------------
// A[c]: rows x inner polynomials at A + c * a_stride polynomials (trans_a: stored inner x rows), B[c]: inner x cols, C[c]: rows x cols.  One workgroup
// per output polynomial (c, i, j) at a time; per 256-coefficient chunk of it and per k < inner, A[c][i][k] and B[c][k][j] are staged in LDS (reduced mod
// q) and thread t adds the terms of coefficient chunk + t.  Exact: for q < 2^31 the positive and negative parts are summed over all of `inner` in
// 128 bits (inner n < 2^33 terms below 2^62) and reduced once; above, every term is reduced.
// FMA (psf_matpoly_mul_add_*_dev): out = E + sign * product, sign = +1 or -1.  The thread that holds coefficient x in [0, q) reads the matching int64 e
// of E (any value, reduced to [0, q)), forms e + x or e + (q - x) < 2q < 2^63 and subtracts q once if needed.  E may be out: the word is read by the
// thread that then writes it.
template <bool FMA> __device__ __forceinline__ uint64_t matpoly_epilogue(uint64_t x, uint64_t q, const int64_t* E, size_t idx, int sign) {
  if constexpr (!FMA) return x;
  else {
    const int64_t v = E[idx] % (int64_t)q;
    const uint64_t e = (uint64_t)(v < 0 ? v + (int64_t)q : v), s = e + (sign < 0 ? q - x : x);
    return s >= q ? s - q : s;
  }
}
template <bool FMA>
__device__ __forceinline__ void matpoly_negacyclic_body(uint64_t q, uint64_t two64, uint32_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint64_t* A,
                                                        size_t a_stride, int trans_a, const int64_t* Bp, const int64_t* E, int sign, uint64_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t mp_smem[];   // a[n] | b[n]
  uint64_t* sa = mp_smem;
  uint64_t* sb = mp_smem + n;
  const bool small = q <= 0x7fffffffull;
  const size_t outs = count * rows * cols;
  for (size_t o = blockIdx.x; o < outs; o += gridDim.x) {
    const size_t j = o % cols, ci = o / cols, i = ci % rows, c = ci / rows;
    for (uint32_t c0 = 0; c0 < n; c0 += 256) {
      const uint32_t cc = c0 + threadIdx.x;
      Acc128 P{0, 0}, N{0, 0};
      uint64_t pos = 0, neg = 0;
      for (size_t k = 0; k < inner; ++k) {
        const uint64_t* pa = A + (c * a_stride + (trans_a ? k * rows + i : i * inner + k)) * n;
        const int64_t* pb = Bp + ((c * inner + k) * cols + j) * n;
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < n; t += 256) {
          sa[t] = pa[t] % q;
          const int64_t v = pb[t] % (int64_t)q;
          sb[t] = (uint64_t)(v < 0 ? v + (int64_t)q : v);
        }
        __syncthreads();
        if (cc >= n) continue;
        if (small) {
          for (uint32_t t = 0; t <= cc; ++t) acc128_add(P, (int64_t)(sa[t] * sb[cc - t]));
          for (uint32_t t = cc + 1; t < n; ++t) acc128_add(N, (int64_t)(sa[t] * sb[n + cc - t]));
        } else {
          for (uint32_t t = 0; t <= cc; ++t) { pos += mulmod_dev(sa[t], sb[cc - t], q); if (pos >= q) pos -= q; }
          for (uint32_t t = cc + 1; t < n; ++t) { neg += mulmod_dev(sa[t], sb[n + cc - t], q); if (neg >= q) neg -= q; }
        }
      }
      if (cc >= n) continue;
      if (small) { pos = acc128_mod(P, q, two64); neg = acc128_mod(N, q, two64); }
      out[o * n + cc] = matpoly_epilogue<FMA>(pos >= neg ? pos - neg : pos + q - neg, q, E, o * n + cc, sign);
    }
  }
}
__global__ __launch_bounds__(256) void k_matpoly_negacyclic(uint64_t q, uint64_t two64, uint32_t n, size_t count, size_t rows, size_t inner, size_t cols,
                                                            const uint64_t* __restrict__ A, size_t a_stride, int trans_a, const int64_t* __restrict__ Bp,
                                                            uint64_t* __restrict__ out) {
  matpoly_negacyclic_body<false>(q, two64, n, count, rows, inner, cols, A, a_stride, trans_a, Bp, nullptr, 1, out);
}
// E and out without __restrict__: they may be the same buffer
__global__ __launch_bounds__(256) void k_matpoly_fma_negacyclic(uint64_t q, uint64_t two64, uint32_t n, size_t count, size_t rows, size_t inner, size_t cols,
                                                                const uint64_t* __restrict__ A, size_t a_stride, int trans_a, const int64_t* __restrict__ Bp,
                                                                const int64_t* E, int sign, uint64_t* out) {
  matpoly_negacyclic_body<true>(q, two64, n, count, rows, inner, cols, A, a_stride, trans_a, Bp, E, sign, out);
}

// ---- the cyclic ring Z_q[X]/(X^n - 1) (common_moduli.rs:72-79): the same two products for every q < 2^62 without an NTT ------------------------------
// The layouts and the work split of k_polymul_negacyclic / k_matpoly_negacyclic; the wrapped terms are ADDED, so out[c] = sum_i a_i b_{(c - i) mod n}
// is one non-negative sum: in 128 bits for q < 2^31 (at most 2^13 * 2^20 terms below 2^62; acc128_mod takes any high word), reduced term by term above.
__global__ __launch_bounds__(256) void k_polymul_cyclic(uint64_t q, uint64_t two64, uint32_t n, size_t count, const uint64_t* __restrict__ A,
                                                        const int64_t* __restrict__ Bp, uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t pc_smem[];   // a[n] | b[n]
  uint64_t* sa = pc_smem;
  uint64_t* sb = pc_smem + n;
  const bool small = q <= 0x7fffffffull;
  for (size_t pair = blockIdx.x; pair < count; pair += gridDim.x) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
      sa[i] = A[pair * n + i] % q;
      const int64_t v = Bp[pair * n + i] % (int64_t)q;
      sb[i] = (uint64_t)(v < 0 ? v + (int64_t)q : v);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < n; c += 256) {
      uint64_t sum = 0;
      if (small) {
        Acc128 S{0, 0};
        for (uint32_t i = 0; i <= c; ++i) acc128_add(S, (int64_t)(sa[i] * sb[c - i]));
        for (uint32_t i = c + 1; i < n; ++i) acc128_add(S, (int64_t)(sa[i] * sb[n + c - i]));
        sum = acc128_mod(S, q, two64);
      } else {
        for (uint32_t i = 0; i <= c; ++i) { sum += mulmod_dev(sa[i], sb[c - i], q); if (sum >= q) sum -= q; }
        for (uint32_t i = c + 1; i < n; ++i) { sum += mulmod_dev(sa[i], sb[n + c - i], q); if (sum >= q) sum -= q; }
      }
      out[pair * n + c] = sum;
    }
  }
}

template <bool FMA>
__device__ __forceinline__ void matpoly_cyclic_body(uint64_t q, uint64_t two64, uint32_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint64_t* A,
                                                    size_t a_stride, int trans_a, const int64_t* Bp, const int64_t* E, int sign, uint64_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t mc_smem[];   // a[n] | b[n]
  uint64_t* sa = mc_smem;
  uint64_t* sb = mc_smem + n;
  const bool small = q <= 0x7fffffffull;
  const size_t outs = count * rows * cols;
  for (size_t o = blockIdx.x; o < outs; o += gridDim.x) {
    const size_t j = o % cols, ci = o / cols, i = ci % rows, c = ci / rows;
    for (uint32_t c0 = 0; c0 < n; c0 += 256) {
      const uint32_t cc = c0 + threadIdx.x;
      Acc128 S{0, 0};
      uint64_t sum = 0;
      for (size_t k = 0; k < inner; ++k) {
        const uint64_t* pa = A + (c * a_stride + (trans_a ? k * rows + i : i * inner + k)) * n;
        const int64_t* pb = Bp + ((c * inner + k) * cols + j) * n;
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < n; t += 256) {
          sa[t] = pa[t] % q;
          const int64_t v = pb[t] % (int64_t)q;
          sb[t] = (uint64_t)(v < 0 ? v + (int64_t)q : v);
        }
        __syncthreads();
        if (cc >= n) continue;
        if (small) {
          for (uint32_t t = 0; t <= cc; ++t) acc128_add(S, (int64_t)(sa[t] * sb[cc - t]));
          for (uint32_t t = cc + 1; t < n; ++t) acc128_add(S, (int64_t)(sa[t] * sb[n + cc - t]));
        } else {
          for (uint32_t t = 0; t <= cc; ++t) { sum += mulmod_dev(sa[t], sb[cc - t], q); if (sum >= q) sum -= q; }
          for (uint32_t t = cc + 1; t < n; ++t) { sum += mulmod_dev(sa[t], sb[n + cc - t], q); if (sum >= q) sum -= q; }
        }
      }
      if (cc >= n) continue;
      out[o * n + cc] = matpoly_epilogue<FMA>(small ? acc128_mod(S, q, two64) : sum, q, E, o * n + cc, sign);
    }
  }
}
__global__ __launch_bounds__(256) void k_matpoly_cyclic(uint64_t q, uint64_t two64, uint32_t n, size_t count, size_t rows, size_t inner, size_t cols,
                                                        const uint64_t* __restrict__ A, size_t a_stride, int trans_a, const int64_t* __restrict__ Bp,
                                                        uint64_t* __restrict__ out) {
  matpoly_cyclic_body<false>(q, two64, n, count, rows, inner, cols, A, a_stride, trans_a, Bp, nullptr, 1, out);
}
__global__ __launch_bounds__(256) void k_matpoly_fma_cyclic(uint64_t q, uint64_t two64, uint32_t n, size_t count, size_t rows, size_t inner, size_t cols,
                                                            const uint64_t* __restrict__ A, size_t a_stride, int trans_a, const int64_t* __restrict__ Bp,
                                                            const int64_t* E, int sign, uint64_t* out) {
  matpoly_cyclic_body<true>(q, two64, n, count, rows, inner, cols, A, a_stride, trans_a, Bp, E, sign, out);
}

// The NTT forms of these products (one transform per wavefront, Montgomery arithmetic) are in psf_ntt_kernels.hpp / psf_ntt.hip.

}  // namespace psf
