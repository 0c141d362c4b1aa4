// psf_rq_kernels.hpp -- the exact schoolbook kernels of the R_q products (psf_rq.hip): polynomial and matrix products over Z_q[X]/(X^n + 1) and
// Z_q[X]/(X^n - 1) for every q < 2^62, with and without the fused addend.  They serve every (q, n) that has no NTT; the NTT forms of the same products
// (one transform per wavefront, Montgomery arithmetic) are in psf_ntt_kernels.hpp / psf_ntt.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "psf_acc128.hpp"

namespace psf {

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

}  // namespace psf
