// psf_ntt_matpoly_body.hpp -- the body of k_matpoly_mul and of k_matpoly_fma (psf_ntt_kernels.hpp), included once in each with PSF_MATPOLY_FMA defined
// as 0 or 1: text, not a function, so that the product kernel compiles to the code it had before the fused form existed (a shared device function
// changes its register allocation).  No include guard.  In scope: the template parameters LOGN, LD, QB, IO, HAT and the kernel arguments p, m, A, B,
// out (PSF_MATPOLY_FMA = 1: E, sign and out through MatFmaKernArgs).
// PSF_MATPOLY_FMA = 1: out = E + sign * product, sign = +1 or -1 (wave-uniform).  The lane that holds a coefficient x in [0, q) after `finish` reads
// the matching word e of E the way operand b is read (load<IO, true>: an int16 in (-q, q), or an int64 of any value reduced here), forms e + x or
// e + (q - x) and brings it to [0, q) with conditional corrections (Kern::add_signed): no transform, no LDS, no barrier.  E may BE out (in place):
// every word of E is read by the lane that then writes that word of out, and by no other.
  using KN = Kern<LOGN, LD, QB>;
  using V = typename KN::V;
  constexpr int C = KN::C, RT = MatTile<LOGN>::RT;
  extern __shared__ __attribute__((aligned(16))) uint32_t mm_smem[];   // zetas [ZN] (| images [rows * inner][C][64] when HAT = 2)
  uint32_t* zt = mm_smem;
  const uint32_t* ah = mm_smem + KN::ZN;
  if constexpr (HAT == 2) {
    const size_t words = m.rows * m.inner * (size_t)KN::N;
    for (size_t i = threadIdx.x; i < words; i += blockDim.x) mm_smem[KN::ZN + i] = reinterpret_cast<const uint32_t*>(A)[i];
  }
  KN::load_tables(zt, p);
  const auto md = make_policy<QB>(p, KN::L);
  const int lane = DevWave::lane();
  const size_t waves = (size_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t* zf = zt;
  const uint32_t* zi = zt + (1 << KN::L);
  for (size_t it = (size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block(); it < m.items; it += waves) {
    const size_t tile = it % m.tiles, cj = it / m.tiles, j = cj % m.cols, c = cj / m.cols, i0 = tile * RT;
    const int nr = (int)(m.rows - i0 < (size_t)RT ? m.rows - i0 : (size_t)RT);
    V acc[RT][C];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < C; ++r) acc[t][r] = 0;
    int since = 0;
    const size_t dia = m.trans_a ? 1 : m.inner;                         // A[i][k] -> A[i + 1][k] in storage order
    for (size_t k = 0; k < m.inner; ++k) {
      V b[C];
      KN::template load<IO, true>(b, B, (c * m.inner + k) * m.cols + j, lane, md, p);
      KN::K::forward(b, md, zf, lane);
      const size_t ia0 = m.trans_a ? k * m.rows + i0 : i0 * m.inner + k;
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        if (t < nr) {
          const size_t ia = ia0 + t * dia;
          V a[C], pr[C];
          if constexpr (HAT == 0) {
            KN::template load<IO, false>(a, A, c * m.a_stride + ia, lane, md, p);
            KN::K::forward(a, md, zf, lane);
          } else if constexpr (HAT == 1) {
            const uint32_t* h = reinterpret_cast<const uint32_t*>(A) + c * m.a_stride + ia * KN::N;
#pragma unroll
            for (int r = 0; r < C; ++r) a[r] = (V)h[r * 64 + lane];
          } else {
#pragma unroll
            for (int r = 0; r < C; ++r) a[r] = (V)ah[ia * KN::N + r * 64 + lane];
          }
          KN::K::leafmul(pr, a, b, md, zf, lane);
          KN::K::acc_add(acc[t], pr, md);
        }
      }
      KN::K::acc_tick(acc, md, (V)m.r1, since);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      if (t < nr) {
        KN::K::acc_close(acc[t], md);
        KN::K::inverse(acc[t], md, zi, lane);
        KN::K::finish(acc[t], md, (V)(QB != 0 ? p.fin_fa : p.fin));
#if PSF_MATPOLY_FMA
        {
          // E, sign and out are read from the kernel-argument segment HERE, per output polynomial (three scalar loads), not held in scalar registers
          // across the item: the product kernel of <8, 2, 0, 64, 1> already takes 99 of the 100 there are, and five more would spill.  The empty
          // asm statement keeps the loads from being hoisted back out of the loop.
          const MatFmaKernArgs __attribute__((address_space(4)))* ka = (const MatFmaKernArgs __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
          asm volatile("" : "+s"(ka));
          V e[C];
          KN::template load_addend<IO>(e, ka->E, (c * m.rows + i0 + t) * m.cols + j, lane, md, p);
          KN::add_signed(acc[t], e, ka->sign, p);
          KN::template store<IO>(acc[t], ka->out, (c * m.rows + i0 + t) * m.cols + j, lane);
        }
#else
        KN::template store<IO>(acc[t], out, (c * m.rows + i0 + t) * m.cols + j, lane);
#endif
      }
    }
  }
