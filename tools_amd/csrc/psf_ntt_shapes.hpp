// psf_ntt_shapes.hpp -- the one list of the shapes that have a wave kernel (make_ntt_tables decides logn, ld, qb).  Every unit of wave kernels
// (psf_ntt.hip, psf_ntt_fma.hip) instantiates its kernels over this list.
#pragma once
#include "psf_hip_util.hpp"

namespace psf {

template <class F> bool for_shape(int logn, int ld, int qb, F&& f) {
#define PSF_SHAPE(LN, LDV, QBV) if (logn == LN && ld == LDV && qb == QBV) { f(ic<LN>{}, ic<LDV>{}, ic<QBV>{}); return true; }
  PSF_SHAPE(7, 0, 12) PSF_SHAPE(8, 1, 12) PSF_SHAPE(9, 2, 12)
  PSF_SHAPE(7, 0, 14) PSF_SHAPE(7, 1, 14) PSF_SHAPE(8, 0, 14) PSF_SHAPE(8, 1, 14) PSF_SHAPE(8, 2, 14) PSF_SHAPE(9, 0, 14) PSF_SHAPE(9, 1, 14) PSF_SHAPE(9, 2, 14)
  PSF_SHAPE(10, 0, 14) PSF_SHAPE(10, 1, 14) PSF_SHAPE(10, 2, 14)
  PSF_SHAPE(7, 0, 0) PSF_SHAPE(7, 1, 0) PSF_SHAPE(8, 0, 0) PSF_SHAPE(8, 1, 0) PSF_SHAPE(8, 2, 0) PSF_SHAPE(9, 0, 0) PSF_SHAPE(9, 1, 0) PSF_SHAPE(9, 2, 0)
  PSF_SHAPE(10, 0, 0) PSF_SHAPE(10, 1, 0) PSF_SHAPE(10, 2, 0)
#undef PSF_SHAPE
  return false;
}

}  // namespace psf
