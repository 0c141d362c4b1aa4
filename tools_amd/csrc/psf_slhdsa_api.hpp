// psf_slhdsa_api.hpp -- what psf_slhdsa.hip (SLH-DSA KeyGen / Verify) offers psf_slhdsa_sign.hip (SLH-DSA signing), as psf_mldsa_api.hpp does for
// ML-DSA: the parameter set of a `param`, the chunked launch of a stage and the upload of strided host rows.  The functions are defined in
// psf_slhdsa.hip; the template lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "psf_hip_util.hpp"
#include "psf_mldsa_api.hpp"
#include "psf_slhdsa_core.hpp"

namespace psf {
namespace slh {

bool set_of(int param, Params* p);
// host rows of `len` bytes at `stride` -> packed device rows
hipError_t upload_rows(void* d, const void* h, size_t count, size_t len, size_t stride);

// a stage of `lanes` lanes as launches of at most 2^31 - 1 workgroups of 256, args.first moving along
template <class Args> psf_status launch_chunked(void (*kern)(Args), size_t lanes, Args a, hipStream_t st) {
  const size_t blocks = (lanes + 255) / 256;
  for (size_t b0 = 0; b0 < blocks; b0 += dsa::kMaxGrid) {
    const size_t nb = blocks - b0 < dsa::kMaxGrid ? blocks - b0 : (size_t)dsa::kMaxGrid;
    a.first = b0 * 256;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return PSF_OK;
}

}  // namespace slh
}  // namespace psf
