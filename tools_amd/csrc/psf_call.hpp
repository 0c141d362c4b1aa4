// psf_call.hpp -- what the bytes-in, bytes-out units (psf_keccak.hip, psf_mlkem.hip, psf_mldsa.hip, psf_mldsa_sign.hip, psf_slhdsa.hip,
// psf_slhdsa_sign.hip, psf_sha2.hip, psf_slhdsa_sha2.hip, psf_slhdsa_sha2_sign.hip) share around their kernels, and nothing of any one scheme: the argument checks and the workspace layout (psf_call_host.hpp, no HIP
// in it), the grid-limit helpers, and HostCall, the device copies of a call on host buffers.
#pragma once
#include <hip/hip_runtime.h>
#include "psf_call_host.hpp"
#include "psf_hip_util.hpp"

namespace psf {

// ---- launches --------------------------------------------------------------------------------------------------------------------------------------
constexpr unsigned kMaxGrid = 0x7fffffffu;
inline unsigned blocks_of(size_t items, size_t per_block) { return (unsigned)((items + per_block - 1) / per_block); }
// a unit whose every grid has at most one workgroup per instance takes this many instances
inline bool grid_fits(size_t count) { return count <= kMaxGrid; }

// a stage of `lanes` lanes as launches of at most 2^31 - 1 workgroups of 256, args.first moving along
template <class Args> psf_status launch_chunked(void (*kern)(Args), size_t lanes, Args a, hipStream_t st) {
  const size_t blocks = (lanes + 255) / 256;
  for (size_t b0 = 0; b0 < blocks; b0 += kMaxGrid) {
    const size_t nb = blocks - b0 < kMaxGrid ? blocks - b0 : (size_t)kMaxGrid;
    a.first = b0 * 256;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return PSF_OK;
}

// ---- a call on host buffers ------------------------------------------------------------------------------------------------------------------------
// host rows of `len` bytes at `stride` <-> packed device rows
inline hipError_t upload_rows(void* d, const void* h, size_t count, size_t len, size_t stride) {
  if (count == 0 || len == 0) return hipSuccess;
  return stride == len ? hipMemcpy(d, h, count * len, hipMemcpyHostToDevice) : hipMemcpy2D(d, len, h, stride, len, count, hipMemcpyHostToDevice);
}
inline hipError_t download_rows(void* h, const void* d, size_t count, size_t len, size_t stride) {
  if (count == 0 || len == 0) return hipSuccess;
  return stride == len ? hipMemcpy(h, d, count * len, hipMemcpyDeviceToHost) : hipMemcpy2D(h, stride, d, len, len, count, hipMemcpyDeviceToHost);
}

// The device side of one call on host buffers (`device` is current): packed copies of the inputs, the outputs, the workspace and the sampler flag, all
// released when the call returns.  in / out / workspace / flag return device pointers and remember the first failure, which status() reports: one
// PSF_TRY before the run covers them all.  A buffer marked SECRET is zero-filled before its release, on every path out of the call.
enum Secrecy : bool { PUBLIC = false, SECRET = true };
class HostCall {
 public:
  HostCall() = default;
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  ~HostCall() {
    for (int i = 0; i < n_; ++i)
      if (secret_[i]) (void)buf_[i].zero(bytes_[i]);
  }
  // `count` host rows of `len` bytes at `stride` (0: one row for all) as packed device rows; NULL or len = 0: nullptr
  const uint8_t* in(const void* h, size_t count, size_t len, size_t stride, Secrecy s = PUBLIC) {
    const size_t rows = stride ? count : 1;
    if (!h || len == 0) return nullptr;
    uint8_t* d = reserve(rows * len, s);
    if (d) note(upload_rows(d, h, rows, len, stride ? stride : len));
    return d;
  }
  uint8_t* out(size_t bytes, Secrecy s = PUBLIC, bool zeroed = false) {
    uint8_t* d = reserve(bytes, s);
    if (d && zeroed) note(buf_[n_ - 1].zero(bytes));
    return d;
  }
  void* workspace(size_t bytes) {
    if (rc_ == PSF_OK && bytes) note(ws_.alloc(bytes));
    return ws_.as<void>();
  }
  // the flag a sampler raises when its input runs out, cleared
  int* flag() {
    if (rc_ == PSF_OK) note(flag_.alloc(sizeof(int)));
    if (rc_ == PSF_OK) note(flag_.zero(sizeof(int)));
    return flag_.as<int>();
  }
  psf_status status() const { return rc_; }
  // packed device rows to host rows at `stride`; a NULL host pointer (an optional output) is skipped
  psf_status fetch(void* h, const void* d, size_t count, size_t len, size_t stride) {
    if (h) note(download_rows(h, d, count, len, stride));
    return rc_;
  }
  psf_status fetch(void* h, const void* d, size_t bytes) { return fetch(h, d, 1, bytes, bytes); }
  // the end of a call: PSF_ERR_SAMPLER when the flag was asked for and is raised
  psf_status finish() {
    int fl = 0;
    if (flag_.as<int>()) HIP_TRY(flag_.download(&fl, sizeof(int)));
    return fl ? PSF_ERR_SAMPLER : PSF_OK;
  }

 private:
  static constexpr int kBufs = 8;
  void note(hipError_t e) {
    if (e == hipSuccess || rc_ != PSF_OK) return;
    std::fprintf(stderr, "[psf_mi355x] a call on host buffers failed: %s\n", hipGetErrorString(e));
    rc_ = PSF_ERR_HIP;
  }
  uint8_t* reserve(size_t bytes, Secrecy s) {
    if (rc_ != PSF_OK) return nullptr;
    if (n_ == kBufs) { rc_ = PSF_ERR_UNSUPPORTED; return nullptr; }
    note(buf_[n_].alloc(bytes));
    if (rc_ != PSF_OK) return nullptr;
    bytes_[n_] = bytes;
    secret_[n_] = s == SECRET;
    return buf_[n_++].as<uint8_t>();
  }
  DevBuf buf_[kBufs], ws_, flag_;
  size_t bytes_[kBufs] = {};
  bool secret_[kBufs] = {};
  int n_ = 0;
  psf_status rc_ = PSF_OK;
};

}  // namespace psf
