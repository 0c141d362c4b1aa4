// psf_sha2.hip -- batched SHA-256 and SHA-512 (FIPS 180-4) on the device, the twin of psf_keccak_dev: `count` independent messages of one length, one
// hash state per LANE (psf_sha2_core.hpp: state and schedule in registers, rounds unrolled, no LDS, no cross-lane traffic), the leading out_len bytes of
// every digest out -- FIPS 205's Trunc.  It is what the SHA-2 parameter sets of SLH-DSA (psf_slhdsa_sha2.hip) are measured against: a one-block message
// costs one compression and the padding block's.
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_sha2_core.hpp"

namespace psf {
namespace sha2 {

struct HashArgs {
  size_t first, count, in_len, in_stride, out_len, out_stride;
  int in_aligned;                // base and stride multiples of 4: every 4-byte group of a message is one load
  const uint8_t* in;
  uint8_t* out;
};

template <int FUNC> __global__ __launch_bounds__(256) void k_sha2(HashArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const PtrReader rd{a.in + c * a.in_stride, a.in_aligned != 0};
  if constexpr (FUNC == PSF_SHA2_256) {
    uint32_t h[8];
    init256(h);
    absorb256<DevOps>(h, rd, a.in_len, 0);
    put_digest256(h, a.out + c * a.out_stride, a.out_len);
  } else {
    uint64_t h[8];
    init512(h);
    absorb512<DevOps>(h, rd, a.in_len, 0);
    put_digest512(h, a.out + c * a.out_stride, a.out_len);
  }
}

// the header's order: func, out_len, strides, NULL pointers, byte counts, overlaps
psf_status check_sha2(int func, size_t count, const uint8_t* in, size_t in_len, size_t in_stride, const uint8_t* out, size_t out_len, size_t out_stride) {
  if (func != PSF_SHA2_256 && func != PSF_SHA2_512) return PSF_ERR_PARAM;
  if (out_len == 0 || out_len > (func == PSF_SHA2_256 ? 32u : 64u)) return PSF_ERR_PARAM;
  if (in_stride < in_len || out_stride < out_len) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  Buf b[2] = {{in, in_len, in_stride, false, in_len == 0, 0}, {out, out_len, out_stride, true, false, 0}};
  PSF_TRY(check_null(b, 2));
  if (in_len > SIZE_MAX / 8 - 128) return PSF_ERR_PARAM;                    // the bit length of the padding
  return check_rest(count, b, 2, Layout{}, false, nullptr, 0);
}

psf_status sha2_launch(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len,
                       size_t out_stride, hipStream_t st) {
  PSF_TRY(use_device(device));
  const HashArgs a{0, count, in_len, in_stride, out_len, out_stride, ((uintptr_t)d_in | in_stride) % 4 == 0, d_in, d_out};
  return launch_chunked(func == PSF_SHA2_256 ? k_sha2<PSF_SHA2_256> : k_sha2<PSF_SHA2_512>, count, a, st);
}

}  // namespace sha2
}  // namespace psf

using namespace psf;

extern "C" {

psf_status psf_sha2_dev(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len,
                        size_t out_stride, void* stream) {
  const psf_status rc = sha2::check_sha2(func, count, d_in, in_len, in_stride, d_out, out_len, out_stride);
  if (rc != PSF_OK || count == 0) return rc;
  return sha2::sha2_launch(device, func, count, d_in, in_len, in_stride, d_out, out_len, out_stride, (hipStream_t)stream);
}

psf_status psf_sha2(int device, int func, size_t count, const uint8_t* in, size_t in_len, size_t in_stride, uint8_t* out, size_t out_len, size_t out_stride) {
  const psf_status rc = sha2::check_sha2(func, count, in, in_len, in_stride, out, out_len, out_stride);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  HostCall h;                                                              // packed rows on the device
  const uint8_t* din = h.in(in, count, in_len, in_stride);
  uint8_t* dout = h.out(count * out_len);
  PSF_TRY(h.status());
  PSF_TRY(sha2::sha2_launch(device, func, count, din, in_len, in_len, dout, out_len, out_len, nullptr));
  return h.fetch(out, dout, count, out_len, out_stride);
}

}  // extern "C"
