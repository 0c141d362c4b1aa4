// psf_keccak.hip -- what makes the R_q arithmetic of the library speak FIPS 203 byte for byte: batched SHA3-256 / SHA3-512 / SHAKE128 / SHAKE256
// (the functions G, H, J, PRF and XOF), SampleNTT (Algorithm 7) and SamplePolyCBD(PRF(sigma, N)) (Algorithm 8) on the device, and the conversion
// between FIPS 203's NTT-domain representation and the images of psf_ntt_forward_dev at (3329, 256).
// One Keccak state per LANE (psf_keccak_core.hpp): `count` independent messages, 25 lanes of 64 bits in registers, no LDS for the state and no
// cross-lane traffic.  Every loop is bounded (message blocks, digest blocks, at most 8 blocks of SampleNTT) and no kernel waits on another workgroup.
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_stream_host.hpp"
#include "psf_host.hpp"
#include "psf_keccak_core.hpp"
#include "psf_ntt_fips.hpp"

namespace psf {
namespace kc {

// ---- hashes ----------------------------------------------------------------------------------------------------------------------------------
struct HashArgs {
  size_t count, in_len, in_stride, out_len, out_stride;
  uint32_t dom;
  int in_aligned, out_aligned;   // base and stride multiples of 8: every 8-byte group of a message / digest is one load / store
};

template <int RATE> __global__ __launch_bounds__(256) void k_keccak(HashArgs a, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  hash<RATE, DevOps>(PtrReader{in + c * a.in_stride, a.in_aligned != 0}, a.in_len, a.dom, PtrWriter{out + c * a.out_stride, a.out_aligned != 0}, a.out_len);
}

// ---- samplers --------------------------------------------------------------------------------------------------------------------------------
// One polynomial per lane, 64 consecutive polynomials per workgroup of ONE wave.  A lane parks its coefficients in LDS as 16-bit words at
// [coefficient][lane] (a row is 64 lanes + 2 words: 33 dwords, so the write of one coefficient by 64 lanes and the read of 64 coefficients of one
// polynomial are both conflict free); then the wave writes the 64 polynomials out one after the other, coefficient lane + 64 k by lane `lane`:
// every store instruction covers 128 (16-bit words) or 512 (64-bit words) consecutive bytes.  33 KiB of LDS per wave: 4 waves per compute unit, one
// per SIMD -- the permutation has 25 independent lanes of work per round, and the sampler is bound by its issue, not by latency.
// A lane past the end of the batch repeats the last polynomial (so that the wave vote of the parse loop sees 64 live lanes) and is not written.
constexpr int kPitch = 66;                                                // (indices below 2^24: 24-bit multiplies, full rate)
constexpr int kSampLds = 256 * kPitch;

template <int IO> __device__ __forceinline__ void emit_wave(const uint16_t* lds, void* __restrict__ out, size_t p0, size_t total, uint32_t lane) {
  const size_t left = total - p0;
  const uint32_t np = left < 64 ? (uint32_t)left : 64u;
  for (uint32_t p = 0; p < np; ++p) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t j = lane + 64 * k;
      const int16_t v = (int16_t)lds[j * kPitch + p];
      const size_t at = (p0 + p) * 256 + j;
      if constexpr (IO == 16) static_cast<int16_t*>(out)[at] = v;
      else static_cast<int64_t*>(out)[at] = (int64_t)v;                  // residues are below 2^15: the sign extension of a CBD value leaves them alone
    }
  }
}

struct NttSampArgs { size_t total, seed_stride; uint32_t k; };

template <int IO> __global__ __launch_bounds__(64) void k_sample_ntt(NttSampArgs a, const uint8_t* __restrict__ seed, void* __restrict__ out, int* __restrict__ fail) {
  __shared__ uint16_t lds[kSampLds];
  const uint32_t lane = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * 64;
  const size_t p = p0 + lane < a.total ? p0 + lane : a.total - 1;
  SeedReader rd;
  if (a.k == 0) rd = SeedReader{seed + p * a.seed_stride, 34, 0};
  else {                                                                 // polynomial (c, i, j): rho_c || j || i
    const uint32_t kk = a.k * a.k;
    const size_t c = p / kk;
    const uint32_t r = (uint32_t)(p - c * kk), i = r / a.k, j = r - i * a.k;
    rd = SeedReader{seed + c * a.seed_stride, 32, j | (i << 8)};
  }
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = 0;
  absorb<kRateShake128, DevOps>(s, rd, 34, kDomShake);
  const bool f = sample_ntt_parse<DevOps>(s, [&](uint32_t j, uint32_t v) { lds[__umul24(j, kPitch) + lane] = (uint16_t)v; }, kSampleNttMaxBlocks);
  if (f && fail) atomicOr(fail, 1);
  __syncthreads();
  emit_wave<IO>(lds, out, p0, a.total, lane);
}

struct CbdSampArgs { size_t total, sigma_stride; uint32_t per_seed, first_nonce; };

template <int ETA, int IO> __global__ __launch_bounds__(64) void k_sample_cbd(CbdSampArgs a, const uint8_t* __restrict__ sigma, void* __restrict__ out) {
  __shared__ uint16_t lds[kSampLds];
  const uint32_t lane = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * 64;
  const size_t p = p0 + lane < a.total ? p0 + lane : a.total - 1;
  const size_t c = p / a.per_seed;
  const uint32_t t = (uint32_t)(p - c * a.per_seed);
  uint64_t w[8 * ETA];
  prf_words<ETA, DevOps>(SeedReader{sigma + c * a.sigma_stride, 32, a.first_nonce + t}, w);
  cbd_fields<ETA>(w, [&](uint32_t j, int v) { lds[__umul24(j, kPitch) + lane] = (uint16_t)(int16_t)v; });
  __syncthreads();
  emit_wave<IO>(lds, out, p0, a.total, lane);
}

// ---- NTT images --------------------------------------------------------------------------------------------------------------------------------
// One thread per written word of a polynomial, the read a gather inside the polynomial through the 256-entry table in the kernel arguments
// (psf_ntt_fips.hpp); a thread keeps its table entry while its workgroup walks the polynomials blockIdx, blockIdx + gridDim, ...
struct ImgArgs { uint8_t src[256]; int32_t q, qinv16, scale; };

template <int IO> __global__ __launch_bounds__(256) void k_image_from(ImgArgs m, const void* __restrict__ fhat, uint32_t* __restrict__ hat, size_t count) {
  const uint32_t w = threadIdx.x, src = m.src[w];
  for (size_t c = blockIdx.x; c < count; c += gridDim.x) {
    uint32_t v;
    if constexpr (IO == 16) v = static_cast<const uint16_t*>(fhat)[c * 256 + src];
    else v = (uint32_t)(static_cast<const uint64_t*>(fhat)[c * 256 + src] % kQ);
    hat[c * 256 + w] = ntt::fips_word_from(v, m.q, m.qinv16, m.scale);
  }
}
template <int IO> __global__ __launch_bounds__(256) void k_image_to(ImgArgs m, const uint32_t* __restrict__ hat, void* __restrict__ fhat, size_t count) {
  const uint32_t k = threadIdx.x, src = m.src[k];
  for (size_t c = blockIdx.x; c < count; c += gridDim.x) {
    const uint32_t v = ntt::fips_word_to(hat[c * 256 + src], m.q, m.qinv16, m.scale);
    if constexpr (IO == 16) static_cast<uint16_t*>(fhat)[c * 256 + k] = (uint16_t)v;
    else static_cast<uint64_t*>(fhat)[c * 256 + k] = v;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// the pointer, stride, overflow and overlap rules every entry point shares: input items (in may be NULL when in_len = 0), output items
psf_status check_io(size_t count, const void* in, size_t in_len, size_t in_stride, const void* out, size_t out_len, size_t out_stride, size_t* in_span,
                    size_t* out_span) {
  if (in_stride < in_len || out_stride < out_len) return PSF_ERR_PARAM;
  if (count && (!out || (!in && in_len))) return PSF_ERR_PARAM;
  if (!span_of(in, count, in_len, in_stride, in_span) || !span_of(out, count, out_len, out_stride, out_span)) return PSF_ERR_PARAM;
  if (overlap(in, *in_span, out, *out_span)) return PSF_ERR_PARAM;
  return PSF_OK;
}

struct FuncSpec { int rate; uint32_t dom; size_t fixed_out; };
bool func_spec(int func, FuncSpec* f) {
  switch (func) {
    case PSF_SHA3_256: *f = {kRateSha3_256, kDomSha3, 32}; return true;
    case PSF_SHA3_512: *f = {kRateSha3_512, kDomSha3, 64}; return true;
    case PSF_SHAKE128: *f = {kRateShake128, kDomShake, 0}; return true;
    case PSF_SHAKE256: *f = {kRateShake256, kDomShake, 0}; return true;
  }
  return false;
}
psf_status check_keccak(int func, size_t count, const uint8_t* in, size_t in_len, size_t in_stride, const uint8_t* out, size_t out_len, size_t out_stride,
                        FuncSpec* f, size_t* in_span, size_t* out_span) {
  if (!func_spec(func, f)) return PSF_ERR_PARAM;
  if (f->fixed_out && out_len != f->fixed_out) return PSF_ERR_PARAM;
  if (out_len == 0) return PSF_ERR_PARAM;
  return check_io(count, in, in_len, in_stride, out, out_len, out_stride, in_span, out_span);
}

psf_status keccak_launch(int device, const FuncSpec& f, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len,
                         size_t out_stride, hipStream_t st) {
  const size_t blocks = (count + 255) / 256;
  if (blocks > kMaxGrid) return PSF_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(device));
  HashArgs a{count, in_len, in_stride, out_len, out_stride, f.dom, ((uintptr_t)d_in | in_stride) % 8 == 0, ((uintptr_t)d_out | out_stride) % 8 == 0};
  for_int<kRateSha3_512, kRateShake256, kRateShake128>(f.rate, [&](auto rate) {
    hipLaunchKernelGGL((k_keccak<decltype(rate)::value>), dim3((unsigned)blocks), dim3(256), 0, st, a, d_in, d_out);
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// SampleNTT: the seed length by form, the number of polynomials, the checks
psf_status check_sample_ntt(size_t count, uint32_t k, const uint8_t* seed, size_t seed_stride, const void* out, int io_bits, size_t* total, size_t* seed_span) {
  if (k > 16) return PSF_ERR_PARAM;
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  const size_t per = k ? (size_t)k * k : 1, poly = (size_t)kN * ((size_t)io_bits / 8);
  if (count > SIZE_MAX / per / poly) return PSF_ERR_PARAM;
  *total = count * per;
  size_t out_span = 0;
  return check_io(count, seed, k ? 32 : 34, seed_stride, out, per * poly, per * poly, seed_span, &out_span);
}
psf_status sample_ntt_launch(int device, size_t total, uint32_t k, const uint8_t* d_seed, size_t seed_stride, void* d_out, int* d_fail, int io_bits, hipStream_t st) {
  const size_t blocks = (total + 63) / 64;
  if (blocks > kMaxGrid) return PSF_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(device));
  const NttSampArgs a{total, seed_stride, k};
  for_int<16, 64>(io_bits, [&](auto io) {
    hipLaunchKernelGGL((k_sample_ntt<decltype(io)::value>), dim3((unsigned)blocks), dim3(64), 0, st, a, d_seed, d_out, d_fail);
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

psf_status check_sample_cbd(size_t count, uint32_t eta, const uint8_t* sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed, const void* out,
                            int io_bits, size_t* total, size_t* sigma_span) {
  if (eta == 0) return PSF_ERR_PARAM;
  if (first_nonce > 256 || per_seed > 256 - first_nonce) return PSF_ERR_PARAM;
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  const size_t poly = (size_t)kN * ((size_t)io_bits / 8), row = (size_t)per_seed * poly;
  if (row && count > SIZE_MAX / row) return PSF_ERR_PARAM;
  *total = count * per_seed;
  size_t out_span = 0;
  const psf_status rc = check_io(count, sigma, 32, sigma_stride, out, row, row, sigma_span, &out_span);
  if (rc != PSF_OK) return rc;
  return eta == 2 || eta == 3 ? PSF_OK : PSF_ERR_UNSUPPORTED;
}
psf_status sample_cbd_launch(int device, size_t total, uint32_t eta, const uint8_t* d_sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed,
                             void* d_out, int io_bits, hipStream_t st) {
  const size_t blocks = (total + 63) / 64;
  if (blocks > kMaxGrid) return PSF_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(device));
  const CbdSampArgs a{total, sigma_stride, per_seed, first_nonce};
  for_int<2, 3>((int)eta, [&](auto e) {
    for_int<16, 64>(io_bits, [&](auto io) {
      hipLaunchKernelGGL((k_sample_cbd<decltype(e)::value, decltype(io)::value>), dim3((unsigned)blocks), dim3(64), 0, st, a, d_sigma, d_out);
    });
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

const ntt::FipsImageMap& image_map() {
  static const ntt::FipsImageMap m = make_fips203_image_map();
  return m;
}
// from = true: fhat (io_bits words) -> hat; false: hat -> fhat
psf_status image_call(int device, size_t count, const void* d_fhat, int io_bits, const uint32_t* d_hat, bool from, hipStream_t st) {
  if (io_bits != 16 && io_bits != 64) return PSF_ERR_PARAM;
  if (count && (!d_fhat || !d_hat)) return PSF_ERR_PARAM;
  const size_t wb = (size_t)io_bits / 8;
  if (count > SIZE_MAX / (kN * 8)) return PSF_ERR_PARAM;
  if (overlap(d_fhat, count * kN * wb, d_hat, count * kN * 4)) return PSF_ERR_PARAM;
  const ntt::FipsImageMap& m = image_map();
  if (!m.ok) return PSF_ERR_UNSUPPORTED;
  if (count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const unsigned blocks = (unsigned)(count < (size_t)cus * 8 ? count : (size_t)cus * 8);      // 8 workgroups of 256 lanes per CU
  ImgArgs a;
  for (int i = 0; i < 256; ++i) a.src[i] = from ? m.fips_of[i] : m.word_of[i];
  a.q = m.q;
  a.qinv16 = m.qinv16;
  a.scale = from ? m.c_from : m.c_to;
  for_int<16, 64>(io_bits, [&](auto io) {
    constexpr int IO = decltype(io)::value;
    if (from) hipLaunchKernelGGL((k_image_from<IO>), dim3(blocks), dim3(256), 0, st, a, d_fhat, const_cast<uint32_t*>(d_hat), count);
    else hipLaunchKernelGGL((k_image_to<IO>), dim3(blocks), dim3(256), 0, st, a, d_hat, const_cast<void*>(d_fhat), count);
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status image_host(int device, size_t count, const void* fhat, const uint32_t* hat, bool from) {
  if (count && (!fhat || !hat)) return PSF_ERR_PARAM;
  if (count > SIZE_MAX / (kN * 8)) return PSF_ERR_PARAM;
  if (overlap(fhat, count * kN * 8, hat, count * kN * 4)) return PSF_ERR_PARAM;
  if (!image_map().ok) return PSF_ERR_UNSUPPORTED;
  if (count == 0) return PSF_OK;
  PSF_TRY(use_device(device));
  DevBuf df, dh;
  HIP_TRY(df.alloc(count * kN * 8));
  HIP_TRY(dh.alloc(count * kN * 4));
  if (from) HIP_TRY(df.upload(fhat, count * kN * 8));
  else HIP_TRY(dh.upload(hat, count * kN * 4));
  const psf_status rc = image_call(device, count, df.as<void>(), 64, dh.as<uint32_t>(), from, nullptr);
  if (rc != PSF_OK) return rc;
  if (from) HIP_TRY(dh.download(const_cast<uint32_t*>(hat), count * kN * 4));
  else HIP_TRY(df.download(const_cast<void*>(fhat), count * kN * 8));
  return PSF_OK;
}

}  // namespace kc
}  // namespace psf

using namespace psf;
using namespace psf::kc;

extern "C" {

psf_status psf_keccak_dev(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len,
                          size_t out_stride, void* stream) {
  FuncSpec f;
  size_t in_span = 0, out_span = 0;
  const psf_status rc = check_keccak(func, count, d_in, in_len, in_stride, d_out, out_len, out_stride, &f, &in_span, &out_span);
  if (rc != PSF_OK || count == 0) return rc;
  return keccak_launch(device, f, count, d_in, in_len, in_stride, d_out, out_len, out_stride, (hipStream_t)stream);
}

psf_status psf_keccak(int device, int func, size_t count, const uint8_t* in, size_t in_len, size_t in_stride, uint8_t* out, size_t out_len, size_t out_stride) {
  FuncSpec f;
  size_t in_span = 0, out_span = 0;
  const psf_status rc = check_keccak(func, count, in, in_len, in_stride, out, out_len, out_stride, &f, &in_span, &out_span);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  HostCall h;                                                            // packed rows on the device
  const uint8_t* din = h.in(in, count, in_len, in_stride);
  uint8_t* dout = h.out(count * out_len);
  PSF_TRY(h.status());
  PSF_TRY(keccak_launch(device, f, count, din, in_len, in_len, dout, out_len, out_len, nullptr));
  return h.fetch(out, dout, count, out_len, out_stride);
}

psf_status psf_sample_ntt_fips203_dev(int device, size_t count, uint32_t k, const uint8_t* d_seed, size_t seed_stride, void* d_out, int* d_fail, int io_bits,
                                      void* stream) {
  size_t total = 0, seed_span = 0;
  const psf_status rc = check_sample_ntt(count, k, d_seed, seed_stride, d_out, io_bits, &total, &seed_span);
  if (rc != PSF_OK || total == 0) return rc;
  return sample_ntt_launch(device, total, k, d_seed, seed_stride, d_out, d_fail, io_bits, (hipStream_t)stream);
}

psf_status psf_sample_ntt_fips203(int device, size_t count, uint32_t k, const uint8_t* seed, size_t seed_stride, uint64_t* out) {
  size_t total = 0, seed_span = 0;
  const psf_status rc = check_sample_ntt(count, k, seed, seed_stride, out, 64, &total, &seed_span);
  if (rc != PSF_OK || total == 0) return rc;
  PSF_TRY(use_device(device));
  const size_t len = k ? 32 : 34, bytes = total * kN * sizeof(uint64_t);
  HostCall h;
  const uint8_t* dseed = h.in(seed, count, len, seed_stride);
  uint8_t* dout = h.out(bytes);
  int* dflag = h.flag();
  PSF_TRY(h.status());
  PSF_TRY(sample_ntt_launch(device, total, k, dseed, len, dout, dflag, 64, nullptr));
  PSF_TRY(h.fetch(out, dout, bytes));
  return h.finish();
}

psf_status psf_sample_cbd_fips203_dev(int device, size_t count, uint32_t eta, const uint8_t* d_sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed,
                                      void* d_out, int io_bits, void* stream) {
  size_t total = 0, sigma_span = 0;
  const psf_status rc = check_sample_cbd(count, eta, d_sigma, sigma_stride, first_nonce, per_seed, d_out, io_bits, &total, &sigma_span);
  if (rc != PSF_OK || total == 0) return rc;
  return sample_cbd_launch(device, total, eta, d_sigma, sigma_stride, first_nonce, per_seed, d_out, io_bits, (hipStream_t)stream);
}

psf_status psf_sample_cbd_fips203(int device, size_t count, uint32_t eta, const uint8_t* sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed,
                                  int64_t* out) {
  size_t total = 0, sigma_span = 0;
  const psf_status rc = check_sample_cbd(count, eta, sigma, sigma_stride, first_nonce, per_seed, out, 64, &total, &sigma_span);
  if (rc != PSF_OK || total == 0) return rc;
  PSF_TRY(use_device(device));
  const size_t bytes = total * kN * sizeof(int64_t);
  HostCall h;
  const uint8_t* dsigma = h.in(sigma, count, 32, sigma_stride);
  uint8_t* dout = h.out(bytes);
  PSF_TRY(h.status());
  PSF_TRY(sample_cbd_launch(device, total, eta, dsigma, 32, first_nonce, per_seed, dout, 64, nullptr));
  return h.fetch(out, dout, bytes);
}

psf_status psf_ntt_image_from_fips203_dev(int device, size_t count, const void* d_fhat, int io_bits, uint32_t* d_hat, void* stream) {
  return image_call(device, count, d_fhat, io_bits, d_hat, true, (hipStream_t)stream);
}
psf_status psf_ntt_image_to_fips203_dev(int device, size_t count, const uint32_t* d_hat, void* d_fhat, int io_bits, void* stream) {
  return image_call(device, count, d_fhat, io_bits, d_hat, false, (hipStream_t)stream);
}
psf_status psf_ntt_image_from_fips203(int device, size_t count, const uint64_t* fhat, uint32_t* hat) { return image_host(device, count, fhat, hat, true); }
psf_status psf_ntt_image_to_fips203(int device, size_t count, const uint32_t* hat, uint64_t* fhat) { return image_host(device, count, fhat, hat, false); }

}  // extern "C"
