// psf_compress.hip -- the two other R_q coefficient maps of the ML-KEM-style schemes next to the products of psf_ntt.hip:
//   FIPS 203 Compress_d / Decompress_d (compression/lossy_compression_fips203.rs:89-112, :143-172) and the message layer
//   out = digit * floor(q/base) mod q / digit = round(base * c / q) mod base (utils/common_encodings.rs:49-91, :125-151).
// Every map is one pass over a flat array of coefficients: memory-bound streams, 16-byte non-temporal loads and stores per lane.
// Exact integer arithmetic without a division on the device: the host precomputes the constants of each call (DESIGN.md "Compression and
// message encodings").
#include <hip/hip_runtime.h>
#include <cstdio>
#include <mutex>
#include "../../include/psf_mi355x.h"

#define CMP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess) {                                                           \
      std::fprintf(stderr, "[psf_mi355x] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return PSF_ERR_HIP;                                                              \
    }                                                                                  \
  } while (0)

namespace psf {
namespace cmp {

typedef unsigned __int128 u128;
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

enum { OP_COMPRESS = 0, OP_DECOMPRESS = 1, OP_ENCODE = 2, OP_DECODE = 3 };

// per-call constants, computed on the host (make_args) and passed by value
struct CmpArgs {
  uint64_t q;      // the modulus, 2 <= q < 2^62
  uint64_t qn;     // q << sh: the normalised divisor (top bit set)
  uint64_t v;      // floor((2^128 - 1) / qn) - 2^64: the reciprocal of the 2-by-1 division (Moeller-Granlund, Algorithm 4)
  uint64_t m16;    // ceil(2^64 / q): floor(n / q) = mulhi64(m16, n) for every n < 2^32 (16-bit words only, q <= 2^16)
  uint64_t c;      // compress: floor(q/2); decompress: 2^(d-1); encode: floor(q/base); decode: floor(q/(2 base))
  uint64_t base;   // decode: the base
  uint64_t mask;   // compress / decompress: 2^d - 1
  uint32_t sh;     // clz(q)
  uint32_t d;      // compress / decompress: d in [1, 63]
};

// floor((hi:lo) / q) for hi < q, remainder in *rem.  The numerator is shifted by sh so that the divisor qn has its top bit set; then one
// 64x64 -> 128 product with the reciprocal and at most two corrections (Moeller, Granlund: Improved division by invariant integers, 2011).
__device__ __forceinline__ uint64_t divrem_q(const CmpArgs& a, uint64_t hi, uint64_t lo, uint64_t* rem) {
  const uint64_t u1 = (hi << a.sh) | ((lo >> 1) >> (63 - a.sh));        // (lo >> 1) >> 63 is 0: sh = 0 needs no branch
  const uint64_t u0 = lo << a.sh;
  uint64_t q0 = a.v * u1;
  uint64_t q1 = __umul64hi(a.v, u1);
  q0 += u0;
  q1 += u1 + 1 + (q0 < u0);
  uint64_t r = u0 - q1 * a.qn;
  if (r > q0) { --q1; r += a.qn; }
  if (r >= a.qn) { ++q1; r -= a.qn; }
  *rem = r >> a.sh;
  return q1;
}

__device__ __forceinline__ uint64_t reduce_q(const CmpArgs& a, uint64_t x) {
  if (x >= a.q) divrem_q(a, 0, x, &x);
  return x;
}

// floor(n / q) for n < 2^32 and q <= 2^16 (Lemire, Kaser, Kurz: Faster remainder by direct computation, 2019, with F = 64 >= 32 + 17)
__device__ __forceinline__ uint32_t div32_q(const CmpArgs& a, uint32_t n) {
  const uint64_t t = (uint64_t)(uint32_t)a.m16 * n;
  const uint64_t h = (a.m16 >> 32) * n + (t >> 32);                    // < 2^64: (2^32 - 1)^2 + 2^32
  return (uint32_t)(h >> 32);
}

// one coefficient, 64-bit words (bit patterns of the ABI's uint64 / int64)
template <int OP> __device__ __forceinline__ uint64_t map64(const CmpArgs& a, uint64_t w) {
  uint64_t r;
  if constexpr (OP == OP_COMPRESS) {                                    // floor((x 2^d + floor(q/2)) / q) mod 2^d, x read mod q
    const uint64_t x = reduce_q(a, w);
    uint64_t lo = x << a.d;
    uint64_t hi = x >> (64 - a.d);                                      // d in [1, 63]
    lo += a.c;
    hi += lo < a.c;
    return divrem_q(a, hi, lo, &r) & a.mask;                            // numerator < q 2^63 + q: hi < q
  } else if constexpr (OP == OP_DECOMPRESS) {                           // floor((y' q + 2^(d-1)) / 2^d) with y' = y mod 2^d: <= q
    const uint64_t y = w & a.mask;
    uint64_t lo = y * a.q;
    uint64_t hi = __umul64hi(y, a.q);
    lo += a.c;
    hi += lo < a.c;
    const uint64_t x = (hi << (64 - a.d)) | (lo >> a.d);
    return x == a.q ? 0 : x;
  } else if constexpr (OP == OP_ENCODE) {                               // digit floor(q/base) mod q: numerator < 2^64 q
    divrem_q(a, __umul64hi(w, a.c), w * a.c, &r);
    return r;
  } else {                                                              // floor((base c + floor(q/(2 base))) / q) mod base, c read mod q
    const uint64_t c = reduce_q(a, w);
    uint64_t lo = c * a.base;
    uint64_t hi = __umul64hi(c, a.base);
    lo += a.c;
    hi += lo < a.c;
    const uint64_t t = divrem_q(a, hi, lo, &r);                         // numerator < q 2^63 + q; the quotient is at most base
    return t == a.base ? 0 : t;
  }
}

// one coefficient, 16-bit words (q, base <= 2^16, d <= 16): every numerator below 2^32, one division by the multiplier m16
template <int OP> __device__ __forceinline__ uint32_t map16(const CmpArgs& a, uint32_t w) {
  const uint32_t q = (uint32_t)a.q;
  if constexpr (OP == OP_COMPRESS) {
    const uint32_t x = w - div32_q(a, w) * q;
    return div32_q(a, (x << a.d) + (uint32_t)a.c) & (uint32_t)a.mask;   // <= (2^16 - 1) 2^16 + 2^15
  } else if constexpr (OP == OP_DECOMPRESS) {                           // y mod 2^d is the same for the word read signed or unsigned
    const uint32_t x = (uint32_t)(((uint64_t)(w & (uint32_t)a.mask) * q + a.c) >> a.d);
    return x == q ? 0 : x;
  } else if constexpr (OP == OP_ENCODE) {
    const uint32_t n = w * (uint32_t)a.c;                               // < 2^16 2^15
    return n - div32_q(a, n) * q;
  } else {
    const uint32_t c = w - div32_q(a, w) * q;
    const uint32_t t = div32_q(a, c * (uint32_t)a.base + (uint32_t)a.c);   // <= (2^16 - 1) 2^16 + 2^14
    return t == (uint32_t)a.base ? 0 : t;
  }
}

template <int OP, int IO> __device__ __forceinline__ void map_one(const CmpArgs& a, const void* in, void* out, size_t e) {
  if constexpr (IO == 16) {
    static_cast<uint16_t*>(out)[e] = (uint16_t)map16<OP>(a, static_cast<const uint16_t*>(in)[e]);
  } else {
    static_cast<uint64_t*>(out)[e] = map64<OP>(a, static_cast<const uint64_t*>(in)[e]);
  }
}

template <int OP, int IO> __device__ __forceinline__ v4u map_vec(const CmpArgs& a, v4u w) {
  v4u r;
  if constexpr (IO == 16) {                                             // 8 words: the low and high half of each dword
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = map16<OP>(a, w[j] & 0xffffu) | (map16<OP>(a, w[j] >> 16) << 16);
  } else {                                                              // 2 words
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint64_t x = map64<OP>(a, (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32));
      r[2 * j] = (uint32_t)x;
      r[2 * j + 1] = (uint32_t)(x >> 32);
    }
  }
  return r;
}

constexpr int kUnroll = 4;       // 16-byte vectors in flight per lane

// elements [0, head) and [head + EPV nvec, len) word by word, the nvec 16-byte vectors between them (16-byte aligned in `in` and in `out`) by
// a grid-stride loop, kUnroll vectors per lane per step.  The host passes head = len, nvec = 0 when the two pointers cannot both be aligned.
template <int OP, int IO>
__global__ __launch_bounds__(256) void k_coeff_map(CmpArgs a, const void* __restrict__ in, void* __restrict__ out, size_t len, size_t head, size_t nvec) {
  constexpr size_t EPV = IO == 16 ? 8 : 2;                              // words per 16-byte vector
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const v4u* vin = reinterpret_cast<const v4u*>(static_cast<const char*>(in) + head * (IO / 8));
  v4u* vout = reinterpret_cast<v4u*>(static_cast<char*>(out) + head * (IO / 8));
  for (size_t i0 = gid; i0 < nvec; i0 += kUnroll * stride) {
    v4u w[kUnroll] = {};
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t i = i0 + u * stride;
      if (i < nvec) w[u] = __builtin_nontemporal_load(vin + i);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t i = i0 + u * stride;
      if (i < nvec) __builtin_nontemporal_store(map_vec<OP, IO>(a, w[u]), vout + i);
    }
  }
  const size_t body = nvec * EPV, rest = len - head - body;
  for (size_t g = gid; g < head + rest; g += stride) map_one<OP, IO>(a, in, out, g < head ? g : g + body);
}

// argument checks: everything before the first HIP call (the CPU suite asserts these codes)
psf_status check_common(uint64_t q, size_t len, const void* in, const void* out) {
  if (q < 2 || (len && (!in || !out))) return PSF_ERR_PARAM;
  if (q >= (1ull << 62)) return PSF_ERR_UNSUPPORTED;
  return PSF_OK;
}
psf_status check_io(int io_bits) { return io_bits == 16 || io_bits == 64 ? PSF_OK : PSF_ERR_PARAM; }
psf_status check_d(uint64_t q, uint32_t d, int io_bits) {
  if (d < 1) return PSF_ERR_PARAM;
  if (d > 63 || (io_bits == 16 && (d > 16 || q > (1ull << 16)))) return PSF_ERR_UNSUPPORTED;
  return PSF_OK;
}
psf_status check_base(uint64_t q, uint64_t base, int io_bits) {
  if (base < 2) return PSF_ERR_PARAM;
  if (base >= (1ull << 63) || (io_bits == 16 && (base > (1ull << 16) || q > (1ull << 16)))) return PSF_ERR_UNSUPPORTED;
  return PSF_OK;
}

CmpArgs make_args(int op, uint64_t q, uint64_t d_or_base) {
  CmpArgs a{};
  a.q = q;
  a.sh = (uint32_t)__builtin_clzll(q);
  a.qn = q << a.sh;
  a.v = (uint64_t)(~(u128)0 / a.qn);                                    // floor((2^128 - 1) / qn) - 2^64, taken mod 2^64
  a.m16 = q <= (1ull << 16) ? (uint64_t)((((u128)1 << 64) + q - 1) / q) : 0;
  if (op == OP_COMPRESS || op == OP_DECOMPRESS) {
    a.d = (uint32_t)d_or_base;
    a.mask = (1ull << a.d) - 1;
    a.c = op == OP_COMPRESS ? q / 2 : 1ull << (a.d - 1);
  } else {
    a.base = d_or_base;
    a.c = op == OP_ENCODE ? q / d_or_base : (uint64_t)(q / ((u128)2 * d_or_base));
  }
  return a;
}

// compute units of a device, queried once
int device_cus(int device) {
  static std::mutex mu;
  static int cus[64] = {0};
  if (device < 0 || device >= 64) return 0;
  std::lock_guard<std::mutex> lk(mu);
  if (!cus[device] && hipDeviceGetAttribute(&cus[device], hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus[device] = 0;
  return cus[device];
}

template <int OP> void launch_op(int io_bits, dim3 grid, hipStream_t st, const CmpArgs& a, const void* in, void* out, size_t len, size_t head, size_t nvec) {
  if (io_bits == 16) hipLaunchKernelGGL((k_coeff_map<OP, 16>), grid, dim3(256), 0, st, a, in, out, len, head, nvec);
  else hipLaunchKernelGGL((k_coeff_map<OP, 64>), grid, dim3(256), 0, st, a, in, out, len, head, nvec);
}

// the launch of checked arguments on device buffers, in `stream`, nothing allocated
psf_status map_dev(int op, int device, uint64_t q, uint64_t d_or_base, size_t len, const void* in, void* out, int io_bits, hipStream_t st) {
  if (len == 0) return PSF_OK;
  CMP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const size_t wb = (size_t)io_bits / 8, epv = 16 / wb;
  const uintptr_t pi = (uintptr_t)in, po = (uintptr_t)out;
  size_t head = len, nvec = 0;
  if (pi % wb == 0 && pi % 16 == po % 16) {                             // both reach a 16-byte boundary after the same number of words
    head = ((16 - pi % 16) % 16) / wb;
    if (head > len) head = len;
    nvec = (len - head) / epv;
  }
  const size_t vwork = (nvec + kUnroll - 1) / kUnroll, swork = len - nvec * epv, work = vwork > swork ? vwork : swork;
  size_t blocks = (work + 255) / 256;
  const size_t cap = (size_t)cus * 8;                                   // 8 workgroups of 256 lanes per CU: 8 waves per SIMD
  blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
  const CmpArgs a = make_args(op, q, d_or_base);
  const dim3 grid((unsigned)blocks);
  switch (op) {
    case OP_COMPRESS: launch_op<OP_COMPRESS>(io_bits, grid, st, a, in, out, len, head, nvec); break;
    case OP_DECOMPRESS: launch_op<OP_DECOMPRESS>(io_bits, grid, st, a, in, out, len, head, nvec); break;
    case OP_ENCODE: launch_op<OP_ENCODE>(io_bits, grid, st, a, in, out, len, head, nvec); break;
    default: launch_op<OP_DECODE>(io_bits, grid, st, a, in, out, len, head, nvec); break;
  }
  CMP_TRY(hipGetLastError());
  return PSF_OK;
}

// host-pointer form: copy in, run on the device (64-bit words), copy out.  No CPU fallback.
psf_status map_host(int op, int device, uint64_t q, uint64_t d_or_base, size_t len, const void* in, void* out) {
  if (len == 0) return PSF_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return PSF_ERR_HIP;
  CMP_TRY(hipSetDevice(device));
  void *din = nullptr, *dout = nullptr;
  auto done = [&](psf_status s) { (void)hipFree(din); (void)hipFree(dout); return s; };
  const size_t bytes = len * sizeof(uint64_t);
  if (hipMalloc(&din, bytes) != hipSuccess || hipMalloc(&dout, bytes) != hipSuccess) return done(PSF_ERR_HIP);
  if (hipMemcpy(din, in, bytes, hipMemcpyHostToDevice) != hipSuccess) return done(PSF_ERR_HIP);
  const psf_status rc = map_dev(op, device, q, d_or_base, len, din, dout, 64, nullptr);
  if (rc != PSF_OK) return done(rc);
  if (hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) != hipSuccess) return done(PSF_ERR_HIP);
  return done(PSF_OK);
}

}  // namespace cmp
}  // namespace psf

using namespace psf::cmp;

extern "C" {

psf_status psf_lossy_compress(int device, uint64_t q, uint32_t d, size_t len, const uint64_t* x, int64_t* y) {
  psf_status rc = check_common(q, len, x, y);
  if (rc == PSF_OK) rc = check_d(q, d, 64);
  return rc != PSF_OK ? rc : map_host(OP_COMPRESS, device, q, d, len, x, y);
}
psf_status psf_lossy_decompress(int device, uint64_t q, uint32_t d, size_t len, const int64_t* y, uint64_t* x) {
  psf_status rc = check_common(q, len, y, x);
  if (rc == PSF_OK) rc = check_d(q, d, 64);
  return rc != PSF_OK ? rc : map_host(OP_DECOMPRESS, device, q, d, len, y, x);
}
psf_status psf_encode_digits(int device, uint64_t q, uint64_t base, size_t len, const uint64_t* digits, uint64_t* out) {
  psf_status rc = check_common(q, len, digits, out);
  if (rc == PSF_OK) rc = check_base(q, base, 64);
  return rc != PSF_OK ? rc : map_host(OP_ENCODE, device, q, base, len, digits, out);
}
psf_status psf_decode_digits(int device, uint64_t q, uint64_t base, size_t len, const uint64_t* coeffs, uint64_t* digits) {
  psf_status rc = check_common(q, len, coeffs, digits);
  if (rc == PSF_OK) rc = check_base(q, base, 64);
  return rc != PSF_OK ? rc : map_host(OP_DECODE, device, q, base, len, coeffs, digits);
}

psf_status psf_lossy_compress_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_x, void* d_y, int io_bits, void* stream) {
  psf_status rc = check_io(io_bits);
  if (rc == PSF_OK) rc = check_common(q, len, d_x, d_y);
  if (rc == PSF_OK) rc = check_d(q, d, io_bits);
  return rc != PSF_OK ? rc : map_dev(OP_COMPRESS, device, q, d, len, d_x, d_y, io_bits, (hipStream_t)stream);
}
psf_status psf_lossy_decompress_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_y, void* d_x, int io_bits, void* stream) {
  psf_status rc = check_io(io_bits);
  if (rc == PSF_OK) rc = check_common(q, len, d_y, d_x);
  if (rc == PSF_OK) rc = check_d(q, d, io_bits);
  return rc != PSF_OK ? rc : map_dev(OP_DECOMPRESS, device, q, d, len, d_y, d_x, io_bits, (hipStream_t)stream);
}
psf_status psf_encode_digits_dev(int device, uint64_t q, uint64_t base, size_t len, const void* d_digits, void* d_out, int io_bits, void* stream) {
  psf_status rc = check_io(io_bits);
  if (rc == PSF_OK) rc = check_common(q, len, d_digits, d_out);
  if (rc == PSF_OK) rc = check_base(q, base, io_bits);
  return rc != PSF_OK ? rc : map_dev(OP_ENCODE, device, q, base, len, d_digits, d_out, io_bits, (hipStream_t)stream);
}
psf_status psf_decode_digits_dev(int device, uint64_t q, uint64_t base, size_t len, const void* d_coeffs, void* d_digits, int io_bits, void* stream) {
  psf_status rc = check_io(io_bits);
  if (rc == PSF_OK) rc = check_common(q, len, d_coeffs, d_digits);
  if (rc == PSF_OK) rc = check_base(q, base, io_bits);
  return rc != PSF_OK ? rc : map_dev(OP_DECODE, device, q, base, len, d_coeffs, d_digits, io_bits, (hipStream_t)stream);
}

}  // extern "C"
