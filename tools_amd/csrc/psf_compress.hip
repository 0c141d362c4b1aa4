// psf_compress.hip -- the two other R_q coefficient maps of the ML-KEM-style schemes next to the products of psf_ntt.hip:
//   FIPS 203 Compress_d / Decompress_d (compression/lossy_compression_fips203.rs:89-112, :143-172) and the message layer
//   out = digit * floor(q/base) mod q / digit = round(base * c / q) mod base (utils/common_encodings.rs:49-91, :125-151).
// and the FIPS 203 byte encodings ByteEncode_d / ByteDecode_d (Algorithms 5 / 6) of the d-bit values, alone or fused with Compress_d / Decompress_d.
// Every map is one pass over a flat array of coefficients: memory-bound streams, 16-byte non-temporal loads and stores per lane.
// Exact integer arithmetic without a division on the device: the host precomputes the constants of each call (DESIGN.md "Compression and
// message encodings").
#include "psf_call_host.hpp"
#include "psf_hip_util.hpp"
#include "psf_stream_host.hpp"

namespace psf {
namespace cmp {

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

// the launch of checked arguments on device buffers, in `stream`, nothing allocated
psf_status map_dev(int op, int device, uint64_t q, uint64_t d_or_base, size_t len, const void* in, void* out, int io_bits, hipStream_t st) {
  if (len == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const size_t wb = (size_t)io_bits / 8, epv = 16 / wb;
  const StreamSplit sp = split_stream_pair((uintptr_t)in, (uintptr_t)out, wb, len, epv);
  const size_t head = sp.head, nvec = sp.nvec;
  const size_t vwork = (nvec + kUnroll - 1) / kUnroll, swork = len - nvec * epv;
  const dim3 grid(grid_blocks(vwork > swork ? vwork : swork, 0, cus, 8));      // 8 workgroups of 256 lanes per CU: 8 waves per SIMD
  const CmpArgs a = make_args(op, q, d_or_base);
  for_int<16, 64>(io_bits, [&](auto io) {
    for_int<OP_COMPRESS, OP_DECOMPRESS, OP_ENCODE, OP_DECODE>(op, [&](auto o) {
      hipLaunchKernelGGL((k_coeff_map<decltype(o)::value, decltype(io)::value>), grid, dim3(256), 0, st, a, in, out, len, head, nvec);
    });
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// host-pointer form: copy in, run on the device (64-bit words), copy out.  No CPU fallback.
psf_status map_host(int op, int device, uint64_t q, uint64_t d_or_base, size_t len, const void* in, void* out) {
  if (len == 0) return PSF_OK;
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  const size_t bytes = len * sizeof(uint64_t);
  DevBuf din, dout;
  HIP_TRY(din.alloc(bytes));
  HIP_TRY(dout.alloc(bytes));
  HIP_TRY(din.upload(in, bytes));
  const psf_status rc = map_dev(op, device, q, d_or_base, len, din.as<void>(), dout.as<void>(), 64, nullptr);
  if (rc != PSF_OK) return rc;
  HIP_TRY(dout.download(out, bytes));
  return PSF_OK;
}

// the four maps behind their entry points: the checks in the header's order, then the device form in `st` or (host) the host-pointer form
psf_status map_call(int op, int device, uint64_t q, uint64_t d_or_base, size_t len, const void* in, void* out, int io_bits, void* st, bool host = false) {
  psf_status rc = check_io(io_bits);
  if (rc == PSF_OK) rc = check_common(q, len, in, out);
  if (rc == PSF_OK) rc = op == OP_COMPRESS || op == OP_DECOMPRESS ? check_d(q, (uint32_t)d_or_base, io_bits) : check_base(q, d_or_base, io_bits);
  if (rc != PSF_OK) return rc;
  return host ? map_host(op, device, q, d_or_base, len, in, out) : map_dev(op, device, q, d_or_base, len, in, out, io_bits, (hipStream_t)st);
}

// ---- FIPS 203 ByteEncode_d / ByteDecode_d (Algorithms 5 / 6) and their fusions with Compress_d / Decompress_d --------------------------------
// Value i of a flat array owns stream bits [i d, i d + d); byte b holds stream bits [8 b, 8 b + 8), least significant first.  A tile is
// kTileVec 16-byte vectors of values (8192 16-bit words or 2048 64-bit words): a whole number of 16-byte vectors of packed bytes for every d.
// Values and bytes move by coalesced 16-byte non-temporal vectors; the bit shuffle between the two layouts goes through LDS (DESIGN.md
// "Compression and message encodings").  Everything outside whole tiles -- the ragged end, the final partial byte, buffers that are not both
// 16-byte aligned -- runs byte by byte (pack) or value by value (unpack) from global memory.
constexpr int kTileVec = 1024;                                          // 4 vectors per lane of a 256-lane workgroup: 16 KiB of values
enum { UNPACK_RAW = 0, UNPACK_MODQ = 1, UNPACK_DECOMPRESS = 2 };

template <int IO> struct LdsWord { typedef uint16_t type; };
template <> struct LdsWord<64> { typedef uint64_t type; };

// floor(s / d) without a division: m = floor((2^W - 1) / d) gives floor(s m / 2^W) in {floor(s/d) - 1, floor(s/d)} for every s < 2^W
// (s/d - s m/2^W = s (2^W - m d) / (d 2^W) <= s / 2^W < 1), and one comparison settles it.
__device__ __forceinline__ uint32_t div_d32(uint32_t s, uint32_t d, uint32_t m) {
  const uint32_t t = __umulhi(s, m);
  return t + ((t + 1) * d <= s);
}
__device__ __forceinline__ uint64_t div_d64(uint64_t s, uint32_t d, uint64_t m) {
  const uint64_t t = __umul64hi(s, m);
  return t + ((t + 1) * d <= s);
}

// the d-bit value of one word on its way into the stream: y mod 2^d, or Compress_d(x)
template <int FUSED, int IO> __device__ __forceinline__ v4u pack_vec(const CmpArgs& a, v4u w) {
  if constexpr (FUSED) return map_vec<OP_COMPRESS, IO>(a, w);
  v4u r;
  if constexpr (IO == 16) {
    const uint32_t m2 = (uint32_t)a.mask * 0x10001u;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = w[j] & m2;
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      r[2 * j] = w[2 * j] & (uint32_t)a.mask;
      r[2 * j + 1] = w[2 * j + 1] & (uint32_t)(a.mask >> 32);
    }
  }
  return r;
}
template <int FUSED, int IO> __device__ __forceinline__ uint64_t pack_word(const CmpArgs& a, const void* in, size_t e) {
  if constexpr (IO == 16) {
    const uint32_t w = static_cast<const uint16_t*>(in)[e];
    return FUSED ? map16<OP_COMPRESS>(a, w) : (w & (uint32_t)a.mask);
  } else {
    const uint64_t w = static_cast<const uint64_t*>(in)[e];
    return FUSED ? map64<OP_COMPRESS>(a, w) : (w & a.mask);
  }
}

// stream bits [s, s + 32) of a tile from its d-bit values in LDS: values floor(s / d) ... while they start below s + 32
template <int IO> __device__ __forceinline__ uint32_t gather_dword(const typename LdsWord<IO>::type* vals, uint32_t s, uint32_t d, uint32_t md) {
  uint32_t idx = div_d32(s, d, md);
  int pos = (int)(idx * d) - (int)s;                                    // in (-d, 0]: where value idx starts, relative to s
  uint32_t dw = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)    // either would divide by d for its trip count
  for (; pos < 32; ++idx, pos += (int)d) {                              // idx d < s + 32 <= the tile's bits: idx stays inside the tile
    const uint64_t v = vals[idx];
    dw |= pos >= 0 ? (uint32_t)(v << pos) : (uint32_t)(v >> -pos);
  }
  return dw;
}

// ByteEncode_d (FUSED = 0) and ByteEncode_d(Compress_d(.)) (FUSED = 1).  Whole tiles: 4 coalesced 16-byte loads per lane, the d-bit values
// parked in LDS, every lane gathers the tile's output dwords tid, tid + 256, ... (d or d / 4 of them: the same count in every lane), and
// the staged dwords leave as coalesced 16-byte stores.  Then bytes [tail0, nbytes) one per lane from global memory: whole bytes only, each
// written by exactly one lane, values at or beyond len read as absent (the unused high bits of the last byte are 0).
template <int FUSED, int IO>
__global__ __launch_bounds__(256) void k_pack(CmpArgs a, uint32_t md32, uint64_t md64, const void* __restrict__ in, uint8_t* __restrict__ out, size_t len,
                                              size_t ntiles, size_t nbytes) {
  typedef typename LdsWord<IO>::type word_t;
  constexpr uint32_t TV = kTileVec * (IO == 16 ? 8 : 2);                // values per tile
  __shared__ v4u s_val[kTileVec];
  __shared__ v4u s_out[kTileVec];                                       // TV d / 128 vectors: at most 1024 (d = 16) or 1008 (d = 63)
  const uint32_t tid = threadIdx.x;
  const uint32_t ndw = TV / 32 * a.d;                                   // packed dwords per tile
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const v4u* vin = static_cast<const v4u*>(in) + t * kTileVec;
    v4u w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = __builtin_nontemporal_load(vin + tid + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u) s_val[tid + 256 * u] = pack_vec<FUSED, IO>(a, w[u]);
    __syncthreads();
    for (uint32_t k = tid; k < ndw; k += 256)
      reinterpret_cast<uint32_t*>(s_out)[k] = gather_dword<IO>(reinterpret_cast<const word_t*>(s_val), 32 * k, a.d, md32);
    __syncthreads();
    v4u* vout = reinterpret_cast<v4u*>(out + t * (size_t)(TV / 8) * a.d);
    for (uint32_t j = tid; j < ndw / 4; j += 256) __builtin_nontemporal_store(s_out[j], vout + j);
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t b = ntiles * (size_t)(TV / 8) * a.d + (size_t)blockIdx.x * blockDim.x + tid; b < nbytes; b += stride) {
    const uint64_t s = (uint64_t)b * 8;
    uint64_t idx = div_d64(s, a.d, md64);
    int pos = (int)(int64_t)(idx * a.d - s);
    uint32_t by = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (; pos < 8 && idx < len; ++idx, pos += (int)a.d) {
      const uint64_t v = pack_word<FUSED, IO>(a, in, idx);
      by |= pos >= 0 ? (uint32_t)(v << pos) : (uint32_t)(v >> -pos);
    }
    out[b] = (uint8_t)by;
  }
}

// what ByteDecode_d does with a d-bit value v: nothing, its residue mod q (noting v >= q), or Decompress_d
template <int MODE, int IO> __device__ __forceinline__ uint64_t unpack_value(const CmpArgs& a, uint64_t v, bool* bad) {
  if constexpr (MODE == UNPACK_RAW) return v;
  if constexpr (MODE == UNPACK_MODQ) {
    *bad |= v >= a.q;
    if constexpr (IO == 16) return (uint32_t)v - div32_q(a, (uint32_t)v) * (uint32_t)a.q;
    else return reduce_q(a, v);
  }
  if constexpr (IO == 16) return map16<OP_DECOMPRESS>(a, (uint32_t)v);
  else return map64<OP_DECOMPRESS>(a, v);
}

// value i of a tile from its packed dwords in LDS (two dwords past the tile may be read; their bits are masked off)
template <int IO> __device__ __forceinline__ uint64_t extract(const uint32_t* s, uint32_t i, const CmpArgs& a) {
  const uint32_t bit = i * a.d, wi = bit >> 5, sh = bit & 31;
  const uint64_t lo = (uint64_t)s[wi] | ((uint64_t)s[wi + 1] << 32);
  if constexpr (IO == 16) return (uint32_t)(lo >> sh) & (uint32_t)a.mask;                     // sh + d <= 47
  else return ((lo >> sh) | (((uint64_t)s[wi + 2] << 32) << (32 - sh))) & a.mask;             // sh + d <= 94
}

// ByteDecode_d (UNPACK_RAW, UNPACK_MODQ) and Decompress_d(ByteDecode_d(.)) (UNPACK_DECOMPRESS): the reverse of k_pack.  Whole tiles: up to 4
// coalesced 16-byte loads of packed bytes per lane into LDS, then every lane extracts the 8 (16-bit) or 2 (64-bit) values of each of its
// 4 output vectors and stores them coalesced.  Then values [ntiles TV, len) one per lane from the bytes in global memory.
template <int MODE, int IO>
__global__ __launch_bounds__(256) void k_unpack(CmpArgs a, const uint8_t* __restrict__ in, void* __restrict__ out, int* __restrict__ flag, size_t len,
                                                size_t ntiles) {
  constexpr uint32_t EPV = IO == 16 ? 8 : 2, TV = kTileVec * EPV;
  __shared__ v4u s_in[kTileVec + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t nvin = TV / 128 * a.d;                                 // packed 16-byte vectors per tile: at most 1024
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(s_in);
  bool bad = false;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const v4u* vin = reinterpret_cast<const v4u*>(in + t * (size_t)(TV / 8) * a.d);
    v4u w[4] = {};
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (tid + 256 * u < nvin) w[u] = __builtin_nontemporal_load(vin + tid + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (tid + 256 * u < nvin) s_in[tid + 256 * u] = w[u];
    __syncthreads();
    v4u* vout = static_cast<v4u*>(out) + t * kTileVec;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t i0 = (tid + 256 * u) * EPV;
      v4u r;
      if constexpr (IO == 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t x0 = (uint32_t)unpack_value<MODE, 16>(a, extract<16>(sw, i0 + 2 * j, a), &bad);
          const uint32_t x1 = (uint32_t)unpack_value<MODE, 16>(a, extract<16>(sw, i0 + 2 * j + 1, a), &bad);
          r[j] = x0 | (x1 << 16);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint64_t x = unpack_value<MODE, 64>(a, extract<64>(sw, i0 + j, a), &bad);
          r[2 * j] = (uint32_t)x;
          r[2 * j + 1] = (uint32_t)(x >> 32);
        }
      }
      __builtin_nontemporal_store(r, vout + tid + 256 * u);
    }
    __syncthreads();
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = ntiles * (size_t)TV + (size_t)blockIdx.x * blockDim.x + tid; i < len; i += stride) {
    const uint64_t bit = (uint64_t)i * a.d;
    const uint8_t* p = in + (bit >> 3);
    const int sh = (int)(bit & 7);
    uint64_t v = 0;
    for (int k = 0; 8 * k < sh + (int)a.d; ++k) {                       // at most 9 bytes, every one below ceil(len d / 8)
      const uint64_t by = p[k];
      const int off = 8 * k - sh;
      v |= off >= 0 ? by << off : by >> -off;
    }
    const uint64_t x = unpack_value<MODE, IO>(a, v & a.mask, &bad);
    if constexpr (IO == 16) static_cast<uint16_t*>(out)[i] = (uint16_t)x;
    else static_cast<uint64_t*>(out)[i] = x;
  }
  if constexpr (MODE == UNPACK_MODQ) {
    if (flag && bad) atomicOr(flag, 1);                                 // one vector atomic per lane that met a value >= q
  }
}

enum { BY_ENCODE = 0, BY_DECODE = 1, BY_COMPRESS_ENCODE = 2, BY_DECODE_DECOMPRESS = 3 };

// argument checks of the eight byte-encoding entry points, every PSF_ERR_PARAM before every PSF_ERR_UNSUPPORTED; *nbytes = ceil(len d / 8)
psf_status check_bytes(int kind, uint64_t q, uint32_t d, size_t len, const void* vals, const void* bytes, int io_bits, size_t* nbytes) {
  if (d < 1 || (io_bits != 16 && io_bits != 64)) return PSF_ERR_PARAM;
  if (len && (!vals || !bytes)) return PSF_ERR_PARAM;
  const size_t wb = (size_t)io_bits / 8;
  if (len > SIZE_MAX / d || len > SIZE_MAX / wb) return PSF_ERR_PARAM;
  *nbytes = len * d / 8 + (len * d % 8 != 0);
  if (overlap(vals, len * wb, bytes, *nbytes)) return PSF_ERR_PARAM;
  if (kind == BY_DECODE && q == 1) return PSF_ERR_PARAM;
  if ((kind == BY_COMPRESS_ENCODE || kind == BY_DECODE_DECOMPRESS) && q < 2) return PSF_ERR_PARAM;
  if (d > 63 || (io_bits == 16 && d > 16)) return PSF_ERR_UNSUPPORTED;
  if (kind != BY_ENCODE && ((io_bits == 16 && q > (1ull << 16)) || q >= (1ull << 62))) return PSF_ERR_UNSUPPORTED;
  return PSF_OK;
}

// the constants of a call: those of Compress_d / Decompress_d where q is used, d and its mask alone otherwise
CmpArgs make_byte_args(int kind, uint64_t q, uint32_t d) {
  if (q >= 2) return make_args(kind == BY_COMPRESS_ENCODE ? OP_COMPRESS : OP_DECOMPRESS, q, d);
  CmpArgs a{};
  a.d = d;
  a.mask = (1ull << d) - 1;
  return a;
}

// the launch of checked arguments on device buffers, in `stream`, nothing allocated.  `vals` is the value buffer (read by the two encodes,
// written by the two decodes), `bytes` the packed one.
psf_status bytes_dev(int kind, int device, uint64_t q, uint32_t d, size_t len, const void* vals, const void* bytes, size_t nbytes, int* flag, int io_bits,
                     hipStream_t st) {
  if (len == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int cus = device_cus(device);
  if (cus <= 0) return PSF_ERR_HIP;
  const size_t tv = (size_t)kTileVec * (io_bits == 16 ? 8 : 2);
  const bool pack = kind == BY_ENCODE || kind == BY_COMPRESS_ENCODE;
  const size_t ntiles = ((uintptr_t)vals % 16 == 0 && (uintptr_t)bytes % 16 == 0) ? len / tv : 0;     // whole tiles need both pointers 16-byte aligned
  const size_t tail = pack ? nbytes - ntiles * (tv / 8) * d : len - ntiles * tv;                          // bytes (pack) or values (unpack), one per lane
  const dim3 grid(grid_blocks(tail, ntiles, cus, pack ? 4 : 8));        // by LDS: 32 KiB (pack) or 16 KiB (unpack) per workgroup of 4 waves
  const CmpArgs a = make_byte_args(kind, q, d);
  const uint32_t md32 = 0xffffffffu / a.d;
  const uint64_t md64 = ~0ull / a.d;
  const int mode = kind == BY_DECODE_DECOMPRESS ? UNPACK_DECOMPRESS : q == 0 ? UNPACK_RAW : UNPACK_MODQ;
  if (mode != UNPACK_MODQ) flag = nullptr;
  for_int<16, 64>(io_bits, [&](auto io) {
    constexpr int IO = decltype(io)::value;
    if (pack) {
      for_int<0, 1>(kind == BY_COMPRESS_ENCODE, [&](auto fused) {
        hipLaunchKernelGGL((k_pack<decltype(fused)::value, IO>), grid, dim3(256), 0, st, a, md32, md64, vals, (uint8_t*)bytes, len, ntiles, nbytes);
      });
    } else {
      for_int<UNPACK_RAW, UNPACK_MODQ, UNPACK_DECOMPRESS>(mode, [&](auto m) {
        hipLaunchKernelGGL((k_unpack<decltype(m)::value, IO>), grid, dim3(256), 0, st, a, (const uint8_t*)bytes, (void*)vals, flag, len, ntiles);
      });
    }
  });
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// host-pointer form: copy in, run on the device (64-bit words), copy out.  No CPU fallback.
psf_status bytes_host(int kind, int device, uint64_t q, uint32_t d, size_t len, const void* vals, const void* bytes, size_t nbytes, int* noncanonical) {
  if (len == 0) return PSF_OK;
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  const bool pack = kind == BY_ENCODE || kind == BY_COMPRESS_ENCODE;
  const bool flagged = kind == BY_DECODE && q && noncanonical;
  const size_t vbytes = len * sizeof(uint64_t);
  DevBuf dvals, dbytes, dflag;
  HIP_TRY(dvals.alloc(vbytes));
  HIP_TRY(dbytes.alloc(nbytes));
  if (flagged) {
    HIP_TRY(dflag.alloc(sizeof(int)));
    HIP_TRY(dflag.zero(sizeof(int)));
  }
  if (pack) HIP_TRY(dvals.upload(vals, vbytes));
  else HIP_TRY(dbytes.upload(bytes, nbytes));
  const psf_status rc = bytes_dev(kind, device, q, d, len, dvals.as<void>(), dbytes.as<void>(), nbytes, dflag.as<int>(), 64, nullptr);
  if (rc != PSF_OK) return rc;
  if (pack) HIP_TRY(dbytes.download((void*)bytes, nbytes));
  else HIP_TRY(dvals.download((void*)vals, vbytes));
  if (flagged) {
    int f = 0;
    HIP_TRY(dflag.download(&f, sizeof(int)));
    if (f) *noncanonical |= 1;
  }
  return PSF_OK;
}

// the four byte forms behind their entry points: the checks, then the device form in `st` or (host) the host-pointer form
psf_status bytes_call(int kind, int device, uint64_t q, uint32_t d, size_t len, const void* vals, const void* bytes, int* flag, int io_bits, void* st,
                      bool host = false) {
  size_t nbytes = 0;
  const psf_status rc = check_bytes(kind, q, d, len, vals, bytes, io_bits, &nbytes);
  if (rc != PSF_OK) return rc;
  return host ? bytes_host(kind, device, q, d, len, vals, bytes, nbytes, flag)
              : bytes_dev(kind, device, q, d, len, vals, bytes, nbytes, flag, io_bits, (hipStream_t)st);
}

}  // namespace cmp
}  // namespace psf

using namespace psf::cmp;

extern "C" {

psf_status psf_lossy_compress(int device, uint64_t q, uint32_t d, size_t len, const uint64_t* x, int64_t* y) {
  return map_call(OP_COMPRESS, device, q, d, len, x, y, 64, nullptr, true);
}
psf_status psf_lossy_decompress(int device, uint64_t q, uint32_t d, size_t len, const int64_t* y, uint64_t* x) {
  return map_call(OP_DECOMPRESS, device, q, d, len, y, x, 64, nullptr, true);
}
psf_status psf_encode_digits(int device, uint64_t q, uint64_t base, size_t len, const uint64_t* digits, uint64_t* out) {
  return map_call(OP_ENCODE, device, q, base, len, digits, out, 64, nullptr, true);
}
psf_status psf_decode_digits(int device, uint64_t q, uint64_t base, size_t len, const uint64_t* coeffs, uint64_t* digits) {
  return map_call(OP_DECODE, device, q, base, len, coeffs, digits, 64, nullptr, true);
}
psf_status psf_lossy_compress_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_x, void* d_y, int io_bits, void* stream) {
  return map_call(OP_COMPRESS, device, q, d, len, d_x, d_y, io_bits, stream);
}
psf_status psf_lossy_decompress_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_y, void* d_x, int io_bits, void* stream) {
  return map_call(OP_DECOMPRESS, device, q, d, len, d_y, d_x, io_bits, stream);
}
psf_status psf_encode_digits_dev(int device, uint64_t q, uint64_t base, size_t len, const void* d_digits, void* d_out, int io_bits, void* stream) {
  return map_call(OP_ENCODE, device, q, base, len, d_digits, d_out, io_bits, stream);
}
psf_status psf_decode_digits_dev(int device, uint64_t q, uint64_t base, size_t len, const void* d_coeffs, void* d_digits, int io_bits, void* stream) {
  return map_call(OP_DECODE, device, q, base, len, d_coeffs, d_digits, io_bits, stream);
}

psf_status psf_byte_encode_dev(int device, uint32_t d, size_t len, const void* d_y, uint8_t* d_bytes, int io_bits, void* stream) {
  return bytes_call(BY_ENCODE, device, 0, d, len, d_y, d_bytes, nullptr, io_bits, stream);
}
psf_status psf_byte_decode_dev(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* d_bytes, void* d_y, int* d_noncanonical, int io_bits, void* stream) {
  return bytes_call(BY_DECODE, device, q, d, len, d_y, d_bytes, d_noncanonical, io_bits, stream);
}
psf_status psf_compress_encode_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_x, uint8_t* d_bytes, int io_bits, void* stream) {
  return bytes_call(BY_COMPRESS_ENCODE, device, q, d, len, d_x, d_bytes, nullptr, io_bits, stream);
}
psf_status psf_decode_decompress_dev(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* d_bytes, void* d_x, int io_bits, void* stream) {
  return bytes_call(BY_DECODE_DECOMPRESS, device, q, d, len, d_x, d_bytes, nullptr, io_bits, stream);
}
psf_status psf_byte_encode(int device, uint32_t d, size_t len, const int64_t* y, uint8_t* bytes) {
  return bytes_call(BY_ENCODE, device, 0, d, len, y, bytes, nullptr, 64, nullptr, true);
}
psf_status psf_byte_decode(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* bytes, int64_t* y, int* noncanonical) {
  return bytes_call(BY_DECODE, device, q, d, len, y, bytes, noncanonical, 64, nullptr, true);
}
psf_status psf_compress_encode(int device, uint64_t q, uint32_t d, size_t len, const uint64_t* x, uint8_t* bytes) {
  return bytes_call(BY_COMPRESS_ENCODE, device, q, d, len, x, bytes, nullptr, 64, nullptr, true);
}
psf_status psf_decode_decompress(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* bytes, uint64_t* x) {
  return bytes_call(BY_DECODE_DECOMPRESS, device, q, d, len, x, bytes, nullptr, 64, nullptr, true);
}

}  // extern "C"
