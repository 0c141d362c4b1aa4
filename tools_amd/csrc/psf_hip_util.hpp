// psf_hip_util.hpp -- what the host side of every HIP translation unit shares: the error macro, the device check, the compute-unit count, the
// owners of device arrays, pinned arrays, streams and events (every hipFree, hipHostFree, hipStreamDestroy and hipEventDestroy of a handle's or a call's resources is
// here), the dynamic-LDS limit of a kernel, and the dispatch of a runtime integer to a template argument.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/psf_mi355x.h"
#include "psf_owned.hpp"

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess) {                                                           \
      std::fprintf(stderr, "[psf_mi355x] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return PSF_ERR_HIP;                                                              \
    }                                                                                  \
  } while (0)

namespace psf {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));              // one 16-byte load or store of a lane

// compute units of a device, queried once
inline int device_cus(int device) {
  static std::mutex mu;
  static int cus[64] = {0};
  if (device < 0 || device >= 64) return 0;
  std::lock_guard<std::mutex> lk(mu);
  if (!cus[device] && hipDeviceGetAttribute(&cus[device], hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus[device] = 0;
  return cus[device];
}

// makes `device` current; PSF_ERR_HIP when there is no such device (no CPU fallback)
inline psf_status use_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return PSF_ERR_HIP;
  HIP_TRY(hipSetDevice(device));
  return PSF_OK;
}

// a launch of `kern` with `smem` bytes of dynamic LDS: above the default 64 KiB the kernel's limit is raised to the 160 KiB of a gfx950 workgroup, once per
// process, kernel and device (`device` is current)
inline psf_status raise_lds_once(const void* kern, int device, size_t smem) {
  if (smem <= 64 * 1024) return PSF_OK;
  static std::mutex mu; static std::vector<std::pair<const void*, int>> raised;
  std::lock_guard<std::mutex> lk(mu);
  if (std::find(raised.begin(), raised.end(), std::make_pair(kern, device)) == raised.end()) {
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    raised.emplace_back(kern, device);
  }
  return PSF_OK;
}

// What a handle or a call holds, released when its owner dies (psf_owned.hpp): members in reverse order of declaration, after the destructor's body.
// DevArr / PinArr: alloc(count, slack_bytes) and grow(need, slack_bytes) return the runtime's code, for HIP_TRY; Stream / Event: hipEventCreate(ev.put()).
// A raw pointer, stream or event in a struct beside these is NOT owned by it.
inline hipError_t dev_acquire(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pin_acquire(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
template <class T> using DevArr = OwnedArr<T, dev_acquire, hipFree>;
template <class T> using PinArr = OwnedArr<T, pin_acquire, hipHostFree>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// untyped device memory that lives for one call: freed on every exit of the scope.  The operations return the runtime's code, for HIP_TRY.
class DevBuf {
 public:
  hipError_t alloc(size_t bytes) { return p_.alloc(bytes); }
  hipError_t upload(const void* src, size_t bytes) { return hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice); }
  hipError_t download(void* dst, size_t bytes) const { return hipMemcpy(dst, p_, bytes, hipMemcpyDeviceToHost); }
  hipError_t zero(size_t bytes) { return hipMemset(p_, 0, bytes); }
  template <class T> T* as() const { return reinterpret_cast<T*>(p_.get()); }

 private:
  DevArr<unsigned char> p_;
};

// a runtime integer as a template argument: f(ic<V>{}) for the V of the list that equals v; false when none does
template <int V> using ic = std::integral_constant<int, V>;
template <int... Vs, class F> bool for_int(int v, F&& f) { return ((v == Vs && (f(ic<Vs>{}), true)) || ...); }

}  // namespace psf
