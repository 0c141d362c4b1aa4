// psf_call_host.hpp -- the HIP-free half of psf_call.hpp: what every bytes-in, bytes-out entry point does with its arguments before anything runs.  The
// workspace layout, the spans of strided buffers, and the argument checks in the order include/psf_mi355x.h documents: NULL pointers, [strides: the
// caller's own rules], byte counts, the workspace size, the workspace (device forms), overlaps.  Plain C++: tests/cpp/call_host_check.cpp compiles this
// text with g++ (tests/test_call_checks_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/psf_mi355x.h"
#include "psf_host.hpp"

#define PSF_TRY(expr)                      \
  do {                                     \
    const psf_status rc__ = (expr);        \
    if (rc__ != PSF_OK) return rc__;       \
  } while (0)

namespace psf {

// ---- the workspace ---------------------------------------------------------------------------------------------------------------------------------
// The workspace of an operation: sections in a fixed order, each rounded up to 256 bytes.  A unit's workspace struct derives from Layout and adds the
// offsets of its sections; ok = false: the size does not fit size_t.
struct Layout {
  size_t total = 0;
  bool ok = true;
  size_t take(u128 bytes) {
    const size_t at = total;
    const u128 end = (u128)total + ((bytes + 255) / 256) * 256;
    if (end > (u128)SIZE_MAX) { ok = false; return 0; }
    total = (size_t)end;
    return at;
  }
};
template <class T> T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(ws) + off); }

// ---- the buffers of a call -------------------------------------------------------------------------------------------------------------------------
// `count` items of `len` bytes, item c at base + c stride (stride 0: one item): the bytes from the first of item 0 to the last of the last item;
// false: the span or its end address does not fit size_t
inline bool span_of(const void* base, size_t count, size_t len, size_t stride, size_t* span) {
  *span = 0;
  if (count == 0 || len == 0) return true;
  if (stride && count - 1 > (SIZE_MAX - len) / stride) return false;
  *span = (count - 1) * stride + len;
  return *span <= SIZE_MAX - (uintptr_t)base;
}
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (na == 0 || nb == 0) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
// a buffer of a call: `count` items of `len` bytes at `stride`; ok_null: may be NULL (an empty message, d_why); span: filled in by check_spans
struct Buf { const void* p; size_t len, stride; bool out, ok_null; size_t span; };

inline psf_status check_null(const Buf* b, int nb) {
  for (int i = 0; i < nb; ++i)
    if (!b[i].p && !b[i].ok_null) return PSF_ERR_PARAM;
  return PSF_OK;
}
inline psf_status check_spans(size_t count, Buf* b, int nb) {
  for (int i = 0; i < nb; ++i)
    if (!span_of(b[i].p, count, b[i].len, b[i].stride, &b[i].span)) return PSF_ERR_PARAM;
  return PSF_OK;
}
inline psf_status check_ws(bool dev, const void* ws, size_t ws_bytes, size_t need) {
  return dev && (!ws || (uintptr_t)ws % 256 != 0 || ws_bytes < need) ? PSF_ERR_PARAM : PSF_OK;       // the host forms allocate their own
}
// no output may touch another buffer or the workspace; a NULL buffer (ok_null) touches nothing
inline psf_status check_overlaps(const Buf* b, int nb, bool dev, const void* ws, size_t need) {
  for (int i = 0; i < nb; ++i) {
    if (!b[i].out || !b[i].p) continue;
    for (int j = 0; j < nb; ++j)
      if (j != i && b[j].p && overlap(b[i].p, b[i].span, b[j].p, b[j].span)) return PSF_ERR_PARAM;
    if (dev && overlap(b[i].p, b[i].span, ws, need)) return PSF_ERR_PARAM;
  }
  return PSF_OK;
}
// what follows check_null and the caller's stride rules, `need` being the workspace of the operation (Layout{}: none)
inline psf_status check_rest(size_t count, Buf* b, int nb, const Layout& need, bool dev, const void* ws, size_t ws_bytes) {
  PSF_TRY(check_spans(count, b, nb));
  if (!need.ok) return PSF_ERR_PARAM;
  PSF_TRY(check_ws(dev, ws, ws_bytes, need.total));
  return check_overlaps(b, nb, dev, ws, need.total);
}

}  // namespace psf
