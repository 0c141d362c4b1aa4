// psf_hostpipe_host.hpp -- the host arithmetic of the host-pointer transport (psf_hostpipe.hpp): the widening of int32 rows into the caller's int64 rows,
// where a host call is cut into slices, how its entries fall into chunks and which slice a chunk has to wait for, and the pieces of a nearest-plane batch.
// Plain C++, no HIP: the sweep of tests/cpp/hostpipe_host_check.cpp compiles it alone.  Every policy (tail length, forced slices, chunk size, piece count)
// comes in as a parameter; the environment switches behind them are read by the caller.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace psf {

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// int32 -> int64 into the caller's rows with streaming stores: the destination is written once and not read here, so there is no point in pulling its
// lines into the cache first (a plain loop moves 20 bytes per entry through the memory system, this one 12) -- the widening of a C3 batch is 1.5 GB of
// host memory traffic per call and has to fit under the next call's 60 ms on a handful of threads.
inline void widen_rows(int64_t* __restrict__ dst, const int32_t* __restrict__ src, size_t cnt) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef int v2i __attribute__((ext_vector_type(2)));
  typedef long long v2l __attribute__((ext_vector_type(2)));
  size_t i = 0;
  while (i < cnt && (reinterpret_cast<uintptr_t>(dst + i) & 15)) { dst[i] = (int64_t)src[i]; ++i; }
  for (; i + 4 <= cnt; i += 4) {
    v4i x;
    std::memcpy(&x, src + i, sizeof(x));
    const v2i a = __builtin_shufflevector(x, x, 0, 1), b = __builtin_shufflevector(x, x, 2, 3);
    __builtin_nontemporal_store(__builtin_convertvector(a, v2l), reinterpret_cast<v2l*>(dst + i));
    __builtin_nontemporal_store(__builtin_convertvector(b, v2l), reinterpret_cast<v2l*>(dst + i + 2));
  }
  for (; i < cnt; ++i) dst[i] = (int64_t)src[i];
  std::atomic_thread_fence(std::memory_order_seq_cst);      // (streaming stores are weakly ordered: fence before the thread reports its chunk done)
}

// The slices of a host call of B rows: slice j is the rows [cuts[j], cuts[j + 1]), nsl <= 4 of them.  cut_tail: everything but the last `tail` rows, then those
// (their transfer is all that remains exposed behind the last kernel; two slices cost the product ~4 ms, so only from 2 * tail rows on).  forced_rows >= 128:
// equal slices of that many rows instead (at most four; experiments).  whole_batch: never a cut.
struct HostSlices { int nsl; size_t cuts[5]; };
inline HostSlices host_slices(size_t B, size_t tail, bool cut_tail, bool whole_batch, long forced_rows) {
  HostSlices s{1, {0, B, B, B, B}};
  if (cut_tail && !whole_batch && B >= 2 * tail) { s.cuts[1] = B - tail; s.cuts[2] = B; s.nsl = 2; }
  if (forced_rows >= 128 && !whole_batch && (size_t)forced_rows < B) {
    s.nsl = 0;
    for (size_t off = 0; off < B && s.nsl < 4; off += (size_t)forced_rows) s.cuts[s.nsl++] = off;
    s.cuts[s.nsl] = B;
  }
  return s;
}

// entries [b0, b0 + cnt) of a flat array
struct HostSpan { size_t b0, cnt; };

// a call's `total` entries in chunks of `chunk` entries (the last one ragged)
inline size_t host_chunks(size_t total, size_t chunk) { return (total + chunk - 1) / chunk; }
inline HostSpan host_chunk(size_t c, size_t total, size_t chunk) {
  const size_t b0 = c * chunk;
  return HostSpan{b0, total - b0 < chunk ? total - b0 : chunk};
}
// the last slice a chunk touches (slice j ends in front of entry slice_end[j]): the chunk may cross PCIe once that slice's rows are complete
inline int host_chunk_slice(HostSpan ch, const size_t* slice_end, int nsl) {
  int j = 0;
  while (j < nsl - 1 && ch.b0 + ch.cnt > slice_end[j]) ++j;
  return j;
}

// the `pieces` pieces of a nearest-plane batch of ne entries: each a multiple of 16 entries (whole 64-byte lines of int32), the last ones short or empty
inline size_t host_piece_len(size_t ne, size_t pieces) { return round_up((ne + pieces - 1) / pieces, 16); }
inline HostSpan host_piece(size_t i, size_t ne, size_t per) {
  const size_t b0 = i * per;
  return HostSpan{b0, b0 >= ne ? 0 : (ne - b0 < per ? ne - b0 : per)};
}

}  // namespace psf
