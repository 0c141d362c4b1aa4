// psf_stream_host.hpp -- the host arithmetic of the one-pass kernels over flat arrays (psf_compress.hip, psf_sample.hip): where the 16-byte
// vectors of a buffer start, and how many workgroups of 256 lanes a pass gets.  Plain C++, no HIP: the sweep of tests/cpp/stream_host_check.cpp
// compiles it alone.  The helpers carry every policy as a parameter; which words go to vectors or tiles is the caller's choice.
#pragma once
#include <cstddef>
#include <cstdint>

namespace psf {

// words of wb bytes before the first 16-byte boundary at address p (at most len)
inline size_t head_words(uintptr_t p, size_t wb, size_t len) {
  const size_t h = ((16 - p % 16) % 16) / wb;
  return h < len ? h : len;
}

// words [0, head) one by one, then nvec units of `unit` words from a 16-byte boundary on, then the rest one by one
struct StreamSplit { size_t head, nvec; };

inline StreamSplit split_stream(uintptr_t p, size_t wb, size_t len, size_t unit) {
  const size_t head = head_words(p, wb, len);
  return StreamSplit{head, (len - head) / unit};
}

// an input and an output that move together: units only when both reach a 16-byte boundary after the same number of words
inline StreamSplit split_stream_pair(uintptr_t in, uintptr_t out, size_t wb, size_t len, size_t unit) {
  if (in % wb != 0 || in % 16 != out % 16) return StreamSplit{len, 0};
  return split_stream(in, wb, len, unit);
}

// workgroups of 256 lanes for `work` lanes' worth of items, at least min_blocks (one per tile, say), at most per_cu on each of the cus units
inline unsigned grid_blocks(size_t work, size_t min_blocks, int cus, int per_cu) {
  size_t blocks = (work + 255) / 256;
  if (blocks < min_blocks) blocks = min_blocks;
  const size_t cap = (size_t)cus * (size_t)per_cu;
  return (unsigned)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

}  // namespace psf
