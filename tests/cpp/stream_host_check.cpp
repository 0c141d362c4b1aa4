// stream_host_check.cpp -- sweep of tools_amd/csrc/psf_stream_host.hpp (plain C++, built with -fsanitize=address,undefined by
// tests/test_cpp_mirror.py): every input and output address modulo 16, words of 2 and 8 bytes, every length 0..40, against the formulas the
// launches used before the header existed (written out below as plain arithmetic) and against the invariants the kernels rely on.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "../../tools_amd/csrc/psf_stream_host.hpp"

static long checks = 0;
#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    ++checks;                                                                                           \
    if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, what); return 1; }         \
  } while (0)

int main() {
  char what[160];
  const uintptr_t base = (uintptr_t)1 << 20;                             // addresses only: nothing is dereferenced
  for (size_t wb : {(size_t)2, (size_t)8}) {
    const size_t epv = 16 / wb;
    for (size_t units : {epv, (size_t)3 * epv}) {                          // a 16-byte vector, and a larger unit that is a multiple of one (a tile)
      for (uintptr_t ai = 0; ai < 16; ++ai)
        for (uintptr_t ao = 0; ao < 16; ++ao)
          for (size_t len = 0; len <= 40; ++len) {
            const uintptr_t pi = base + ai, po = base + ao;
            std::snprintf(what, sizeof what, "wb %zu unit %zu in%%16 %zu out%%16 %zu len %zu", wb, units, (size_t)ai, (size_t)ao, len);
            // one pointer (the fills): head words up to the boundary, then whole units
            size_t h1 = ((16 - pi % 16) % 16) / wb;
            if (h1 > len) h1 = len;
            const size_t n1 = (len - h1) / units;
            REQUIRE(psf::head_words(pi, wb, len) == h1);
            const psf::StreamSplit s1 = psf::split_stream(pi, wb, len, units);
            REQUIRE(s1.head == h1 && s1.nvec == n1);
            REQUIRE(s1.head <= len && s1.head + s1.nvec * units <= len);
            if (pi % wb == 0) {
              REQUIRE(len - s1.head - s1.nvec * units < units);
              if (s1.nvec > 0) REQUIRE((pi + s1.head * wb) % 16 == 0);
            }
            // an input and an output that move together (the coefficient maps)
            size_t h2 = len, n2 = 0;
            if (pi % wb == 0 && pi % 16 == po % 16) {
              h2 = ((16 - pi % 16) % 16) / wb;
              if (h2 > len) h2 = len;
              n2 = (len - h2) / units;
            }
            const psf::StreamSplit s2 = psf::split_stream_pair(pi, po, wb, len, units);
            REQUIRE(s2.head == h2 && s2.nvec == n2);
            REQUIRE(s2.head <= len && s2.head + s2.nvec * units <= len);
            if (s2.nvec > 0) {
              REQUIRE((pi + s2.head * wb) % 16 == 0 && (po + s2.head * wb) % 16 == 0);
              REQUIRE(len - s2.head - s2.nvec * units < units);
            }
            const bool together = pi % wb == 0 && po % wb == 0 && pi % 16 == po % 16;
            if (!together) REQUIRE(s2.head == len && s2.nvec == 0);
          }
    }
  }
  // workgroups: ceil(work / 256), at least min_blocks, between 1 and per_cu on each of the cus units
  for (int cus : {1, 3, 256})
    for (int per_cu : {4, 8})
      for (size_t min_blocks : {(size_t)0, (size_t)1, (size_t)5, (size_t)4000})
        for (size_t work : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)3000, (size_t)524288, (size_t)524289, (size_t)1 << 40}) {
          std::snprintf(what, sizeof what, "cus %d per_cu %d min_blocks %zu work %zu", cus, per_cu, min_blocks, work);
          size_t want = (work + 255) / 256;
          if (want < min_blocks) want = min_blocks;
          const size_t cap = (size_t)cus * per_cu;
          want = want < 1 ? 1 : want > cap ? cap : want;
          const size_t blocks = psf::grid_blocks(work, min_blocks, cus, per_cu);
          REQUIRE(blocks == want);
          REQUIRE(blocks >= 1 && blocks <= std::max<size_t>(1, cap));
          REQUIRE(blocks >= std::min(min_blocks, cap));
          if (blocks < cap) REQUIRE(blocks * 256 >= work);
        }
  std::printf("STREAM_HOST_OK %ld checks\n", checks);
  return 0;
}
