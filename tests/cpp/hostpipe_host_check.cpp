// hostpipe_host_check.cpp -- sweep of tools_amd/csrc/psf_hostpipe_host.hpp (plain C++, built with clang++ -fsanitize=address,undefined by
// tests/test_cpp_mirror.py): widen_rows at every alignment of source and destination and every length 0..40, the slice cuts of a host call, the chunk
// geometry with the slice a chunk waits for, and the pieces of a nearest-plane batch.  Every expectation is the obvious scalar loop, written out here.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <stdlib.h>
#include <vector>
#include "../../tools_amd/csrc/psf_hostpipe_host.hpp"

static long checks = 0;
#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    ++checks;                                                                                           \
    if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, what); return 1; }         \
  } while (0)

int main() {
  char what[200];

  // widen_rows: destination at both 8-byte offsets of a 16-byte line, source at all four 4-byte offsets; the source is sized exactly (a read past it is an ASan
  // report: its last entry ends the allocation), the word behind the destination must survive
  const int32_t special[4] = {INT32_MIN, INT32_MAX, -1, 0};
  const int64_t GUARD = 0x5a5a5a5a5a5a5a5aLL;
  for (size_t doff = 0; doff < 2; ++doff)
    for (size_t soff = 0; soff < 4; ++soff)
      for (size_t len = 0; len <= 40; ++len) {
        std::snprintf(what, sizeof what, "widen_rows dst+%zu src+%zu len %zu", doff * 8, soff * 4, len);
        void *sblock = nullptr, *dblock = nullptr;                        // 16-byte aligned blocks; the source block ends with src[len - 1]
        REQUIRE(posix_memalign(&sblock, 16, (soff + len) * sizeof(int32_t) + (soff + len ? 0 : 4)) == 0);
        REQUIRE(posix_memalign(&dblock, 16, (doff + len + 1) * sizeof(int64_t)) == 0);
        int32_t* src = static_cast<int32_t*>(sblock) + soff;
        int64_t* dst = static_cast<int64_t*>(dblock) + doff;
        REQUIRE((uintptr_t)src % 16 == soff * 4 && (uintptr_t)dst % 16 == doff * 8);
        for (size_t i = 0; i < len; ++i) src[i] = i < 8 ? special[(i + len) % 4] : (int32_t)((uint32_t)(i * 2654435761u) ^ (uint32_t)(len << 20));
        for (size_t i = 0; i < len; ++i) dst[i] = 7;
        dst[len] = GUARD;
        psf::widen_rows(dst, src, len);
        for (size_t i = 0; i < len; ++i) REQUIRE(dst[i] == (int64_t)src[i]);
        REQUIRE(dst[len] == GUARD);
        std::free(sblock);
        std::free(dblock);
      }
  // slice cuts, tail 1024
  const size_t tail = 1024;
  for (size_t B = 1; B <= 5000; ++B) {
    std::snprintf(what, sizeof what, "slices B %zu", B);
    const psf::HostSlices cut = psf::host_slices(B, tail, true, false, 0);
    if (B >= 2048) REQUIRE(cut.nsl == 2 && cut.cuts[0] == 0 && cut.cuts[1] == B - 1024 && cut.cuts[2] == B);
    else REQUIRE(cut.nsl == 1 && cut.cuts[0] == 0 && cut.cuts[1] == B);
    const psf::HostSlices plain = psf::host_slices(B, tail, false, false, 0);
    REQUIRE(plain.nsl == 1 && plain.cuts[0] == 0 && plain.cuts[1] == B);
    for (long v : {0L, 127L, 128L, 500L, 1024L, 4999L, 5000L})
      for (int ct = 0; ct < 2; ++ct) {
        const psf::HostSlices whole = psf::host_slices(B, tail, ct != 0, true, v);
        REQUIRE(whole.nsl == 1 && whole.cuts[0] == 0 && whole.cuts[1] == B);
        const psf::HostSlices f = psf::host_slices(B, tail, ct != 0, false, v);
        REQUIRE(f.nsl >= 1 && f.nsl <= 4 && f.cuts[0] == 0 && f.cuts[f.nsl] == B);
        for (int j = 0; j < f.nsl; ++j) REQUIRE(f.cuts[j] < f.cuts[j + 1]);
        if (v >= 128 && (size_t)v < B) {                                  // equal slices of v rows, the fourth takes what is left
          const size_t want = (B + (size_t)v - 1) / (size_t)v < 4 ? (B + (size_t)v - 1) / (size_t)v : 4;
          REQUIRE((size_t)f.nsl == want);
          for (int j = 0; j < f.nsl; ++j) REQUIRE(f.cuts[j] == (size_t)j * (size_t)v);
        } else {                                                          // not forced: the tail rule alone
          const psf::HostSlices t = psf::host_slices(B, tail, ct != 0, false, 0);
          REQUIRE(f.nsl == t.nsl);
          for (int j = 0; j <= f.nsl; ++j) REQUIRE(f.cuts[j] == t.cuts[j]);
        }
      }
  }

  // chunks: they tile [0, total) exactly; the slice a chunk waits for is the largest slice that holds one of its entries
  for (size_t CE : {(size_t)1, (size_t)7, (size_t)64, (size_t)1000})
    for (size_t mult = 1; mult <= 5; ++mult)
      for (size_t d = 0; d <= 2; ++d) {
        const size_t total = mult * CE + d - 1;                             // one entry short of a multiple of the chunk, the multiple, one beyond
        if (total == 0) continue;                                           // (no call has no entries)
        for (int nsl : {1, 2, 4}) {
          // slice ends: nsl increasing cuts, the last one at total; several placements, among them cuts on and next to chunk boundaries
          for (size_t variant = 0; variant < 6; ++variant) {
            if ((size_t)nsl > total) continue;
            size_t end[4];
            for (int j = 0; j < nsl; ++j) {
              size_t e = total * (size_t)(j + 1) / (size_t)nsl;
              if (j < nsl - 1) {
                if (variant == 1) e = e / CE * CE;                          // on a chunk boundary
                if (variant == 2) e = e / CE * CE + 1;
                if (variant == 3 && e / CE * CE > 0) e = e / CE * CE - 1;
                if (variant == 4) e = (size_t)(j + 1);                      // short first slices
                if (variant == 5) e = total - (size_t)(nsl - 1 - j);        // short last slices
              }
              end[j] = e;
            }
            bool increasing = end[0] > 0 && end[nsl - 1] == total;
            for (int j = 1; j < nsl; ++j) increasing = increasing && end[j] > end[j - 1];
            if (!increasing) continue;
            std::snprintf(what, sizeof what, "chunks CE %zu total %zu nsl %d variant %zu", CE, total, nsl, variant);
            const size_t nch = psf::host_chunks(total, CE);
            REQUIRE(nch == (total + CE - 1) / CE);
            size_t next = 0;
            for (size_t c = 0; c < nch; ++c) {
              const psf::HostSpan ch = psf::host_chunk(c, total, CE);
              REQUIRE(ch.b0 == next && ch.cnt >= 1 && ch.cnt <= CE);
              next = ch.b0 + ch.cnt;
              int want = -1;                                                // brute force: the slice of every entry of the chunk
              for (size_t i = ch.b0; i < ch.b0 + ch.cnt; ++i) {
                int j = 0;
                while (i >= end[j]) ++j;
                if (j > want) want = j;
              }
              REQUIRE(psf::host_chunk_slice(ch, end, nsl) == want);
            }
            REQUIRE(next == total);
          }
        }
      }

  // the four pieces of a nearest-plane batch: disjoint, ascending, from multiples of 16, covering [0, ne)
  std::vector<size_t> nes;
  for (size_t ne = 1; ne <= 300; ++ne) nes.push_back(ne);
  for (size_t ne : {((size_t)1 << 20) - 1, (size_t)1 << 20, ((size_t)1 << 20) + 1}) nes.push_back(ne);
  for (size_t ne : nes) {
    std::snprintf(what, sizeof what, "pieces ne %zu", ne);
    const size_t per = psf::host_piece_len(ne, 4);
    size_t want_per = (ne + 3) / 4;
    while (want_per % 16) ++want_per;
    REQUIRE(per == want_per);
    size_t next = 0;
    for (size_t i = 0; i < 4; ++i) {
      const psf::HostSpan pc = psf::host_piece(i, ne, per);
      REQUIRE(pc.b0 % 16 == 0);
      if (pc.cnt) { REQUIRE(pc.b0 == next && pc.b0 + pc.cnt <= ne); next = pc.b0 + pc.cnt; }
      else REQUIRE(next == ne && pc.b0 >= ne);                              // an empty piece only once everything is covered
    }
    REQUIRE(next == ne);
  }
  std::printf("HOSTPIPE_HOST_OK %ld checks\n", checks);
  return 0;
}
