// call_host_check.cpp -- the shared argument checks and workspace layout of tools_amd/csrc/psf_call_host.hpp as a stand-alone host program (no HIP).
// Reads one case per line from stdin, prints one line of results per case; tests/test_call_checks_cpu.py holds the expected answers, computed with
// unbounded integers.  Addresses are numbers only: nothing is ever read or written through them.
//   span BASE COUNT LEN STRIDE                      -> OK SPAN
//   overlap A NA B NB                               -> 0 | 1
//   take BYTES...                                   -> OK TOTAL OFFSET...
//   check COUNT DEV WS WS_BYTES NEED_OK NEED NB (P LEN STRIDE OUT OK_NULL)...
//        -> the codes of check_null, check_spans, check_ws, check_overlaps each on its own, the code of check_null followed by check_rest, and the spans
//           that run left in the buffers (they start at 7: a check that returned before check_spans leaves them there)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_call_host.hpp"

using namespace psf;

static u128 parse_u128(const std::string& s) {
  u128 v = 0;
  for (char ch : s) v = v * 10 + (u128)(ch - '0');
  return v;
}
static const void* addr(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "span") {
      uint64_t base = 0, count = 0, len = 0, stride = 0;
      in >> base >> count >> len >> stride;
      if (!in) { std::fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
      size_t span = 0;
      const bool ok = span_of(addr(base), count, len, stride, &span);
      std::printf("%d %zu\n", ok ? 1 : 0, span);
    } else if (what == "overlap") {
      uint64_t a = 0, na = 0, b = 0, nb = 0;
      in >> a >> na >> b >> nb;
      if (!in) { std::fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
      std::printf("%d\n", overlap(addr(a), na, addr(b), nb) ? 1 : 0);
    } else if (what == "take") {
      Layout l;
      std::vector<size_t> offs;
      std::string tok;
      while (in >> tok) offs.push_back(l.take(parse_u128(tok)));
      std::printf("%d %zu", l.ok ? 1 : 0, l.total);
      for (size_t o : offs) std::printf(" %zu", o);
      std::printf("\n");
    } else if (what == "check") {
      uint64_t count = 0, ws = 0, ws_bytes = 0, need_total = 0;
      int dev = 0, need_ok = 0, nb = 0;
      in >> count >> dev >> ws >> ws_bytes >> need_ok >> need_total >> nb;
      std::vector<Buf> b(nb);
      for (Buf& x : b) {
        uint64_t p = 0, len = 0, stride = 0;
        int out = 0, ok_null = 0;
        in >> p >> len >> stride >> out >> ok_null;
        x = Buf{addr(p), len, stride, out != 0, ok_null != 0, 7};
      }
      Layout need;
      need.ok = need_ok != 0;
      need.total = need_total;
      std::vector<Buf> each = b;
      const int r_null = check_null(each.data(), nb), r_spans = check_spans(count, each.data(), nb);
      const int r_ws = check_ws(dev != 0, addr(ws), ws_bytes, need_total), r_over = check_overlaps(each.data(), nb, dev != 0, addr(ws), need_total);
      int all = check_null(b.data(), nb);
      if (all == PSF_OK) all = check_rest(count, b.data(), nb, need, dev != 0, addr(ws), ws_bytes);
      if (!in) { std::fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
      std::printf("%d %d %d %d %d", r_null, r_spans, r_ws, r_over, all);
      for (const Buf& x : b) std::printf(" %zu", x.span);
      std::printf("\n");
    } else if (!what.empty()) {
      std::fprintf(stderr, "unknown case: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
