// The Keccak core of the library (tools_amd/csrc/psf_keccak_core.hpp) on the CPU: the same text the device kernels compile, over the plain C++ back
// end.  Test infrastructure (built with -fsanitize=address,undefined and driven by tests/test_keccak_cpu.py).  One command per line on stdin:
//   hash <func 0..3> <message hex | -> <out_len> [offset]   -> digest hex     (offset: the message and the digest start that many bytes past an
//                                                                              8-byte boundary; 0 takes the aligned path of the reader and writer)
//   ntt <34 bytes hex> <max_blocks>                         -> fail flag and 256 coefficients
//   cbd <eta> <32 bytes hex> <N>                            -> 256 coefficients
// Message and digest live in heap blocks of their exact size, so a read or write past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_keccak_core.hpp"

using namespace psf::kc;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> v;
  if (h == "-") return v;
  for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static void print_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
  std::printf("\n");
}

// a block whose byte `off` is the first of `n` usable bytes and whose last usable byte is the last byte of the allocation
struct Block {
  uint8_t* base;
  uint8_t* p;
  Block(size_t n, size_t off) {
    void* m = nullptr;
    if (posix_memalign(&m, 8, off + n + (n + off == 0))) std::abort();
    base = static_cast<uint8_t*>(m);
    p = base + off;
  }
  ~Block() { std::free(base); }
};

template <int RATE> static void run_hash(uint32_t dom, const std::vector<uint8_t>& msg, size_t out_len, size_t off) {
  Block in(msg.size(), off), out(out_len, off);
  if (!msg.empty()) std::memcpy(in.p, msg.data(), msg.size());
  hash<RATE, PlainOps>(PtrReader{in.p, off == 0}, msg.size(), dom, PtrWriter{out.p, off == 0}, out_len);
  print_hex(out.p, out_len);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd;
    if (!(is >> cmd)) continue;
    if (cmd == "hash") {
      int func = 0;
      std::string hex;
      size_t out_len = 0, off = 0;
      is >> func >> hex >> out_len;
      if (!(is >> off)) off = 0;
      const std::vector<uint8_t> msg = unhex(hex);
      if (func == 0) run_hash<kRateSha3_256>(kDomSha3, msg, out_len, off);
      else if (func == 1) run_hash<kRateSha3_512>(kDomSha3, msg, out_len, off);
      else if (func == 2) run_hash<kRateShake128>(kDomShake, msg, out_len, off);
      else if (func == 3) run_hash<kRateShake256>(kDomShake, msg, out_len, off);
      else return 2;
    } else if (cmd == "ntt") {
      std::string hex;
      int max_blocks = 0;
      is >> hex >> max_blocks;
      const std::vector<uint8_t> seed = unhex(hex);
      if (seed.size() != 34) return 2;
      Block in(34, 3);
      std::memcpy(in.p, seed.data(), 34);
      uint64_t s[25] = {0};
      absorb<kRateShake128, PlainOps>(s, SeedReader{in.p, 34, 0}, 34, kDomShake);
      std::vector<int> coef(256, -1);
      const bool fail = sample_ntt_parse<PlainOps>(s, [&](uint32_t j, uint32_t v) { coef.at(j) = (int)v; }, max_blocks);
      std::printf("%d", (int)fail);
      for (int v : coef) std::printf(" %d", v);
      std::printf("\n");
    } else if (cmd == "cbd") {
      int eta = 0;
      std::string hex;
      unsigned nonce = 0;
      is >> eta >> hex >> nonce;
      const std::vector<uint8_t> sigma = unhex(hex);
      if (sigma.size() != 32 || (eta != 2 && eta != 3)) return 2;
      Block in(32, 1);
      std::memcpy(in.p, sigma.data(), 32);
      std::vector<int> coef(256, 99);
      auto put = [&](uint32_t j, int v) { coef.at(j) = v; };
      const SeedReader rd{in.p, 32, nonce};
      if (eta == 2) { uint64_t w[16]; prf_words<2, PlainOps>(rd, w); cbd_fields<2>(w, put); }
      else { uint64_t w[24]; prf_words<3, PlainOps>(rd, w); cbd_fields<3>(w, put); }
      for (int i = 0; i < 256; ++i) std::printf(i ? " %d" : "%d", coef[i]);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
