// The SHA-2 core of the library (tools_amd/csrc/psf_sha2_core.hpp) on the CPU: the same text the device kernels compile, over the plain C++ back end.
// Test infrastructure, driven by tests/test_sha2_cpu.py, which also builds it with -fsanitize=address,undefined.  One case per line of the file named on
// the command line; <func> is 0 (SHA-256) or 1 (SHA-512) as in include/psf_mi355x.h, "-" is the empty string:
//   hash <func> <message hex> <off>            -> the digest, hex; the message sits `off` bytes past a 16-byte boundary (0: the 4-byte loads)
//   mid <func> <prefix hex> <rest hex>         -> the digest of prefix || rest, the prefix (whole blocks) compressed first and the rest absorbed from that
//                                                 midstate
// A message lives in a heap block that ends with its last byte, so a read past the end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_sha2_core.hpp"

using namespace psf::sha2;

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
// the bytes at `off` past a 16-byte boundary (malloc's alignment), in a block of exactly off + size bytes
struct Placed {
  uint8_t* block;
  uint8_t* p;
  Placed(const std::vector<uint8_t>& v, size_t off) : block(static_cast<uint8_t*>(std::malloc(off + v.size() + (off + v.size() == 0 ? 1 : 0)))), p(block + off) {
    if (!v.empty()) std::memcpy(p, v.data(), v.size());
  }
  ~Placed() { std::free(block); }
};

static void digest(int func, const uint8_t* p, size_t len, bool aligned) {
  uint8_t out[64];
  if (func == 0) {
    uint32_t h[8];
    init256(h);
    absorb256<PlainOps>(h, PtrReader{p, aligned}, len, 0);
    put_digest256(h, out, 32);
    print_hex(out, 32);
  } else {
    uint64_t h[8];
    init512(h);
    absorb512<PlainOps>(h, PtrReader{p, aligned}, len, 0);
    put_digest512(h, out, 64);
    print_hex(out, 64);
  }
}

static int from_mid(int func, const std::vector<uint8_t>& pre, const std::vector<uint8_t>& rest) {
  const size_t block = func == 0 ? 64 : 128;
  if (pre.size() % block != 0) return 2;
  uint8_t out[64];
  const PtrReader rp{pre.data(), false}, rr{rest.data(), false};
  if (func == 0) {
    uint32_t h[8], w[16];
    init256(h);
    for (size_t off = 0; off < pre.size(); off += 64) {
      for (int i = 0; i < 16; ++i) w[i] = rp.be32(off + 4 * i);
      compress256<PlainOps>(h, w);
    }
    absorb256<PlainOps>(h, rr, rest.size(), pre.size());
    put_digest256(h, out, 32);
    print_hex(out, 32);
  } else {
    uint64_t h[8], w[16];
    init512(h);
    for (size_t off = 0; off < pre.size(); off += 128) {
      for (int i = 0; i < 16; ++i) w[i] = ((uint64_t)rp.be32(off + 8 * i) << 32) | rp.be32(off + 8 * i + 4);
      compress512<PlainOps>(h, w);
    }
    absorb512<PlainOps>(h, rr, rest.size(), pre.size());
    put_digest512(h, out, 64);
    print_hex(out, 64);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream is(line);
    std::string cmd;
    int func = -1;
    if (!(is >> cmd >> func)) continue;
    if (func != 0 && func != 1) return 2;
    if (cmd == "hash") {
      std::string a;
      size_t off = 0;
      is >> a >> off;
      const Placed m(unhex(a), off);
      digest(func, m.p, unhex(a).size(), off % 4 == 0);
    } else if (cmd == "mid") {
      std::string a, b;
      is >> a >> b;
      const int rc = from_mid(func, unhex(a), unhex(b));
      if (rc) return rc;
    } else {
      return 2;
    }
  }
  return 0;
}
