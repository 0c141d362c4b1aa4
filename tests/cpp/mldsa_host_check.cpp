// The FIPS 204 core of the library (tools_amd/csrc/psf_mldsa_core.hpp) on the CPU: the same text the device kernels compile, over the plain C++
// back end.  Test infrastructure (built with -fsanitize=address,undefined and driven by tests/test_mldsa_core_cpu.py).  One command per line on stdin:
//   ntt <34 bytes hex> <max_blocks>             -> fail flag and 256 coefficients (RejNTTPoly)
//   bounded <eta> <66 bytes hex> <max_blocks>   -> fail flag and 256 coefficients (RejBoundedPoly)
//   ball <tau> <c~ hex> <max_blocks>            -> fail flag and 256 coefficients (SampleInBall)
//   hint <k> <omega> <omega + k bytes hex>      -> ok flag and the k * 256 bits as hex masks (32 bytes per polynomial, bit j of byte j / 8)
//   round <r> ...                               -> for every r in [0, q): r1 r0 of Power2Round, r1 r0 of Decompose at both gamma2, UseHint(0 / 1, r) at both
//   pack <packing 0..7> <8 values>              -> the bytes of 8 fields, hex
//   unpack <packing 0..7> <bytes hex>           -> 8 values
// Inputs live in heap blocks of their exact size, so a read past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_mldsa_core.hpp"

namespace kc = psf::kc;
using kc::absorb; using kc::PlainOps; using kc::SeedReader; using kc::PtrReader; using kc::kDomShake; using kc::kRateShake128; using kc::kRateShake256;
using namespace psf::dsa;

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
static void print_poly(bool flag, const std::vector<int>& coef) {
  std::printf("%d", (int)flag);
  for (int v : coef) std::printf(" %d", v);
  std::printf("\n");
}
// a heap copy of exactly the bytes given
struct Exact {
  uint8_t* p;
  explicit Exact(const std::vector<uint8_t>& v) : p(static_cast<uint8_t*>(std::malloc(v.size() + (v.empty() ? 1 : 0)))) {
    if (!v.empty()) std::memcpy(p, v.data(), v.size());
  }
  ~Exact() { std::free(p); }
};

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd;
    if (!(is >> cmd)) continue;
    if (cmd == "ntt") {
      std::string hex;
      int max_blocks = 0;
      is >> hex >> max_blocks;
      const std::vector<uint8_t> seed = unhex(hex);
      if (seed.size() != 34) return 2;
      const Exact in(seed);
      uint64_t s[25] = {0};
      absorb<kRateShake128, PlainOps>(s, SeedReader{in.p, 34, 0}, 34, kDomShake);
      std::vector<int> coef(256, -1);
      print_poly(rej_ntt_parse<PlainOps>(s, [&](uint32_t j, uint32_t v) { coef.at(j) = (int)v; }, max_blocks), coef);
    } else if (cmd == "bounded") {
      int eta = 0, max_blocks = 0;
      std::string hex;
      is >> eta >> hex >> max_blocks;
      const std::vector<uint8_t> seed = unhex(hex);
      if (seed.size() != 66 || (eta != 2 && eta != 4)) return 2;
      const Exact in(seed);
      uint64_t s[25] = {0};
      absorb<kRateShake256, PlainOps>(s, SeedReader{in.p, 64, (uint32_t)seed[64] | ((uint32_t)seed[65] << 8)}, 66, kDomShake);
      std::vector<int> coef(256, 99);
      auto put = [&](uint32_t j, int v) { coef.at(j) = v; };
      print_poly(eta == 2 ? rej_bounded_parse<2, PlainOps>(s, put, max_blocks) : rej_bounded_parse<4, PlainOps>(s, put, max_blocks), coef);
    } else if (cmd == "ball") {
      unsigned tau = 0;
      int max_blocks = 0;
      std::string hex;
      is >> tau >> hex >> max_blocks;
      const std::vector<uint8_t> ct = unhex(hex);
      if (tau < 1 || tau > 64) return 2;
      const Exact in(ct);
      uint64_t s[25] = {0};
      absorb<kRateShake256, PlainOps>(s, PtrReader{in.p, false}, ct.size(), kDomShake);
      std::vector<int> coef(256, 0);
      print_poly(sample_in_ball_parse<PlainOps>(s, tau, [&](uint32_t j) { return coef.at(j); }, [&](uint32_t j, int v) { coef.at(j) = v; }, max_blocks), coef);
    } else if (cmd == "hint") {
      unsigned k = 0, omega = 0;
      std::string hex;
      is >> k >> omega >> hex;
      const std::vector<uint8_t> y = unhex(hex);
      if (y.size() != omega + k) return 2;
      const Exact in(y);
      std::vector<uint8_t> h(32 * k, 0);
      const bool ok = hint_bit_unpack([&](uint32_t pos) { return (uint32_t)in.p[pos]; }, k, omega,
                                      [&](uint32_t i, uint32_t j) { h.at(32 * i + (j >> 3)) |= (uint8_t)(1u << (j & 7)); });
      std::printf("%d ", (int)ok);
      print_hex(h.data(), h.size());
    } else if (cmd == "round") {
      unsigned long r = 0;
      bool first = true;
      while (is >> r) {
        if (r >= kQ) return 2;
        uint32_t p1, l1, h1;
        int32_t p0, l0, h0;
        power2round((uint32_t)r, p1, p0);
        decompose<kGamma2Low>((uint32_t)r, l1, l0);
        decompose<kGamma2High>((uint32_t)r, h1, h0);
        std::printf("%s%u %d %u %d %u %d %u %u %u %u", first ? "" : " ", p1, p0, l1, l0, h1, h0, use_hint<kGamma2Low>(0, (uint32_t)r),
                    use_hint<kGamma2Low>(1, (uint32_t)r), use_hint<kGamma2High>(0, (uint32_t)r), use_hint<kGamma2High>(1, (uint32_t)r));
        first = false;
      }
      std::printf("\n");
    } else if (cmd == "pack") {
      int which = -1;
      is >> which;
      if (which < 0 || which >= kPackings) return 2;
      const PackSpec sp = kPackTable[which];
      uint32_t f[8];
      for (int j = 0; j < 8; ++j) {
        long v = 0;
        is >> v;
        f[j] = value_to_field(sp.top, (int32_t)v);
      }
      std::vector<uint8_t> out((size_t)sp.bits, 0);
      const Exact dst(out);
      if (!for_bits(sp.bits, [&](auto b) { pack8<decltype(b)::value>(dst.p, f); })) return 2;
      print_hex(dst.p, (size_t)sp.bits);
    } else if (cmd == "unpack") {
      int which = -1;
      std::string hex;
      is >> which >> hex;
      if (which < 0 || which >= kPackings) return 2;
      const PackSpec sp = kPackTable[which];
      const std::vector<uint8_t> bytes = unhex(hex);
      if (bytes.size() != (size_t)sp.bits) return 2;
      const Exact src(bytes);
      uint32_t f[8];
      if (!for_bits(sp.bits, [&](auto b) { unpack8<decltype(b)::value>(src.p, f); })) return 2;
      for (int j = 0; j < 8; ++j) std::printf(j ? " %d" : "%d", field_to_value(sp.top, f[j]));
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
