// What signing adds to the FIPS 204 core of the library (tools_amd/csrc/psf_mldsa_core.hpp) on the CPU: the same text the device kernels compile,
// over the plain C++ back end.  Test infrastructure (built with -fsanitize=address,undefined and driven by tests/test_mldsa_sign_cpu.py).  One command
// per line on stdin:
//   mask <18|20> <66 bytes hex>                 -> the 256 coefficients of ExpandMask's polynomial for rho'' || le16(nonce)
//   bits <r> ...                                -> for every r in [0, q): HighBits LowBits at gamma2 = (q - 1) / 88, then at (q - 1) / 32
//   makehint <0|1> <r> <z> ...                  -> MakeHint(z, r) for pairs (r, z), z any residue; 0: the low gamma2, 1: the high one
//   norm <bound> <r> ...                        -> norm_reaches(r, bound) for residues r
//   low <bound> <r0> ...                        -> low_reaches(r0, bound) for signed r0
//   hintpack <k> <omega> <32 k bytes hex>       -> the omega + k bytes of HintBitPack of the masks (bit j of polynomial i: byte 32 i + j / 8, bit j % 8)
//   kappa <l> <kappa> ...                       -> kappa_exhausted(kappa, l)
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
using kc::absorb; using kc::PlainOps; using kc::SeedReader; using kc::kDomShake; using kc::kRateShake256;
using namespace psf::dsa;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> v;
  for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
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
    if (cmd == "mask") {
      int bits = 0;
      std::string hex;
      is >> bits >> hex;
      const std::vector<uint8_t> seed = unhex(hex);
      if (seed.size() != 66 || (bits != 18 && bits != 20)) return 2;
      const Exact in(seed);
      uint64_t s[25] = {0};
      absorb<kRateShake256, PlainOps>(s, SeedReader{in.p, 64, (uint32_t)seed[64] | ((uint32_t)seed[65] << 8)}, 66, kDomShake);
      std::vector<long> coef(256, 1L << 40);
      int puts = 0;
      auto put = [&](uint32_t j, int32_t v) { coef.at(j) = v; ++puts; };
      if (bits == 18) expand_mask_parse<18, PlainOps>(s, put);
      else expand_mask_parse<20, PlainOps>(s, put);
      if (puts != 256) return 3;
      for (int j = 0; j < 256; ++j) std::printf(j ? " %ld" : "%ld", coef[j]);
      std::printf("\n");
    } else if (cmd == "bits") {
      unsigned long r = 0;
      bool first = true;
      while (is >> r) {
        if (r >= kQ) return 2;
        std::printf("%s%u %d %u %d", first ? "" : " ", high_bits<kGamma2Low>((uint32_t)r), low_bits<kGamma2Low>((uint32_t)r), high_bits<kGamma2High>((uint32_t)r),
                    low_bits<kGamma2High>((uint32_t)r));
        first = false;
      }
      std::printf("\n");
    } else if (cmd == "makehint") {
      int high = 0;
      unsigned long r = 0, z = 0;
      bool first = true;
      is >> high;
      while (is >> r >> z) {
        if (r >= kQ || z >= kQ) return 2;
        const uint32_t sum = (uint32_t)((r + z) % kQ);
        std::printf("%s%u", first ? "" : " ", high ? make_hint<kGamma2High>((uint32_t)r, sum) : make_hint<kGamma2Low>((uint32_t)r, sum));
        first = false;
      }
      std::printf("\n");
    } else if (cmd == "norm" || cmd == "low") {
      unsigned long bound = 0;
      long v = 0;
      bool first = true;
      is >> bound;
      while (is >> v) {
        if (cmd == "norm" && (v < 0 || v >= (long)kQ)) return 2;
        std::printf("%s%u", first ? "" : " ", cmd == "norm" ? norm_reaches((uint32_t)v, (uint32_t)bound) : low_reaches((int32_t)v, (uint32_t)bound));
        first = false;
      }
      std::printf("\n");
    } else if (cmd == "hintpack") {
      unsigned k = 0, omega = 0;
      std::string hex;
      is >> k >> omega >> hex;
      const std::vector<uint8_t> h = unhex(hex);
      if (h.size() != 32 * k) return 2;
      const Exact in(h);
      const Exact out(std::vector<uint8_t>(omega + k, 0xEE));
      int puts = 0;
      hint_bit_pack([&](uint32_t i, uint32_t b) { return (uint32_t)in.p[32 * i + b]; }, k, omega, [&](uint32_t pos, uint32_t v) { out.p[pos] = (uint8_t)v; ++puts; });
      if (puts != (int)(omega + k)) return 3;
      for (size_t i = 0; i < omega + k; ++i) std::printf("%02x", out.p[i]);
      std::printf("\n");
    } else if (cmd == "kappa") {
      unsigned long l = 0, kap = 0;
      bool first = true;
      is >> l;
      while (is >> kap) {
        std::printf("%s%d", first ? "" : " ", (int)kappa_exhausted((uint32_t)kap, (uint32_t)l));
        first = false;
      }
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
