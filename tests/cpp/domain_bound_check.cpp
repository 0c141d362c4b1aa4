// psf::domain_bound_exact (tools_amd/csrc/psf_host.hpp: the bound check_domain hands its kernel) on the CPU, no HIP: reads lines "s r m" (hex floats and a
// decimal integer) and prints the three limbs of floor(s^2 m r^2), most significant first.  tests/test_check_domain_exact_cpu.py compares them with Python's
// Fraction.  Built with g++ -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include "../../tools_amd/csrc/psf_host.hpp"

int main() {
  char sb[64], rb[64];
  unsigned long long m;
  while (std::scanf("%63s %63s %llu", sb, rb, &m) == 3) {
    const psf::NormBound b = psf::domain_bound_exact(std::strtod(sb, nullptr), std::strtod(rb, nullptr), (uint64_t)m);
    std::printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "\n", b.w[2], b.w[1], b.w[0]);
  }
  return 0;
}
