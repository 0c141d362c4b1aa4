// CPU model of the FIPS 203 interop of the NTT images (tools_amd/csrc/psf_ntt_fips.hpp, make_fips203_image_map of psf_host.cpp) at q = 3329, n = 256.
// Test infrastructure (built and run by tests/test_ntt_fips_model.py).  The forward transform, leaf product, inverse and finish are the templates of
// psf_ntt_core.hpp over the 64-lane host back end of ntt_model.cpp (every 24-bit multiply asserts its operand ranges); Algorithm 9 is written out
// here with zeta = 17.  Checked, for random and extreme f:
//   to(forward(f))                                  = Algorithm 9 (f)
//   finish(inverse(leafmul(from(Alg 9 (f)), forward(b)))) = the schoolbook product f b
//   from(to(image)) as the operand of the same product    = the same product
#define main ntt_model_main_unused                 // the host back end (HostWave, schoolbook, rnd) lives in the model of the transforms
#include "ntt_model.cpp"
#undef main
#include "../../tools_amd/csrc/psf_ntt_fips.hpp"

static const uint32_t Q = 3329;

static uint32_t bitrev7(uint32_t i) {
  uint32_t r = 0;
  for (int b = 0; b < 7; ++b) if (i & (1u << b)) r |= 1u << (6 - b);
  return r;
}
static uint32_t powmod(uint32_t b, uint32_t e) {
  uint64_t r = 1, x = b;
  for (; e; e >>= 1) { if (e & 1) r = r * x % Q; x = x * x % Q; }
  return (uint32_t)r;
}
// FIPS 203 Algorithm 9
static std::vector<uint32_t> fips_ntt(std::vector<uint32_t> f) {
  int i = 1;
  for (int len = 128; len >= 2; len /= 2)
    for (int start = 0; start < 256; start += 2 * len) {
      const uint32_t z = powmod(17, bitrev7((uint32_t)i++));
      for (int j = start; j < start + len; ++j) {
        const uint32_t t = (uint32_t)((uint64_t)z * f[j + len] % Q);
        f[j + len] = (f[j] + Q - t) % Q;
        f[j] = (f[j] + t) % Q;
      }
    }
  return f;
}

// the word maps with the operand ranges of their 24-bit multiply asserted
static void chk_mul(long long a, long long b) {
  if (a < -(1ll << 23) || a >= (1ll << 23) || b < -(1ll << 23) || b >= (1ll << 23) || std::llabs(a * b) + (3329ll << 15) >= (1ll << 31)) {
    std::fprintf(stderr, "interop multiply out of range: %lld * %lld\n", a, b);
    std::abort();
  }
}
static uint32_t word_from(const FipsImageMap& m, uint32_t v) { chk_mul(m.c_from, v); return fips_word_from(v, m.q, m.qinv16, m.c_from); }
static uint32_t word_to(const FipsImageMap& m, uint32_t x) { chk_mul(m.c_to, (int32_t)x); return fips_word_to(x, m.q, m.qinv16, m.c_to); }

using W = HostWave;
using M = Mod16D<W>;
using BD = Bounds16<12, 8, 1>;
using K = Core<W, M, BD, 8, 1>;
typedef M::V Regs[4];

struct Ctx {
  NttPlan pl;
  NttTables tb;
  M md;
  const uint32_t *zf, *zi;
};

static void to_regs(const std::vector<uint32_t>& words, Regs& x) {
  for (int r = 0; r < 4; ++r)
    for (int l = 0; l < 64; ++l) x[r].v[l] = (int32_t)words[r * 64 + l];
}
static std::vector<uint32_t> image_of(const Ctx& c, const std::vector<uint32_t>& f) {
  Regs x;
  to_regs(f, x);
  K::forward(x, c.md, c.zf, W::lane());
  std::vector<uint32_t> w(256);
  for (int r = 0; r < 4; ++r)
    for (int l = 0; l < 64; ++l) {
      if (std::abs(x[r].v[l]) > BD::r.xf) { std::fprintf(stderr, "forward output above xf\n"); std::abort(); }
      w[r * 64 + l] = (uint32_t)x[r].v[l];
    }
  return w;
}
static std::vector<uint64_t> product(const Ctx& c, const std::vector<uint32_t>& image, const std::vector<int64_t>& b) {
  Regs a, y, p;
  to_regs(image, a);
  for (int r = 0; r < 4; ++r)
    for (int l = 0; l < 64; ++l) y[r].v[l] = (int32_t)(b[r * 64 + l] % (int64_t)Q);
  K::forward(y, c.md, c.zf, W::lane());
  K::leafmul(p, a, y, c.md, c.zf, W::lane());
  K::inverse(p, c.md, c.zi, W::lane());
  K::finish(p, c.md, M::V((int32_t)ntt_final_scale(c.tb, c.pl, 1 + 2 * BD::r.nrf + BD::r.nri)));
  std::vector<uint64_t> out(256);
  for (int r = 0; r < 4; ++r)
    for (int l = 0; l < 64; ++l) out[r * 64 + l] = (uint64_t)(int64_t)p[r].v[l];
  return out;
}

static int run_case(const Ctx& c, const FipsImageMap& m, const char* name, const std::vector<uint32_t>& f, const std::vector<int64_t>& b) {
  const std::vector<uint32_t> want_hat = fips_ntt(f);
  const std::vector<uint32_t> img = image_of(c, f);
  int bad_to = 0, bad_from = 0, bad_round = 0;
  std::vector<uint32_t> got_hat(256), img2(256), img3(256);
  for (int k = 0; k < 256; ++k) {
    got_hat[k] = word_to(m, img[m.word_of[k]]);
    bad_to += got_hat[k] != want_hat[k];
  }
  for (int w = 0; w < 256; ++w) {
    img2[w] = word_from(m, want_hat[m.fips_of[w]]);
    if (std::abs((int32_t)img2[w]) >= (int32_t)Q) { std::fprintf(stderr, "from: word outside (-q, q)\n"); std::abort(); }
    img3[w] = word_from(m, word_to(m, img[w]));
  }
  const std::vector<uint64_t> fa(f.begin(), f.end());
  const std::vector<uint64_t> want = schoolbook(fa, b, Q);
  const std::vector<uint64_t> got2 = product(c, img2, b), got3 = product(c, img3, b);
  for (int i = 0; i < 256; ++i) { bad_from += got2[i] != want[i]; bad_round += got3[i] != want[i]; }
  std::printf("%s: to %d, from %d, from(to) %d mismatches: %s\n", name, bad_to, bad_from, bad_round, bad_to + bad_from + bad_round ? "FAIL" : "ok");
  return bad_to + bad_from + bad_round != 0;
}

int main() {
  Ctx c;
  c.pl = make_ntt_plan(Q, 256);
  c.tb = make_ntt_tables(c.pl);
  const FipsImageMap m = make_fips203_image_map();
  if (!c.pl.ok || !c.tb.wave || c.tb.qb != 12 || !m.ok) { std::printf("no plan or no map\n"); return 1; }
  c.md.q = (int)Q; c.md.nq = -(int)Q; c.md.qinv = c.tb.qinv16; c.md.zoff = 2 << c.pl.L;
  c.zf = c.tb.zetas.data();
  c.zi = c.zf + (1u << c.pl.L);
  // the map is a permutation of whole leaves
  int perm_bad = 0;
  bool hit[256] = {};
  for (int k = 0; k < 256; ++k) { hit[m.word_of[k]] = true; perm_bad += m.fips_of[m.word_of[k]] != k; }
  for (int w = 0; w < 256; ++w) perm_bad += !hit[w];
  std::printf("zeta = %llu, nrf = %d, c_from = %d, c_to = %d; FIPS 203 leaf of image leaf 0 ... 7:", (unsigned long long)c.pl.zetas[1 << (c.pl.L - 1)], BD::r.nrf, m.c_from, m.c_to);
  for (int g = 0; g < 8; ++g) {
    const int p = 2 * g, word = Sched<8>::reg_of_nat(p & 3) * 64 + (p >> 2);
    std::printf(" %d", m.fips_of[word] / 2);
  }
  std::printf("\n");
  int bad = perm_bad != 0;
  std::vector<int64_t> b(256), bx(256);
  for (int i = 0; i < 256; ++i) { b[i] = (int64_t)(rnd() % (2 * Q - 1)) - (int64_t)(Q - 1); bx[i] = (i & 1) ? (int64_t)Q - 1 : -((int64_t)Q - 1); }
  for (int t = 0; t < 8; ++t) {
    std::vector<uint32_t> f(256);
    for (auto& v : f) v = (uint32_t)(rnd() % Q);
    bad += run_case(c, m, "random", f, t & 1 ? bx : b);
  }
  bad += run_case(c, m, "all 0", std::vector<uint32_t>(256, 0), b);
  bad += run_case(c, m, "all q-1", std::vector<uint32_t>(256, Q - 1), bx);
  bad += run_case(c, m, "all q-1, random b", std::vector<uint32_t>(256, Q - 1), b);
  for (int pos : {0, 1, 2, 127, 128, 254, 255}) {
    std::vector<uint32_t> f(256, 0);
    f[pos] = pos & 1 ? Q - 1 : 1;
    bad += run_case(c, m, "unit vector", f, bx);
  }
  std::printf("NTT_FIPS_MODEL %s\n", bad ? "FAIL" : "OK");
  return bad != 0;
}
