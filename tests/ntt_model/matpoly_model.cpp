// CPU model of the accumulation step of the R_q matrix product (k_matpoly_mul): the templates of tools_amd/csrc/psf_ntt_core.hpp -- forward,
// leafmul, acc_add / acc_tick / acc_close, inverse, finish -- instantiated over a 64-lane array, for EVERY wave shape of for_shape (psf_ntt_shapes.hpp).
// Test infrastructure (built and run by tests/test_matpoly_model.py).  Each shape runs
//   * worst-case operands: a = q - 1 everywhere, b = +-(q - 1) by coefficient parity, the SAME summand `inner` = 4099 times (every leaf product of
//     one sign, the fastest growth of the accumulators), past the fold interval of the 16-bit form; and
//   * random operands: 37 different summands;
// for two accumulator rows at once, against a schoolbook sum.  Every 24-bit multiply and every Montgomery step asserts its operand ranges.
// The 64-lane wave back end is the one of tests/ntt_model/ntt_model.cpp.
#include <array>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>
#include "../../tools_amd/csrc/psf_host.hpp"
#include "../../tools_amd/csrc/psf_ntt_core.hpp"

using namespace psf;
using namespace psf::ntt;

template <class T> struct HV {
  std::array<T, 64> v;
  HV() { v.fill(0); }
  HV(T s) { v.fill(s); }
  template <class O> explicit HV(const HV<O>& o) { for (int l = 0; l < 64; ++l) v[l] = (T)o.v[l]; }
};
#define HV_OP(op)                                                                                              \
  template <class T> HV<T> operator op(const HV<T>& a, const HV<T>& b) { HV<T> r; for (int l = 0; l < 64; ++l) r.v[l] = (T)(a.v[l] op b.v[l]); return r; } \
  template <class T> HV<T> operator op(const HV<T>& a, T b) { HV<T> r; for (int l = 0; l < 64; ++l) r.v[l] = (T)(a.v[l] op b); return r; }
HV_OP(+) HV_OP(-) HV_OP(&)
static HV<int32_t> operator&(const HV<int32_t>& a, int b) { return a & HV<int32_t>(b); }
static HV<uint32_t> operator+(const HV<uint32_t>& a, int b) { return a + HV<uint32_t>((uint32_t)b); }

static long long g_max_prod = 0;
struct HostWave {
  using I = HV<int32_t>;
  using U = HV<uint32_t>;
  using Tab = const uint32_t*;
  static I lane() { I r; for (int l = 0; l < 64; ++l) r.v[l] = l; return r; }
  static I izero() { return I(0); }
  static U uzero() { return U(0u); }
  static I sra(I x, int s) { for (auto& e : x.v) e >>= s; return x; }
  static I srl(I x, int s) { for (auto& e : x.v) e = (int32_t)((uint32_t)e >> s); return x; }
  static I shl(I x, int s) { for (auto& e : x.v) e = (int32_t)((uint32_t)e << s); return x; }
  static I mont16(I t, int qinv, int nq) {
    for (auto& e : t.v) {
      const int16_t m = (int16_t)(uint16_t)((uint32_t)e * (uint32_t)qinv);
      const long long r = (long long)e + (long long)m * nq;
      if (r & 0xffff) { std::fprintf(stderr, "Montgomery step not exact\n"); std::abort(); }
      if (r < -(1ll << 31) || r >= (1ll << 31)) { std::fprintf(stderr, "Montgomery step overflows 32 bits: t = %d\n", e); std::abort(); }
      e = (int32_t)(r >> 16);
    }
    return t;
  }
  static int32_t chk24(long long a, long long b, long long c) {
    if (a < -(1ll << 23) || a >= (1ll << 23) || b < -(1ll << 23) || b >= (1ll << 23)) { std::fprintf(stderr, "24-bit operand out of range: %lld * %lld\n", a, b); std::abort(); }
    const long long t = a * b + c;
    if (t < -(1ll << 31) || t >= (1ll << 31)) { std::fprintf(stderr, "32-bit overflow: %lld * %lld + %lld\n", a, b, c); std::abort(); }
    if (std::llabs(t) > g_max_prod) g_max_prod = std::llabs(t);
    return (int32_t)t;
  }
  static I mul24(I a, I b) { I r; for (int l = 0; l < 64; ++l) r.v[l] = chk24(a.v[l], b.v[l], 0); return r; }
  static I mul24(int a, I b) { return mul24(I(a), b); }
  static I mad24(I a, I b, I c) { I r; for (int l = 0; l < 64; ++l) r.v[l] = chk24(a.v[l], b.v[l], c.v[l]); return r; }
  static I mad24(I a, int b, I c) { return mad24(a, I(b), c); }
  static U mullo_u(U a, U b) { for (int l = 0; l < 64; ++l) a.v[l] *= b.v[l]; return a; }
  static U mullo_u(U a, uint32_t b) { return mullo_u(a, U(b)); }
  static U mulhi_u(U a, U b) { for (int l = 0; l < 64; ++l) a.v[l] = (uint32_t)(((uint64_t)a.v[l] * b.v[l]) >> 32); return a; }
  static U mulhi_u(U a, uint32_t b) { return mulhi_u(a, U(b)); }
  static U nonzero(U x) { for (auto& e : x.v) e = e != 0; return x; }
  static U csub(U r, uint32_t q) { for (auto& e : r.v) e = e >= q ? e - q : e; return r; }
  static U cadd(U x, uint32_t q) { for (auto& e : x.v) e = e + (q & (uint32_t)((int32_t)e >> 31)); return x; }
  template <class V> static V tab(Tab t, I idx, int off) { V r; for (int l = 0; l < 64; ++l) r.v[l] = (decltype(r.v[0]))t[idx.v[l] + off]; return r; }
  template <class V> static V tab_const(Tab t, int idx) { V r; for (int l = 0; l < 64; ++l) r.v[l] = (decltype(r.v[0]))t[idx]; return r; }
  static I umin(I a, I b) { I r; for (int l = 0; l < 64; ++l) r.v[l] = (uint32_t)a.v[l] < (uint32_t)b.v[l] ? a.v[l] : b.v[l]; return r; }
  template <class V> static void tab_pair(Tab t, int zoff, I idx, int off, V& pk, V& zq) {
    for (int l = 0; l < 64; ++l) { pk.v[l] = (int32_t)t[zoff + 2 * (idx.v[l] + off)]; zq.v[l] = (int32_t)t[zoff + 2 * (idx.v[l] + off) + 1]; }
  }
  template <class V> static void tab_pair_const(Tab t, int zoff, int idx, V& pk, V& zq) { tab_pair<V>(t, zoff, I(0), idx, pk, zq); }
  static I dot2mont(I x, I zq, I pk) {
    for (int l = 0; l < 64; ++l) {
      const int32_t xv = x.v[l];
      if (xv < -32768 || xv > 32767) { std::fprintf(stderr, "dot-product form: operand %d outside 16 bits\n", xv); std::abort(); }
      const int16_t m = (int16_t)(uint16_t)((uint16_t)xv * (uint16_t)zq.v[l]);
      const long long S = (long long)xv * (int16_t)(pk.v[l] & 0xffff) + (long long)m * (int16_t)((uint32_t)pk.v[l] >> 16);
      if (S & 0xffff) { std::fprintf(stderr, "dot-product form: not exact\n"); std::abort(); }
      if (S < -(1ll << 31) || S >= (1ll << 31)) { std::fprintf(stderr, "dot-product form: overflow\n"); std::abort(); }
      x.v[l] = (int32_t)(S >> 16);
    }
    return x;
  }
  template <class V> static V sel_odd(I lane, V a, V b) { V r; for (int l = 0; l < 64; ++l) r.v[l] = (lane.v[l] & 1) ? a.v[l] : b.v[l]; return r; }
  template <int K, int C, int J, class V> static void exchange(V (&x)[C]) {
    for (int r = 0; r < C; ++r)
      if (!((r >> J) & 1)) swap<K>(x[r], x[r | (1 << J)]);
  }
  template <int K, class V> static void swap(V& a, V& b) {
    V na, nb;
    for (int l = 0; l < 64; ++l) {
      const int pl = l ^ (1 << K);
      const bool hi = (l >> K) & 1;
      na.v[l] = hi ? b.v[pl] : a.v[l];
      nb.v[l] = hi ? b.v[l] : a.v[pl];
    }
    a = na; b = nb;
  }
};

static std::vector<uint64_t> schoolbook(const std::vector<uint64_t>& a, const std::vector<int64_t>& b, uint64_t q) {
  const size_t n = a.size();
  std::vector<uint64_t> out(n);
  for (size_t c = 0; c < n; ++c) {
    i128 acc = 0;
    for (size_t i = 0; i < n; ++i) {
      const size_t j = (c + n - i) % n;
      const i128 t = (i128)(a[i] % q) * (i128)(b[j] % (int64_t)q);
      acc += (i <= c) ? t : -t;
    }
    acc %= (i128)q;
    if (acc < 0) acc += q;
    out[c] = (uint64_t)acc;
  }
  return out;
}

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// the largest prime q below the top of the shape's range whose plan has exactly this wave shape
static uint64_t prime_for(int logn, int ld, int qb) {
  const uint64_t hi = qb == 12 ? (1u << 12) : qb == 14 ? (1u << 14) : (1ull << 31), lo = qb == 0 ? (1u << 14) : 5;
  for (uint64_t q = hi - 3; q >= lo; q -= 4) {                       // q = 1 mod 4
    const NttPlan pl = make_ntt_plan(q, 1u << logn);
    if (!pl.ok) continue;
    const NttTables tb = make_ntt_tables(pl);
    if (tb.wave && tb.logn == logn && tb.ld == ld && tb.qb == qb) return q;
  }
  return 0;
}

constexpr int RT = 2;

template <int LOGN, int LD, int QB> static int run_case(bool extreme) {
  using W = HostWave;
  constexpr int N = 1 << LOGN, C = N / 64;
  const uint64_t q = prime_for(LOGN, LD, QB);
  if (!q) { std::printf("no prime for shape %d %d %d\n", LOGN, LD, QB); return 1; }
  const NttPlan pl = make_ntt_plan(q, N);
  const NttTables tb = make_ntt_tables(pl);
  const int inner = extreme ? 4099 : 37;
  const int distinct = extreme ? 1 : inner;                          // extreme: one summand, added `inner` times
  std::vector<std::vector<uint64_t>> a(RT * distinct, std::vector<uint64_t>(N));
  std::vector<std::vector<int64_t>> b(distinct, std::vector<int64_t>(N));
  for (int k = 0; k < distinct; ++k) {
    for (int i = 0; i < N; ++i) {
      for (int t = 0; t < RT; ++t) a[t * distinct + k][i] = extreme ? (t == 0 ? q - 1 : (i & 2 ? q - 1 : 0)) : rnd() % q;
      b[k][i] = extreme ? ((i & 1) ? (int64_t)q - 1 : -((int64_t)q - 1)) : (int64_t)(rnd() % (2 * q - 1)) - (int64_t)(q - 1);
    }
  }
  std::vector<std::vector<uint64_t>> want(RT, std::vector<uint64_t>(N, 0));
  for (int t = 0; t < RT; ++t)
    for (int k = 0; k < distinct; ++k) {
      const std::vector<uint64_t> p = schoolbook(a[t * distinct + k], b[k], q);
      for (int i = 0; i < N; ++i) want[t][i] = (uint64_t)(((u128)want[t][i] + (u128)p[i] * (u128)(inner / distinct)) % q);
    }
  const uint32_t* zf = tb.zetas.data();
  const uint32_t* zi = zf + (1u << pl.L);
  const auto lane = W::lane();
  int bad = 0;
  long long T = 0;
  auto run = [&](auto md, auto core, auto canonical_in, int e) {
    using M = decltype(md);
    using K = decltype(core);
    using V = typename M::V;
    V acc[RT][C];
    for (int t = 0; t < RT; ++t)
      for (int r = 0; r < C; ++r) acc[t][r] = V(0);
    const int r1c = (int)((1u << 16) % q);
    const V r1 = V(r1c > (int)(q / 2) ? r1c - (int)q : r1c);
    int since = 0;
    std::vector<std::array<V, C>> ca(RT * distinct);                      // leaf products, computed once per distinct summand
    for (int k = 0; k < distinct; ++k) {
      V y[C];
      for (int r = 0; r < C; ++r)
        for (int l = 0; l < 64; ++l) y[r].v[l] = canonical_in(b[k][r * 64 + l]);
      K::forward(y, md, zf, lane);
      for (int t = 0; t < RT; ++t) {
        V x[C], c[C];
        for (int r = 0; r < C; ++r)
          for (int l = 0; l < 64; ++l) x[r].v[l] = canonical_in((int64_t)a[t * distinct + k][r * 64 + l]);
        K::forward(x, md, zf, lane);
        K::leafmul(c, x, y, md, zf, lane);
        for (int r = 0; r < C; ++r) ca[t * distinct + k][r] = c[r];
      }
    }
    for (int k = 0; k < inner; ++k) {
      for (int t = 0; t < RT; ++t) {
        V c[C];
        for (int r = 0; r < C; ++r) c[r] = ca[t * distinct + k % distinct][r];
        K::acc_add(acc[t], c, md);
      }
      K::template acc_tick<RT>(acc, md, r1, since);
    }
    T = K::AS::T;
    for (int t = 0; t < RT; ++t) {
      K::acc_close(acc[t], md);
      K::inverse(acc[t], md, zi, lane);
      K::finish(acc[t], md, V(ntt_final_scale(tb, pl, e)));
      for (int r = 0; r < C; ++r)
        for (int l = 0; l < 64; ++l) bad += (uint64_t)(uint32_t)acc[t][r].v[l] != want[t][r * 64 + l];
    }
  };
  if constexpr (QB != 0) {
    using M = std::conditional_t<QB == 12, Mod16D<W>, Mod16<W, QB>>;
    using BD = Bounds16<QB, LOGN, LD>;
    M md; md.q = (int)q; md.nq = -(int)q; md.qinv = tb.qinv16;
    if constexpr (QB == 12) md.zoff = 2 << pl.L;
    const int e = 1 + 2 * BD::r.nrf + BD::r.nri + 1;                     // + the R^-1 of acc_close: fin_fa
    run(md, Core<W, M, BD, LOGN, LD>{}, [&](int64_t v) { return (int32_t)(v % (int64_t)q); }, e);
  } else {
    using M = Mod32<W>;
    M md; md.q = (uint32_t)q; md.nqinv = tb.nqinv32;
    run(md, Core<W, M, NoBounds, LOGN, LD>{}, [&](int64_t v) { const int64_t r = v % (int64_t)q; return (uint32_t)(r < 0 ? r + (int64_t)q : r); }, 1);
  }
  std::printf("shape %d %d %d q=%llu inner=%d T=%lld %s: %s (%d mismatches)\n", LOGN, LD, QB, (unsigned long long)q, inner, T, extreme ? "extreme" : "random",
              bad ? "FAIL" : "ok", bad);
  return bad != 0;
}

int main() {
  int bad = 0;
  for (int ex = 1; ex >= 0; --ex) {
#define PSF_SHAPE(LN, LDV, QBV) bad += run_case<LN, LDV, QBV>(ex);
    // the wave shapes of for_shape (psf_ntt_shapes.hpp)
    PSF_SHAPE(7, 0, 12) PSF_SHAPE(8, 1, 12) PSF_SHAPE(9, 2, 12)
    PSF_SHAPE(7, 0, 14) PSF_SHAPE(7, 1, 14) PSF_SHAPE(8, 0, 14) PSF_SHAPE(8, 1, 14) PSF_SHAPE(8, 2, 14) PSF_SHAPE(9, 0, 14) PSF_SHAPE(9, 1, 14) PSF_SHAPE(9, 2, 14)
    PSF_SHAPE(10, 0, 14) PSF_SHAPE(10, 1, 14) PSF_SHAPE(10, 2, 14)
    PSF_SHAPE(7, 0, 0) PSF_SHAPE(7, 1, 0) PSF_SHAPE(8, 0, 0) PSF_SHAPE(8, 1, 0) PSF_SHAPE(8, 2, 0) PSF_SHAPE(9, 0, 0) PSF_SHAPE(9, 1, 0) PSF_SHAPE(9, 2, 0)
    PSF_SHAPE(10, 0, 0) PSF_SHAPE(10, 1, 0) PSF_SHAPE(10, 2, 0)
#undef PSF_SHAPE
  }
  std::printf("MATPOLY_MODEL %s\n", bad ? "FAIL" : "OK");
  return bad != 0;
}
