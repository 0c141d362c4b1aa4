// The FIPS 205 core of the library (tools_amd/csrc/psf_slhdsa_core.hpp) on the CPU: the same text the device kernels compile, over the plain C++
// back end, composed as the kernels of psf_slhdsa.hip compose it (chain ends staged in an array, then T_len; FORS roots staged, then T_k; the layers in
// turn).  Test infrastructure, driven by tests/test_slhdsa_cpu.py, which also builds it with -fsanitize=address,undefined.  One case per line of the
// file named on the command line; <param> is 0 ... 5 as in include/psf_mi355x.h, "-" is the empty string:
//   keygen <param> <SK.seed hex> <SK.prf hex> <PK.seed hex>   -> pk hex, sk hex
//   verify <param> <pk hex> <M hex> <sig hex>                 -> 0 or 1
//   split <param> <digest hex, m bytes>                       -> idx_tree idx_leaf and the k indices of md, decimal
//   digits <param> <n bytes hex>                              -> the len digits of wots_pkFromSig
// Inputs live in heap blocks of their exact size, so a read past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_slhdsa_core.hpp"

using namespace psf::slh;
using psf::kc::PlainOps;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> v;
  if (h == "-") return v;
  for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static void print_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}
// a heap copy of exactly the bytes given
struct Exact {
  uint8_t* p;
  size_t n;
  explicit Exact(const std::vector<uint8_t>& v) : p(static_cast<uint8_t*>(std::malloc(v.size() + (v.empty() ? 1 : 0)))), n(v.size()) {
    if (!v.empty()) std::memcpy(p, v.data(), v.size());
  }
  ~Exact() { std::free(p); }
};

template <int NW> static void keygen(const Params& p, const uint8_t* sk_seed_b, const uint8_t* sk_prf, const uint8_t* pk_seed_b) {
  const uint32_t n = p.n, len = wots_len(n), leaves = 1u << p.hp, layer = p.d - 1;
  uint64_t seed[NW], sk_seed[NW];
  load_words<NW>(pk_seed_b, seed);
  load_words<NW>(sk_seed_b, sk_seed);
  std::vector<uint64_t> ends((size_t)len * NW), nodes((size_t)leaves * NW);
  for (uint32_t leaf = 0; leaf < leaves; ++leaf) {
    for (uint32_t c = 0; c < len; ++c) {
      uint64_t v[NW];
      wots_chain_end<NW, PlainOps>(seed, sk_seed, layer, 0, leaf, c, v);
      for (int i = 0; i < NW; ++i) ends[(size_t)c * NW + i] = v[i];
    }
    uint64_t out[NW];
    wots_pk<NW, PlainOps>(seed, layer, 0, leaf, [&](size_t w) { return ends[w]; }, out);
    for (int i = 0; i < NW; ++i) nodes[(size_t)leaf * NW + i] = out[i];
  }
  uint32_t z = 0;
  for (uint32_t width = leaves / 2; width >= 1; width /= 2) {
    ++z;
    for (uint32_t t = 0; t < width; ++t) {
      uint64_t l[NW], r[NW], out[NW];
      for (int i = 0; i < NW; ++i) { l[i] = nodes[(size_t)(2 * t) * NW + i]; r[i] = nodes[(size_t)(2 * t + 1) * NW + i]; }
      xmss_parent<NW, PlainOps>(seed, layer, 0, z, t, l, r, out);
      for (int i = 0; i < NW; ++i) nodes[(size_t)t * NW + i] = out[i];
    }
  }
  uint64_t root[NW];
  for (int i = 0; i < NW; ++i) root[i] = nodes[i];
  std::vector<uint8_t> rb(n);
  store_words<NW>(rb.data(), root);
  print_hex(pk_seed_b, n); print_hex(rb.data(), n);
  std::printf(" ");
  print_hex(sk_seed_b, n); print_hex(sk_prf, n); print_hex(pk_seed_b, n); print_hex(rb.data(), n);
  std::printf("\n");
}

template <int NW> static int verify(const Params& p, const uint8_t* pk, const uint8_t* msg, size_t msg_len, const uint8_t* sig) {
  const uint32_t n = p.n, len = wots_len(n);
  uint64_t dw[8];
  h_msg<PlainOps>(n, sig, pk, msg, msg_len, dw);
  uint8_t digest[64];
  store_words<8>(digest, dw);
  auto dbyte = [&](uint32_t i) { return digest[i]; };
  const Split sp = digest_split(p, dbyte);
  uint64_t seed[NW];
  load_words<NW>(pk, seed);
  std::vector<uint64_t> roots((size_t)p.k * NW);
  for (uint32_t t = 0; t < p.k; ++t) {
    uint64_t node[NW];
    fors_root<NW, PlainOps>(seed, sp.idx_tree, sp.idx_leaf, p.a, t, base_2b(dbyte, p.a, t), sig + n + (size_t)t * (p.a + 1) * n, node);
    for (int i = 0; i < NW; ++i) roots[(size_t)t * NW + i] = node[i];
  }
  uint64_t node[NW];
  fors_pk<NW, PlainOps>(seed, sp.idx_tree, sp.idx_leaf, p.k, [&](size_t w) { return roots[w]; }, node);
  const uint8_t* ht = sig + (size_t)(1 + p.k * (1 + p.a)) * n;
  std::vector<uint64_t> ends((size_t)len * NW);
  for (uint32_t j = 0; j < p.d; ++j) {
    const uint8_t* xs = ht + (size_t)j * (len + p.hp) * n;
    const uint64_t tree = layer_tree(p, sp, j);
    const uint32_t leaf = layer_leaf(p, sp, j);
    uint8_t m1[32];
    store_words<NW>(m1, node);
    for (uint32_t c = 0; c < len; ++c) {
      uint64_t v[NW];
      load_words<NW>(xs + (size_t)c * n, v);
      wots_chain_from_sig<NW, PlainOps>(seed, j, tree, leaf, c, wots_digit(n, [&](uint32_t i) { return m1[i]; }, c), v);
      for (int i = 0; i < NW; ++i) ends[(size_t)c * NW + i] = v[i];
    }
    wots_pk<NW, PlainOps>(seed, j, tree, leaf, [&](size_t w) { return ends[w]; }, node);
    xmss_root<NW, PlainOps>(seed, j, tree, leaf, p.hp, xs + (size_t)len * n, node);
  }
  uint64_t root[NW];
  load_words<NW>(pk + n, root);
  uint64_t diff = 0;
  for (int i = 0; i < NW; ++i) diff |= root[i] ^ node[i];
  return diff == 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream is(line);
    std::string cmd;
    int param = -1;
    if (!(is >> cmd >> param)) continue;
    if (param < 0 || param >= kSets) return 2;
    const Params p = kParams[param];
    if (cmd == "keygen") {
      std::string a, b, c;
      is >> a >> b >> c;
      const Exact sk_seed(unhex(a)), sk_prf(unhex(b)), pk_seed(unhex(c));
      if (sk_seed.n != p.n || sk_prf.n != p.n || pk_seed.n != p.n) return 2;
      if (p.n == 16) keygen<2>(p, sk_seed.p, sk_prf.p, pk_seed.p);
      else if (p.n == 24) keygen<3>(p, sk_seed.p, sk_prf.p, pk_seed.p);
      else keygen<4>(p, sk_seed.p, sk_prf.p, pk_seed.p);
    } else if (cmd == "verify") {
      std::string a, b, c;
      is >> a >> b >> c;
      const Exact pk(unhex(a)), msg(unhex(b)), sig(unhex(c));
      if (pk.n != 2 * p.n || sig.n != sig_bytes(p)) return 2;
      const int ok = p.n == 16 ? verify<2>(p, pk.p, msg.p, msg.n, sig.p) : p.n == 24 ? verify<3>(p, pk.p, msg.p, msg.n, sig.p) : verify<4>(p, pk.p, msg.p, msg.n, sig.p);
      std::printf("%d\n", ok);
    } else if (cmd == "split") {
      std::string a;
      is >> a;
      const Exact d(unhex(a));
      if (d.n != p.m) return 2;
      auto dbyte = [&](uint32_t i) { return d.p[i]; };
      const Split sp = digest_split(p, dbyte);
      std::printf("%llu %u", (unsigned long long)sp.idx_tree, sp.idx_leaf);
      for (uint32_t t = 0; t < p.k; ++t) std::printf(" %u", base_2b(dbyte, p.a, t));
      std::printf("\n");
    } else if (cmd == "digits") {
      std::string a;
      is >> a;
      const Exact m1(unhex(a));
      if (m1.n != p.n) return 2;
      for (uint32_t i = 0; i < wots_len(p.n); ++i) std::printf("%s%u", i ? " " : "", wots_digit(p.n, [&](uint32_t j) { return m1.p[j]; }, i));
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
