// The FIPS 205 section 11.2 core of the library (tools_amd/csrc/psf_slhdsa_sha2_core.hpp) on the CPU: the same text the device kernels compile, over the
// plain C++ back end, composed as the kernels of psf_slhdsa_sha2.hip compose it (the midstate made once at the entry of every stage; chain ends staged in
// an array, then T_len; FORS roots staged, then T_k; the layers in turn).  Test infrastructure, driven by tests/test_slhdsa_sha2_cpu.py, which also builds
// it with -fsanitize=address,undefined.  One case per line of the file named on the command line; <param> is 0 ... 5 as in include/psf_mi355x.h
// (PSF_SLHDSA_SHA2_*), "-" is the empty string:
//   keygen <param> <SK.seed hex> <SK.prf hex> <PK.seed hex>   -> pk hex, sk hex
//   verify <param> <pk hex> <M hex> <sig hex>                 -> 0 or 1
//   split <param> <digest hex, m bytes>                       -> idx_tree idx_leaf and the k indices of md, decimal
//   digits <param> <n bytes hex>                              -> the len digits of wots_pkFromSig
//   count <param> <SK.seed> <SK.prf> <PK.seed> <pk> <M> <sig> -> "kg256 kg512 vf256 vf512 ok": the SHA-256 and SHA-512 compressions of that KeyGen and of
//                                                                that Verify, every one counted where it happens (Ops::tick), and the verdict
// Inputs live in heap blocks of their exact size, so a read past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_slhdsa_sha2_core.hpp"

using namespace psf::slh2;

static unsigned long long g_ticks[2];
struct CountOps : psf::sha2::PlainOps {
  static void tick(int family) { ++g_ticks[family]; }
};

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

// the three stages of KeyGen; root: n bytes
template <int NQ> static void keygen(const Params& p, const uint8_t* sk_seed_b, const uint8_t* pk_seed_b, uint8_t* root_b) {
  const uint32_t len = wots_len(p.n), leaves = 1u << p.hp, layer = p.d - 1;
  std::vector<uint32_t> ends((size_t)leaves * len * NQ), nodes((size_t)leaves * NQ);
  {                                                                        // k_kg_chains
    Mid<NQ> mid;
    mid_f<NQ, CountOps>(pk_seed_b, mid);
    uint32_t sk_seed[NQ];
    load_be<NQ>(sk_seed_b, sk_seed);
    for (uint32_t leaf = 0; leaf < leaves; ++leaf)
      for (uint32_t c = 0; c < len; ++c) {
        uint32_t v[NQ];
        wots_chain_end<NQ, CountOps>(mid, sk_seed, layer, 0, leaf, c, v);
        for (int i = 0; i < NQ; ++i) ends[((size_t)leaf * len + c) * NQ + i] = v[i];
      }
  }
  {                                                                        // k_kg_leaf
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk_seed_b, mid);
    for (uint32_t leaf = 0; leaf < leaves; ++leaf) {
      uint32_t out[NQ];
      const uint32_t* e = ends.data() + (size_t)leaf * len * NQ;
      wots_pk<NQ, CountOps>(mid, layer, 0, leaf, [&](size_t w) { return e[w]; }, out);
      for (int i = 0; i < NQ; ++i) nodes[(size_t)leaf * NQ + i] = out[i];
    }
  }
  {                                                                        // k_kg_tree
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk_seed_b, mid);
    uint32_t z = 0;
    for (uint32_t width = leaves / 2; width >= 1; width /= 2) {
      ++z;
      for (uint32_t t = 0; t < width; ++t) {
        uint32_t l[NQ], r[NQ], out[NQ];
        for (int i = 0; i < NQ; ++i) { l[i] = nodes[(size_t)(2 * t) * NQ + i]; r[i] = nodes[(size_t)(2 * t + 1) * NQ + i]; }
        xmss_parent<NQ, CountOps>(mid, layer, 0, z, t, l, r, out);
        for (int i = 0; i < NQ; ++i) nodes[(size_t)t * NQ + i] = out[i];
      }
    }
  }
  uint32_t root[NQ];
  for (int i = 0; i < NQ; ++i) root[i] = nodes[i];
  store_be<NQ>(root_b, root);
}

template <int NQ> static int verify(const Params& p, const uint8_t* pk, const uint8_t* msg, size_t msg_len, const uint8_t* sig) {
  const uint32_t n = p.n, len = wots_len(n);
  uint8_t digest[64];
  if (NQ == 4) h_msg_256<CountOps>(sig, pk, msg, msg_len, digest);        // k_vf_digest
  else h_msg_512<CountOps>(n, sig, pk, msg, msg_len, digest);
  auto dbyte = [&](uint32_t i) { return digest[i]; };
  const Split sp = digest_split(p, dbyte);
  std::vector<uint32_t> roots((size_t)p.k * NQ);
  {                                                                        // k_vf_fors
    Mid<NQ> mid;
    mid_fh<NQ, CountOps>(pk, mid);
    for (uint32_t t = 0; t < p.k; ++t) {
      uint32_t node[NQ];
      fors_root<NQ, CountOps>(mid, sp.idx_tree, sp.idx_leaf, p.a, t, base_2b(dbyte, p.a, t), sig + n + (size_t)t * (p.a + 1) * n, node);
      for (int i = 0; i < NQ; ++i) roots[(size_t)t * NQ + i] = node[i];
    }
  }
  uint32_t node[NQ];
  {                                                                        // k_vf_fors_pk
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk, mid);
    fors_pk<NQ, CountOps>(mid, sp.idx_tree, sp.idx_leaf, p.k, [&](size_t w) { return roots[w]; }, node);
  }
  const uint8_t* ht = sig + (size_t)(1 + p.k * (1 + p.a)) * n;
  std::vector<uint32_t> ends((size_t)len * NQ);
  for (uint32_t j = 0; j < p.d; ++j) {
    const uint8_t* xs = ht + (size_t)j * (len + p.hp) * n;
    const uint64_t tree = layer_tree(p, sp, j);
    const uint32_t leaf = layer_leaf(p, sp, j);
    {                                                                      // k_vf_wots
      Mid<NQ> mid;
      mid_f<NQ, CountOps>(pk, mid);
      for (uint32_t c = 0; c < len; ++c) {
        uint32_t v[NQ];
        load_be<NQ>(xs + (size_t)c * n, v);
        wots_chain_from_sig<NQ, CountOps>(mid, j, tree, leaf, c, wots_digit(n, [&](uint32_t i) { return byte_of(node, i); }, c), v);
        for (int i = 0; i < NQ; ++i) ends[(size_t)c * NQ + i] = v[i];
      }
    }
    {                                                                      // k_vf_xmss
      Mid<NQ> mid;
      mid_h<NQ, CountOps>(pk, mid);
      wots_pk<NQ, CountOps>(mid, j, tree, leaf, [&](size_t w) { return ends[w]; }, node);
      xmss_root<NQ, CountOps>(mid, j, tree, leaf, p.hp, xs + (size_t)len * n, node);
    }
  }
  uint32_t root[NQ], diff = 0;
  load_be<NQ>(pk + n, root);
  for (int i = 0; i < NQ; ++i) diff |= root[i] ^ node[i];
  return diff == 0;
}

static void keygen_n(const Params& p, const uint8_t* sk_seed, const uint8_t* pk_seed, uint8_t* root) {
  if (p.n == 16) keygen<4>(p, sk_seed, pk_seed, root);
  else if (p.n == 24) keygen<6>(p, sk_seed, pk_seed, root);
  else keygen<8>(p, sk_seed, pk_seed, root);
}
static int verify_n(const Params& p, const uint8_t* pk, const uint8_t* msg, size_t msg_len, const uint8_t* sig) {
  return p.n == 16 ? verify<4>(p, pk, msg, msg_len, sig) : p.n == 24 ? verify<6>(p, pk, msg, msg_len, sig) : verify<8>(p, pk, msg, msg_len, sig);
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
    const uint32_t n = p.n;
    if (cmd == "keygen" || cmd == "count") {
      std::string a, b, c;
      is >> a >> b >> c;
      const Exact sk_seed(unhex(a)), sk_prf(unhex(b)), pk_seed(unhex(c));
      if (sk_seed.n != n || sk_prf.n != n || pk_seed.n != n) return 2;
      std::vector<uint8_t> root(n);
      g_ticks[0] = g_ticks[1] = 0;
      keygen_n(p, sk_seed.p, pk_seed.p, root.data());
      if (cmd == "keygen") {
        print_hex(pk_seed.p, n); print_hex(root.data(), n);
        std::printf(" ");
        print_hex(sk_seed.p, n); print_hex(sk_prf.p, n); print_hex(pk_seed.p, n); print_hex(root.data(), n);
        std::printf("\n");
        continue;
      }
      std::printf("%llu %llu ", g_ticks[0], g_ticks[1]);
      std::string d, e, f;
      is >> d >> e >> f;
      const Exact pk(unhex(d)), msg(unhex(e)), sig(unhex(f));
      if (pk.n != 2 * n || sig.n != sig_bytes(p)) return 2;
      g_ticks[0] = g_ticks[1] = 0;
      const int ok = verify_n(p, pk.p, msg.p, msg.n, sig.p);
      std::printf("%llu %llu %d\n", g_ticks[0], g_ticks[1], ok);
    } else if (cmd == "verify") {
      std::string a, b, c;
      is >> a >> b >> c;
      const Exact pk(unhex(a)), msg(unhex(b)), sig(unhex(c));
      if (pk.n != 2 * n || sig.n != sig_bytes(p)) return 2;
      std::printf("%d\n", verify_n(p, pk.p, msg.p, msg.n, sig.p));
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
      if (m1.n != n) return 2;
      for (uint32_t i = 0; i < wots_len(n); ++i) std::printf("%s%u", i ? " " : "", wots_digit(n, [&](uint32_t j) { return m1.p[j]; }, i));
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
