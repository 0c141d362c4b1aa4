// The signing part of the FIPS 205 core (tools_amd/csrc/psf_slhdsa_sign_core.hpp over psf_slhdsa_core.hpp) on the CPU: the same text the device
// kernels compile, over the plain C++ back end, composed by the decomposition of psf_slhdsa_sign.hip: the digest; FORS in blocks of 512 leaves reduced
// to height min(a, 9), then the tops; T_k; then ALL d layers' chain ends, leaves and trees from the digest alone; and last the WOTS+ signature values,
// recomputed from the layer messages.  The slot of an authentication path a node goes to is asked of the header's is_auth_node, not restated.  Test
// infrastructure, driven by tests/test_slhdsa_sign_cpu.py, which also builds it with -fsanitize=address,undefined.  One case per line of the file named
// on the command line; <param> is 0 ... 5 as in include/psf_mi355x.h, "-" is the empty string:
//   sign <param> <sk hex> <M hex> <addrnd hex, or - for the deterministic variant>   -> sig hex
// Inputs live in heap blocks of their exact size, so a read past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_slhdsa_sign_core.hpp"

using namespace psf::slh;
using psf::kc::PlainOps;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> v;
  if (h == "-") return v;
  for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return v;
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

constexpr uint32_t kBlock = 512, kBlockHeight = 9;

template <int NW> static void sign(const Params& p, const uint8_t* sk, const uint8_t* msg, size_t msg_len, const uint8_t* addrnd, uint8_t* sig) {
  const uint32_t n = p.n, len = wots_len(n), leaves = 1u << p.hp;
  const uint8_t* pk = sk + 2 * n;
  uint64_t seed[NW], sk_seed[NW];
  load_words<NW>(pk, seed);
  load_words<NW>(sk, sk_seed);
  // the digest
  uint64_t r4[4], r[NW], dw[8];
  prf_msg<PlainOps>(n, sk + n, addrnd ? addrnd : pk, msg, msg_len, r4);
  for (int i = 0; i < NW; ++i) r[i] = r4[i];
  store_words<NW>(sig, r);
  h_msg<PlainOps>(n, sig, pk, msg, msg_len, dw);
  uint8_t digest[64];
  store_words<8>(digest, dw);
  auto dbyte = [&](uint32_t i) { return digest[i]; };
  const Split sp = digest_split(p, dbyte);
  auto fors_at = [&](uint32_t t) { return sig + n + (size_t)t * (p.a + 1) * n; };
  // FORS: blocks of 512 leaves
  const uint32_t top = p.a < kBlockHeight ? p.a : kBlockHeight, total = p.k << p.a, subs = p.a > kBlockHeight ? 1u << (p.a - kBlockHeight) : 1;
  std::vector<uint64_t> sub((size_t)p.k * subs * NW), roots((size_t)p.k * NW), blk((size_t)kBlock * NW);
  for (uint32_t base = 0; base < total; base += kBlock) {
    for (uint32_t j = 0; j < kBlock; ++j) {
      const uint32_t leaf = base + j, t = leaf >> p.a, x = leaf & ((1u << p.a) - 1);
      if (t >= p.k) continue;
      const uint32_t idx = base_2b(dbyte, p.a, t);
      uint64_t v[NW];
      fors_sk<NW, PlainOps>(seed, sk_seed, sp.idx_tree, sp.idx_leaf, leaf, v);
      if (x == idx) store_words<NW>(fors_at(t), v);
      fors_leaf<NW, PlainOps>(seed, sp.idx_tree, sp.idx_leaf, leaf, v, v);
      if (is_auth_node(idx, 0, x)) store_words<NW>(fors_at(t) + n, v);
      for (int i = 0; i < NW; ++i) blk[(size_t)j * NW + i] = v[i];
    }
    for (uint32_t z = 1; z <= top; ++z) {
      for (uint32_t i = 0; i < (kBlock >> z); ++i) {
        const uint32_t node = (base >> z) + i, t = node >> (p.a - z), x = node & ((1u << (p.a - z)) - 1);
        if (t >= p.k) continue;
        uint64_t l[NW], rr[NW], out[NW];
        for (int w = 0; w < NW; ++w) { l[w] = blk[(size_t)(2 * i) * NW + w]; rr[w] = blk[(size_t)(2 * i + 1) * NW + w]; }
        fors_parent<NW, PlainOps>(seed, sp.idx_tree, sp.idx_leaf, z, node, l, rr, out);
        for (int w = 0; w < NW; ++w) blk[(size_t)i * NW + w] = out[w];
        if (z < p.a) {
          if (is_auth_node(base_2b(dbyte, p.a, t), z, x)) store_words<NW>(fors_at(t) + (size_t)(1 + z) * n, out);
          if (z == kBlockHeight)
            for (int w = 0; w < NW; ++w) sub[((size_t)t * subs + x) * NW + w] = out[w];
        } else {
          for (int w = 0; w < NW; ++w) roots[(size_t)t * NW + w] = out[w];
        }
      }
    }
  }
  // the tops
  for (uint32_t t = 0; p.a > kBlockHeight && t < p.k; ++t) {
    uint64_t* s = sub.data() + (size_t)t * subs * NW;
    const uint32_t idx = base_2b(dbyte, p.a, t);
    for (uint32_t z = kBlockHeight + 1; z <= p.a; ++z)
      for (uint32_t i = 0; i < (1u << (p.a - z)); ++i) {
        uint64_t l[NW], rr[NW], out[NW];
        for (int w = 0; w < NW; ++w) { l[w] = s[(size_t)(2 * i) * NW + w]; rr[w] = s[(size_t)(2 * i + 1) * NW + w]; }
        fors_parent<NW, PlainOps>(seed, sp.idx_tree, sp.idx_leaf, z, (t << (p.a - z)) + i, l, rr, out);
        for (int w = 0; w < NW; ++w) s[(size_t)i * NW + w] = out[w];
        if (z < p.a) {
          if (is_auth_node(idx, z, i)) store_words<NW>(fors_at(t) + (size_t)(1 + z) * n, out);
        } else {
          for (int w = 0; w < NW; ++w) roots[(size_t)t * NW + w] = out[w];
        }
      }
  }
  // the messages of the layers: T_k for layer 0, the root of layer j - 1 for layer j
  std::vector<uint64_t> msgs((size_t)p.d * 4);
  {
    uint64_t out[NW];
    fors_pk<NW, PlainOps>(seed, sp.idx_tree, sp.idx_leaf, p.k, [&](size_t w) { return roots[w]; }, out);
    for (int i = 0; i < NW; ++i) msgs[i] = out[i];
  }
  uint8_t* ht = sig + (size_t)(1 + p.k * (1 + p.a)) * n;
  // every layer's tree: none of this reads a message
  std::vector<uint64_t> ends((size_t)len * NW), nodes((size_t)leaves * NW);
  for (uint32_t j = 0; j < p.d; ++j) {
    const uint64_t tree = layer_tree(p, sp, j);
    const uint32_t idx = layer_leaf(p, sp, j);
    uint8_t* auth = ht + (size_t)j * (len + p.hp) * n + (size_t)len * n;
    for (uint32_t leaf = 0; leaf < leaves; ++leaf) {
      for (uint32_t c = 0; c < len; ++c) {
        uint64_t v[NW];
        wots_chain_end<NW, PlainOps>(seed, sk_seed, j, tree, leaf, c, v);
        for (int i = 0; i < NW; ++i) ends[(size_t)c * NW + i] = v[i];
      }
      uint64_t out[NW];
      wots_pk<NW, PlainOps>(seed, j, tree, leaf, [&](size_t w) { return ends[w]; }, out);
      for (int i = 0; i < NW; ++i) nodes[(size_t)leaf * NW + i] = out[i];
      if (is_auth_node(idx, 0, leaf)) store_words<NW>(auth, out);
    }
    for (uint32_t z = 1; z <= p.hp; ++z)
      for (uint32_t t = 0; t < (leaves >> z); ++t) {
        uint64_t l[NW], rr[NW], out[NW];
        for (int i = 0; i < NW; ++i) { l[i] = nodes[(size_t)(2 * t) * NW + i]; rr[i] = nodes[(size_t)(2 * t + 1) * NW + i]; }
        xmss_parent<NW, PlainOps>(seed, j, tree, z, t, l, rr, out);
        for (int i = 0; i < NW; ++i) nodes[(size_t)t * NW + i] = out[i];
        if (z < p.hp) {
          if (is_auth_node(idx, z, t)) store_words<NW>(auth + (size_t)z * n, out);
        } else if (j + 1 < p.d) {
          for (int i = 0; i < NW; ++i) msgs[(size_t)(j + 1) * 4 + i] = out[i];
        }
      }
  }
  // the WOTS+ signature values, recomputed
  for (uint32_t j = 0; j < p.d; ++j) {
    uint8_t m1[32];
    uint64_t mw[NW];
    for (int i = 0; i < NW; ++i) mw[i] = msgs[(size_t)j * 4 + i];
    store_words<NW>(m1, mw);
    for (uint32_t c = 0; c < len; ++c) {
      uint64_t v[NW];
      wots_sig_value<NW, PlainOps>(seed, sk_seed, j, layer_tree(p, sp, j), layer_leaf(p, sp, j), c, wots_digit(n, [&](uint32_t i) { return m1[i]; }, c), v);
      store_words<NW>(ht + (size_t)j * (len + p.hp) * n + (size_t)c * n, v);
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream is(line);
    std::string cmd, a, b, c;
    int param = -1;
    if (!(is >> cmd >> param >> a >> b >> c)) continue;
    if (cmd != "sign" || param < 0 || param >= kSets) return 2;
    const Params p = kParams[param];
    const Exact sk(unhex(a)), msg(unhex(b)), rnd(unhex(c));
    if (sk.n != 4 * p.n || (c != "-" && rnd.n != p.n)) return 2;
    const std::vector<uint8_t> zero(sig_bytes(p));
    const Exact sig(zero);
    const uint8_t* addrnd = c == "-" ? nullptr : rnd.p;
    if (p.n == 16) sign<2>(p, sk.p, msg.p, msg.n, addrnd, sig.p);
    else if (p.n == 24) sign<3>(p, sk.p, msg.p, msg.n, addrnd, sig.p);
    else sign<4>(p, sk.p, msg.p, msg.n, addrnd, sig.p);
    for (size_t i = 0; i < sig.n; ++i) std::printf("%02x", sig.p[i]);
    std::printf("\n");
  }
  return 0;
}
