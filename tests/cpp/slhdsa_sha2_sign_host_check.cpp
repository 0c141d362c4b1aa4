// The signing part of the FIPS 205 core for the SHA-2 sets (tools_amd/csrc/psf_slhdsa_sha2_sign_core.hpp over psf_slhdsa_sha2_core.hpp) on the CPU: the same
// text the device kernels compile, over the plain C++ back end, composed by the decomposition of psf_slhdsa_sha2_sign.hip: R by HMAC; the digest; FORS in
// blocks of 512 leaves reduced to height min(a, 9), then the tops; T_k; then ALL d layers' chain ends and leaves from the digest alone; the trees 512 / 2^h'
// to a block of 512 nodes, a lane of the block staying with one tree; and last the WOTS+ signature values, recomputed from the layer messages.  The midstate
// is made once at the entry of every stage.  The slot of an authentication path a node goes to is asked of the header's is_auth_node, not restated.  Test
// infrastructure, driven by tests/test_slhdsa_sha2_sign_cpu.py, which also builds it with -fsanitize=address,undefined.  One case per line of the file
// named on the command line; <param> is 0 ... 5 as in include/psf_mi355x.h (PSF_SLHDSA_SHA2_*), "-" is the empty string:
//   sign <param> <sk hex> <M hex> <addrnd hex, or - for the deterministic variant>   -> sig hex, then "c256 c512 digits": the SHA-256 and SHA-512
//                                                                                       compressions of that signature, every one counted where it happens
//                                                                                       (Ops::tick), and the sum of the d len signed WOTS+ digits
//   prf <param> <SK.prf hex> <opt_rand hex> <M hex>                                  -> R hex, then "c256 c512" of that PRF_msg
// Inputs live in heap blocks of their exact size, so a read past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../tools_amd/csrc/psf_slhdsa_sha2_sign_core.hpp"

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
// a heap copy of exactly the bytes given; p is NULL for the empty string, as a caller without a message has it
struct Exact {
  uint8_t* p;
  size_t n;
  explicit Exact(const std::vector<uint8_t>& v) : p(v.empty() ? nullptr : static_cast<uint8_t*>(std::malloc(v.size()))), n(v.size()) {
    if (!v.empty()) std::memcpy(p, v.data(), v.size());
  }
  ~Exact() { std::free(p); }
};

constexpr uint32_t kBlock = 512, kBlockHeight = 9;

template <int NQ> static unsigned long long sign(const Params& p, const uint8_t* sk, const uint8_t* msg, size_t msg_len, const uint8_t* addrnd, uint8_t* sig) {
  const uint32_t n = p.n, len = wots_len(n), leaves = 1u << p.hp;
  const uint8_t* pk = sk + 2 * n;
  uint32_t sk_seed[NQ];
  load_be<NQ>(sk, sk_seed);
  {                                                                        // k_sg_prf_msg
    uint32_t r[NQ];
    prf_msg<NQ, CountOps>(sk + n, addrnd ? addrnd : pk, msg, msg_len, r);
    store_be<NQ>(sig, r);
  }
  uint8_t digest[64];
  if (NQ == 4) h_msg_256<CountOps>(sig, pk, msg, msg_len, digest);        // k_sg_digest
  else h_msg_512<CountOps>(n, sig, pk, msg, msg_len, digest);
  auto dbyte = [&](uint32_t i) { return digest[i]; };
  const Split sp = digest_split(p, dbyte);
  auto fors_at = [&](uint32_t t) { return sig + n + (size_t)t * (p.a + 1) * n; };
  // FORS: blocks of 512 leaves
  const uint32_t top = p.a < kBlockHeight ? p.a : kBlockHeight, total = p.k << p.a, subs = p.a > kBlockHeight ? 1u << (p.a - kBlockHeight) : 1;
  std::vector<uint32_t> sub((size_t)p.k * subs * NQ), roots((size_t)p.k * NQ), blk((size_t)kBlock * NQ);
  {                                                                        // k_sg_fors
    Mid<NQ> mid;
    mid_fh<NQ, CountOps>(pk, mid);
    for (uint32_t base = 0; base < total; base += kBlock) {
      for (uint32_t j = 0; j < kBlock; ++j) {
        const uint32_t leaf = base + j, t = leaf >> p.a, x = leaf & ((1u << p.a) - 1);
        if (t >= p.k) continue;
        const uint32_t idx = base_2b(dbyte, p.a, t);
        uint32_t v[NQ];
        fors_sk<NQ, CountOps>(mid, sk_seed, sp.idx_tree, sp.idx_leaf, leaf, v);
        if (x == idx) store_be<NQ>(fors_at(t), v);
        fors_leaf<NQ, CountOps>(mid, sp.idx_tree, sp.idx_leaf, leaf, v, v);
        if (is_auth_node(idx, 0, x)) store_be<NQ>(fors_at(t) + n, v);
        for (int i = 0; i < NQ; ++i) blk[(size_t)j * NQ + i] = v[i];
      }
      for (uint32_t z = 1; z <= top; ++z) {
        for (uint32_t i = 0; i < (kBlock >> z); ++i) {
          const uint32_t node = (base >> z) + i, t = node >> (p.a - z), x = node & ((1u << (p.a - z)) - 1);
          if (t >= p.k) continue;
          uint32_t l[NQ], rr[NQ], out[NQ];
          for (int w = 0; w < NQ; ++w) { l[w] = blk[(size_t)(2 * i) * NQ + w]; rr[w] = blk[(size_t)(2 * i + 1) * NQ + w]; }
          fors_parent<NQ, CountOps>(mid, sp.idx_tree, sp.idx_leaf, z, node, l, rr, out);
          for (int w = 0; w < NQ; ++w) blk[(size_t)i * NQ + w] = out[w];
          if (z < p.a) {
            if (is_auth_node(base_2b(dbyte, p.a, t), z, x)) store_be<NQ>(fors_at(t) + (size_t)(1 + z) * n, out);
            if (z == kBlockHeight)
              for (int w = 0; w < NQ; ++w) sub[((size_t)t * subs + x) * NQ + w] = out[w];
          } else {
            for (int w = 0; w < NQ; ++w) roots[(size_t)t * NQ + w] = out[w];
          }
        }
      }
    }
  }
  if (p.a > kBlockHeight) {                                                // k_sg_fors_top
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk, mid);
    for (uint32_t t = 0; t < p.k; ++t) {
      uint32_t* s = sub.data() + (size_t)t * subs * NQ;
      const uint32_t idx = base_2b(dbyte, p.a, t);
      for (uint32_t z = kBlockHeight + 1; z <= p.a; ++z)
        for (uint32_t i = 0; i < (1u << (p.a - z)); ++i) {
          uint32_t l[NQ], rr[NQ], out[NQ];
          for (int w = 0; w < NQ; ++w) { l[w] = s[(size_t)(2 * i) * NQ + w]; rr[w] = s[(size_t)(2 * i + 1) * NQ + w]; }
          fors_parent<NQ, CountOps>(mid, sp.idx_tree, sp.idx_leaf, z, (t << (p.a - z)) + i, l, rr, out);
          for (int w = 0; w < NQ; ++w) s[(size_t)i * NQ + w] = out[w];
          if (z < p.a) {
            if (is_auth_node(idx, z, i)) store_be<NQ>(fors_at(t) + (size_t)(1 + z) * n, out);
          } else {
            for (int w = 0; w < NQ; ++w) roots[(size_t)t * NQ + w] = out[w];
          }
        }
    }
  }
  // the messages of the layers, 8 words each: T_k for layer 0, the root of layer j - 1 for layer j
  std::vector<uint32_t> msgs((size_t)p.d * 8);
  {                                                                        // k_sg_fors_pk
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk, mid);
    uint32_t out[NQ];
    fors_pk<NQ, CountOps>(mid, sp.idx_tree, sp.idx_leaf, p.k, [&](size_t w) { return roots[w]; }, out);
    for (int i = 0; i < NQ; ++i) msgs[i] = out[i];
  }
  uint8_t* ht = sig + (size_t)(1 + p.k * (1 + p.a)) * n;
  // every layer's chain ends and leaves: none of this reads a message
  std::vector<uint32_t> ends((size_t)p.d * leaves * len * NQ), nodes(((size_t)p.d * leaves + kBlock) * NQ);
  {                                                                        // k_sg_chains
    Mid<NQ> mid;
    mid_f<NQ, CountOps>(pk, mid);
    for (size_t g = 0; g < (size_t)p.d * leaves * len; ++g) {
      const uint32_t layer = (uint32_t)(g / ((size_t)leaves * len)), r2 = (uint32_t)(g % ((size_t)leaves * len)), leaf = r2 / len, c = r2 % len;
      uint32_t v[NQ];
      wots_chain_end<NQ, CountOps>(mid, sk_seed, layer, layer_tree(p, sp, layer), leaf, c, v);
      for (int i = 0; i < NQ; ++i) ends[g * NQ + i] = v[i];
    }
  }
  {                                                                        // k_sg_leaf
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk, mid);
    for (size_t g = 0; g < (size_t)p.d * leaves; ++g) {
      const uint32_t layer = (uint32_t)(g / leaves), leaf = (uint32_t)(g % leaves);
      const uint32_t* e = ends.data() + g * len * NQ;
      uint32_t out[NQ];
      wots_pk<NQ, CountOps>(mid, layer, layer_tree(p, sp, layer), leaf, [&](size_t w) { return e[w]; }, out);
      for (int i = 0; i < NQ; ++i) nodes[g * NQ + i] = out[i];
    }
  }
  {                                                                        // k_sg_tree: 512 / 2^h' trees to a block, lane `tid` stays with tree tid >> (h' - 1)
    Mid<NQ> mid;
    mid_h<NQ, CountOps>(pk, mid);
    const uint32_t per = kBlock >> p.hp, half = leaves / 2;
    for (uint32_t wg = 0; wg * per < p.d; ++wg) {
      uint32_t* lds = nodes.data() + (size_t)wg * kBlock * NQ;             // reduced in place: each tree inside its own 2^h' nodes
      for (uint32_t z = 0; z <= p.hp; ++z) {
        std::vector<uint32_t> outs((size_t)256 * NQ);
        std::vector<char> act(256, 0);
        for (uint32_t tid = 0; tid < 256; ++tid) {
          const uint32_t lt = tid / half, i = tid % half, j = wg * per + lt;
          if (j >= p.d) continue;
          const uint64_t tree = layer_tree(p, sp, j);
          const uint32_t idx = layer_leaf(p, sp, j);
          uint8_t* auth = ht + (size_t)j * (len + p.hp) * n + (size_t)len * n;
          uint32_t* mine = lds + ((size_t)lt << p.hp) * NQ;
          if (z == 0) {
            for (uint32_t e = 0; e < 2; ++e)
              if (is_auth_node(idx, 0, 2 * i + e)) {
                uint32_t v[NQ];
                for (int w = 0; w < NQ; ++w) v[w] = mine[(size_t)(2 * i + e) * NQ + w];
                store_be<NQ>(auth, v);
              }
            continue;
          }
          if (i >= (leaves >> z)) continue;
          uint32_t l[NQ], rr[NQ], out[NQ];
          for (int w = 0; w < NQ; ++w) { l[w] = mine[(size_t)(2 * i) * NQ + w]; rr[w] = mine[(size_t)(2 * i + 1) * NQ + w]; }
          xmss_parent<NQ, CountOps>(mid, j, tree, z, i, l, rr, out);
          act[tid] = 1;
          for (int w = 0; w < NQ; ++w) outs[(size_t)tid * NQ + w] = out[w];
          if (z < p.hp) {
            if (is_auth_node(idx, z, i)) store_be<NQ>(auth + (size_t)z * n, out);
          } else if (j + 1 < p.d) {
            for (int w = 0; w < NQ; ++w) msgs[(size_t)(j + 1) * 8 + w] = out[w];
          }
        }
        for (uint32_t tid = 0; tid < 256; ++tid)                          // after the barrier
          if (act[tid])
            for (int w = 0; w < NQ; ++w) lds[(((size_t)(tid / half) << p.hp) + tid % half) * NQ + w] = outs[(size_t)tid * NQ + w];
      }
    }
  }
  unsigned long long digits = 0;
  {                                                                        // k_sg_wots: the signature values, recomputed
    Mid<NQ> mid;
    mid_f<NQ, CountOps>(pk, mid);
    for (uint32_t j = 0; j < p.d; ++j) {
      const uint32_t* m1 = msgs.data() + (size_t)j * 8;
      for (uint32_t c = 0; c < len; ++c) {
        uint32_t v[NQ];
        const uint32_t digit = wots_digit(n, [&](uint32_t i) { return byte_of(m1, i); }, c);
        digits += digit;
        wots_sig_value<NQ, CountOps>(mid, sk_seed, j, layer_tree(p, sp, j), layer_leaf(p, sp, j), c, digit, v);
        store_be<NQ>(ht + (size_t)j * (len + p.hp) * n + (size_t)c * n, v);
      }
    }
  }
  return digits;
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
    if (param < 0 || param >= kSets) return 2;
    const Params p = kParams[param];
    g_ticks[0] = g_ticks[1] = 0;
    if (cmd == "sign") {
      const Exact sk(unhex(a)), msg(unhex(b)), rnd(unhex(c));
      if (sk.n != 4 * p.n || (c != "-" && rnd.n != p.n)) return 2;
      const std::vector<uint8_t> zero(sig_bytes(p));
      const Exact sig(zero);
      const uint8_t* addrnd = c == "-" ? nullptr : rnd.p;
      unsigned long long digits;
      if (p.n == 16) digits = sign<4>(p, sk.p, msg.p, msg.n, addrnd, sig.p);
      else if (p.n == 24) digits = sign<6>(p, sk.p, msg.p, msg.n, addrnd, sig.p);
      else digits = sign<8>(p, sk.p, msg.p, msg.n, addrnd, sig.p);
      print_hex(sig.p, sig.n);
      std::printf(" %llu %llu %llu\n", g_ticks[0], g_ticks[1], digits);
    } else if (cmd == "prf") {
      const Exact key(unhex(a)), rnd(unhex(b)), msg(unhex(c));
      if (key.n != p.n || rnd.n != p.n) return 2;
      uint8_t out[32];
      if (p.n == 16) { uint32_t r[4]; prf_msg<4, CountOps>(key.p, rnd.p, msg.p, msg.n, r); store_be<4>(out, r); }
      else if (p.n == 24) { uint32_t r[6]; prf_msg<6, CountOps>(key.p, rnd.p, msg.p, msg.n, r); store_be<6>(out, r); }
      else { uint32_t r[8]; prf_msg<8, CountOps>(key.p, rnd.p, msg.p, msg.n, r); store_be<8>(out, r); }
      print_hex(out, p.n);
      std::printf(" %llu %llu\n", g_ticks[0], g_ticks[1]);
    } else {
      return 2;
    }
  }
  return 0;
}
