// psf_slhdsa_sha2_sign.hip -- SLH-DSA signing on the device for the six SHA-2 parameter sets, batched: slh_sign_internal (FIPS 205 Algorithm 19), bytes in
// and bytes out, `count` instances per call.  FIPS 205's text is psf_slhdsa_sha2_core.hpp and psf_slhdsa_sha2_sign_core.hpp; this unit adds the kernels and
// the glue.  The stage split is psf_slhdsa_sign.hip's: every layer's (tree address, leaf index) follows from the digest, so the d XMSS trees of a signature
// are built side by side in the same launches; only the WOTS+ MESSAGE of layer j waits for layer j - 1 (its root; the FORS public key for j = 0).
// NQ = n / 4 = 4, 6, 8: a node is NQ big-endian 32-bit words, in registers, LDS and the workspace alike.
//   k_sg_prf_msg<NQ>   one lane per instance: R = PRF_msg(SK.prf, opt_rand, M) by HMAC -> sig[0, n)
//   k_sg_digest<NQ>    one lane per instance: 64 bytes of H_msg(R, PK.seed, PK.root, M) -> the workspace (at n > 16 the public inner digest passes through
//                      those same 64 bytes, as in Verify)
//   k_sg_fors<NQ>      one workgroup per 512 FORS leaves (one subtree of height 9 when a >= 9, else 2^(9 - a) whole trees): PRF and F per leaf in
//                      registers, the leaves in LDS, min(a, 9) levels of H; the revealed secret value and path slots 0 ... min(a, 9) - 1 -> the
//                      signature; the tree root (a <= 9) or subtree root (a > 9) -> the workspace
//   k_sg_fors_top<NQ>  a > 9 only: one lane per (instance, tree): the 2^(a - 9) subtree roots reduced in place; path slots 10 ... a - 1; the tree root
//   k_sg_fors_pk<NQ>   one lane per instance: T_k over the k roots -> the message of layer 0
//   k_sg_chains<NQ>    one lane per (instance, layer, leaf, chain): PRF and the 15 steps of F; the chain END (public) -> the workspace
//   k_sg_leaf<NQ>      one lane per (instance, layer, leaf): T_len over the len chain ends -> the leaf
//   k_sg_tree<NQ>      one workgroup per 512 / 2^h' whole trees of the (instance d + layer) index space: their 512 leaves in LDS, h' levels of H, lane `tid`
//                      staying with tree tid >> (h' - 1) of the workgroup; the h' path nodes -> the signature; the root -> the message of layer j + 1
//   k_sg_wots<NQ>      one lane per (instance, layer, chain): PRF and `digit` steps of F, recomputed -> the signature
// Every lane makes the midstate(s) its stage needs from PK.seed at kernel entry, once.  No secret leaves registers: the stores of every kernel write a value
// that the signature reveals or that a verifier recomputes from it (DESIGN.md "SLH-DSA: signing for the SHA-2 sets" goes through them one by one).  Every
// index, digit, branch and loop bound comes from the lane index, the digest or a root.  Lane and byte indices are size_t; every stage goes through
// launch_chunked.
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_slhdsa_sha2_api.hpp"
#include "psf_slhdsa_sha2_sign_core.hpp"

namespace psf {
namespace slh2 {

using Dev = sha2::DevOps;

// `first`: the launches of one stage are chunks of at most 2^31 - 1 workgroups; lane g of the stage is first + its index in the launch, and workgroup
// first / 256 + blockIdx.x where a workgroup is the unit
struct SgArgs {
  size_t first, count, sk_stride, msg_len, msg_stride, sig_len, rnd_stride;
  Params p;
  uint32_t len, leaves, fors_wgs;
  const uint8_t* sk; const uint8_t* msg; const uint8_t* opt_rand;             // opt_rand of instance c at opt_rand + c rnd_stride: addrnd, or PK.seed in the key
  uint8_t* sig;
  uint8_t* digest; uint32_t* fors_sub; uint32_t* fors_roots; uint32_t* msgs; uint32_t* ends; uint32_t* nodes;
};
constexpr int kSgDigestBytes = 64, kSgMsgWords = 8;                        // per instance: 64 bytes of H_msg; per (instance, layer): 32 bytes of message
constexpr uint32_t kSgLeaves = 512, kSgForsHeight = 9;                     // the leaves of one workgroup, FORS and XMSS (h' <= 9)

__device__ __forceinline__ const uint8_t* digest_of(const SgArgs& a, size_t inst) { return a.digest + inst * kSgDigestBytes; }
__device__ __forceinline__ size_t fors_off(const SgArgs& a, uint32_t t) { return (size_t)a.p.n + (size_t)t * (a.p.a + 1) * a.p.n; }
__device__ __forceinline__ size_t xmss_off(const SgArgs& a, uint32_t layer) {
  return (size_t)(1 + a.p.k * (1 + a.p.a)) * a.p.n + (size_t)layer * (a.len + a.p.hp) * a.p.n;
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_prf_msg(SgArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint32_t r[NQ];
  prf_msg<NQ, Dev>(a.sk + c * a.sk_stride + a.p.n, a.opt_rand + c * a.rnd_stride, a.msg + c * a.msg_stride, a.msg_len, r);
  store_be<NQ>(a.sig + c * a.sig_len, r);
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_digest(SgArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint8_t* out = a.digest + c * kSgDigestBytes;
  const uint8_t* pk = a.sk + c * a.sk_stride + 2 * a.p.n;                  // PK.seed || PK.root, contiguous in the key
  if constexpr (NQ == 4) h_msg_256<Dev>(a.sig + c * a.sig_len, pk, a.msg + c * a.msg_stride, a.msg_len, out);
  else h_msg_512<Dev>(a.p.n, a.sig + c * a.sig_len, pk, a.msg + c * a.msg_stride, a.msg_len, out);
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_fors(SgArgs a) {
  __shared__ uint32_t lds[kSgLeaves * NQ];
  const uint32_t tid = threadIdx.x;
  const size_t wg = a.first / 256 + blockIdx.x;
  if (wg >= a.count * a.fors_wgs) return;                                  // the whole workgroup
  const size_t inst = wg / a.fors_wgs;
  const uint32_t base = (uint32_t)(wg - inst * a.fors_wgs) * kSgLeaves;    // the first of this workgroup's leaves in the index space of the k trees
  const uint8_t* d = digest_of(a, inst);
  auto dbyte = [&](uint32_t i) { return d[i]; };
  const Split sp = digest_split(a.p, dbyte);
  const uint8_t* sk = a.sk + inst * a.sk_stride;
  uint8_t* sig = a.sig + inst * a.sig_len;
  Mid<NQ> mid;
  mid_fh<NQ, Dev>(sk + 2 * a.p.n, mid);
  uint32_t sk_seed[NQ];
  load_be<NQ>(sk, sk_seed);
  const uint32_t top = a.p.a < kSgForsHeight ? a.p.a : kSgForsHeight;
#pragma clang loop unroll(disable)
  for (uint32_t j = tid; j < kSgLeaves; j += 256) {
    const uint32_t leaf = base + j, t = leaf >> a.p.a, x = leaf & ((1u << a.p.a) - 1);
    if (t < a.p.k) {                                                       // the last workgroup of an f set is partly empty
      const uint32_t idx = base_2b(dbyte, a.p.a, t);
      uint8_t* ts = sig + fors_off(a, t);
      uint32_t v[NQ];
      fors_sk<NQ, Dev>(mid, sk_seed, sp.idx_tree, sp.idx_leaf, leaf, v);
      if (x == idx) store_be<NQ>(ts, v);                                   // the one secret value the signature reveals
      fors_leaf<NQ, Dev>(mid, sp.idx_tree, sp.idx_leaf, leaf, v, v);
      if (is_auth_node(idx, 0, x)) store_be<NQ>(ts + a.p.n, v);
#pragma unroll
      for (int i = 0; i < NQ; ++i) lds[j * NQ + i] = v[i];
    }
  }
  __syncthreads();
  for (uint32_t z = 1; z <= top; ++z) {
    const uint32_t node = (base >> z) + tid, t = node >> (a.p.a - z);      // node `tid` of this workgroup at height z, in the index space of the k trees
    const bool act = tid < (kSgLeaves >> z) && t < a.p.k;
    uint32_t out[NQ];
    if (act) {
      uint32_t l[NQ], r[NQ];
#pragma unroll
      for (int i = 0; i < NQ; ++i) { l[i] = lds[2 * tid * NQ + i]; r[i] = lds[(2 * tid + 1) * NQ + i]; }
      fors_parent<NQ, Dev>(mid, sp.idx_tree, sp.idx_leaf, z, node, l, r, out);
    }
    __syncthreads();
    if (act) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) lds[tid * NQ + i] = out[i];
      const uint32_t x = node & ((1u << (a.p.a - z)) - 1);
      if (z < a.p.a) {
        if (is_auth_node(base_2b(dbyte, a.p.a, t), z, x)) store_be<NQ>(sig + fors_off(a, t) + (size_t)(1 + z) * a.p.n, out);
        if (z == kSgForsHeight) {                                          // a > 9: the root of subtree x of tree t
#pragma unroll
          for (int i = 0; i < NQ; ++i) a.fors_sub[(((inst * a.p.k + t) << (a.p.a - kSgForsHeight)) + x) * NQ + i] = out[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < NQ; ++i) a.fors_roots[(inst * a.p.k + t) * NQ + i] = out[i];
      }
    }
    __syncthreads();
  }
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_fors_top(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.p.k) return;
  const size_t inst = g / a.p.k;
  const uint32_t t = (uint32_t)(g - inst * a.p.k);
  const uint8_t* d = digest_of(a, inst);
  auto dbyte = [&](uint32_t i) { return d[i]; };
  const Split sp = digest_split(a.p, dbyte);
  const uint32_t idx = base_2b(dbyte, a.p.a, t);
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.sk + inst * a.sk_stride + 2 * a.p.n, mid);
  uint8_t* ts = a.sig + inst * a.sig_len + fors_off(a, t);
  uint32_t* sub = a.fors_sub + (g << (a.p.a - kSgForsHeight)) * NQ;        // this tree's subtree roots, reduced in place: node i overwrites a child of node <= i
#pragma clang loop unroll(disable)
  for (uint32_t z = kSgForsHeight + 1; z <= a.p.a; ++z) {
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < (1u << (a.p.a - z)); ++i) {
      uint32_t l[NQ], r[NQ], out[NQ];
#pragma unroll
      for (int w = 0; w < NQ; ++w) { l[w] = sub[2 * i * NQ + w]; r[w] = sub[(2 * i + 1) * NQ + w]; }
      fors_parent<NQ, Dev>(mid, sp.idx_tree, sp.idx_leaf, z, (t << (a.p.a - z)) + i, l, r, out);
#pragma unroll
      for (int w = 0; w < NQ; ++w) sub[i * NQ + w] = out[w];
      if (z < a.p.a) {
        if (is_auth_node(idx, z, i)) store_be<NQ>(ts + (size_t)(1 + z) * a.p.n, out);
      } else {
#pragma unroll
        for (int w = 0; w < NQ; ++w) a.fors_roots[g * NQ + w] = out[w];
      }
    }
  }
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_fors_pk(SgArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* d = digest_of(a, c);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.sk + c * a.sk_stride + 2 * a.p.n, mid);
  uint32_t out[NQ];
  const uint32_t* roots = a.fors_roots + c * a.p.k * NQ;
  fors_pk<NQ, Dev>(mid, sp.idx_tree, sp.idx_leaf, a.p.k, [&](size_t w) { return roots[w]; }, out);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.msgs[c * a.p.d * kSgMsgWords + i] = out[i];
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_chains(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per_layer = (size_t)a.leaves * a.len, per = a.p.d * per_layer;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), layer = r / (uint32_t)per_layer, r2 = r - layer * (uint32_t)per_layer, leaf = r2 / a.len, c = r2 - leaf * a.len;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint8_t* sk = a.sk + inst * a.sk_stride;
  Mid<NQ> mid;
  mid_f<NQ, Dev>(sk + 2 * a.p.n, mid);
  uint32_t sk_seed[NQ], v[NQ];
  load_be<NQ>(sk, sk_seed);
  wots_chain_end<NQ, Dev>(mid, sk_seed, layer, layer_tree(a.p, sp, layer), leaf, c, v);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.ends[g * NQ + i] = v[i];
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_leaf(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.p.d * a.leaves;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), layer = r / a.leaves, leaf = r - layer * a.leaves;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.sk + inst * a.sk_stride + 2 * a.p.n, mid);
  uint32_t out[NQ];
  const uint32_t* ends = a.ends + g * a.len * NQ;
  wots_pk<NQ, Dev>(mid, layer, layer_tree(a.p, sp, layer), leaf, [&](size_t w) { return ends[w]; }, out);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.nodes[g * NQ + i] = out[i];
}

// Packed: tree T = instance d + layer is a global index, its leaves are nodes[T 2^h' ...], and workgroup wg holds the 512 / 2^h' trees from wg 512 / 2^h' on
// (64 at h' = 3, 32 at h' = 4, 2 at h' = 8, 1 at h' = 9), each reduced in place inside its own 2^h' nodes of LDS.  The trees of one workgroup may belong to
// different instances, so to different keys: lane `tid` stays with tree tid >> (h' - 1) of the workgroup on every level (node tid mod 2^(h' - 1) of it, while
// the level has that many), and makes that tree's midstate once.  Address, leaf index, path slots and the message slot of the root all come from T.
template <int NQ> __global__ __launch_bounds__(256) void k_sg_tree(SgArgs a) {
  __shared__ uint32_t lds[kSgLeaves * NQ];
  const uint32_t tid = threadIdx.x;
  const size_t wg = a.first / 256 + blockIdx.x, trees = a.count * a.p.d;
  const size_t first_tree = wg * (kSgLeaves >> a.p.hp);
  if (first_tree >= trees) return;                                         // the whole workgroup
  const size_t total = trees * a.leaves * NQ, from = wg * kSgLeaves * NQ;  // in words of the nodes section
  for (uint32_t t = tid; t < kSgLeaves * NQ; t += 256)
    if (from + t < total) lds[t] = a.nodes[from + t];                      // the last workgroup may be partly empty
  const uint32_t lt = tid >> (a.p.hp - 1), i = tid & ((a.leaves >> 1) - 1);
  const size_t tree_id = first_tree + lt;
  const bool have = tree_id < trees;
  // a lane past the last tree (the last workgroup only) stays for the barriers: it reads the digest and the key of instance 0, which are in bounds whatever
  // `count` is, makes a midstate it never uses (one compression) and stores nothing -- every store below is under `have`
  const size_t inst = have ? tree_id / a.p.d : 0;
  const uint32_t layer = have ? (uint32_t)(tree_id - inst * a.p.d) : 0;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t b) { return d[b]; });
  const uint64_t tree = layer_tree(a.p, sp, layer);
  const uint32_t idx = layer_leaf(a.p, sp, layer);
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.sk + inst * a.sk_stride + 2 * a.p.n, mid);
  uint8_t* auth = a.sig + inst * a.sig_len + xmss_off(a, layer) + (size_t)a.len * a.p.n;
  uint32_t* mine = lds + ((size_t)lt << a.p.hp) * NQ;
  __syncthreads();
  if (have) {
#pragma clang loop unroll(disable)
    for (uint32_t e = 0; e < 2; ++e)
      if (is_auth_node(idx, 0, 2 * i + e)) {
        uint32_t v[NQ];
#pragma unroll
        for (int w = 0; w < NQ; ++w) v[w] = mine[(2 * i + e) * NQ + w];
        store_be<NQ>(auth, v);
      }
  }
  for (uint32_t z = 1; z <= a.p.hp; ++z) {
    const bool act = have && i < (a.leaves >> z);
    uint32_t out[NQ];
    if (act) {
      uint32_t l[NQ], r[NQ];
#pragma unroll
      for (int w = 0; w < NQ; ++w) { l[w] = mine[2 * i * NQ + w]; r[w] = mine[(2 * i + 1) * NQ + w]; }
      xmss_parent<NQ, Dev>(mid, layer, tree, z, i, l, r, out);
    }
    __syncthreads();
    if (act) {
#pragma unroll
      for (int w = 0; w < NQ; ++w) mine[i * NQ + w] = out[w];
      if (z < a.p.hp) {
        if (is_auth_node(idx, z, i)) store_be<NQ>(auth + (size_t)z * a.p.n, out);
      } else if (layer + 1 < a.p.d) {                                      // the root: what layer + 1 signs
#pragma unroll
        for (int w = 0; w < NQ; ++w) a.msgs[(tree_id + 1) * kSgMsgWords + w] = out[w];
      }
    }
    __syncthreads();
  }
}

template <int NQ> __global__ __launch_bounds__(256) void k_sg_wots(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.p.d * a.len;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), layer = r / a.len, c = r - layer * a.len;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint32_t* m1 = a.msgs + (inst * a.p.d + layer) * kSgMsgWords;
  const uint32_t digit = wots_digit(a.p.n, [&](uint32_t i) { return byte_of(m1, i); }, c);
  const uint8_t* sk = a.sk + inst * a.sk_stride;
  Mid<NQ> mid;
  mid_f<NQ, Dev>(sk + 2 * a.p.n, mid);
  uint32_t sk_seed[NQ], v[NQ];
  load_be<NQ>(sk, sk_seed);
  wots_sig_value<NQ, Dev>(mid, sk_seed, layer, layer_tree(a.p, sp, layer), layer_leaf(a.p, sp, layer), c, digit, v);
  store_be<NQ>(a.sig + inst * a.sig_len + xmss_off(a, layer) + (size_t)c * a.p.n, v);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
// workgroups of k_sg_fors per instance: k 2^(a - 9) subtrees, or the k trees 2^(9 - a) to a workgroup
uint32_t fors_wgs(const Params& p) {
  return p.a >= kSgForsHeight ? p.k << (p.a - kSgForsHeight) : (p.k + (1u << (kSgForsHeight - p.a)) - 1) >> (kSgForsHeight - p.a);
}
// the sections, their order and their sizes are those of psf_slhdsa_sign.hip: a node is n bytes there and here
struct SignWs : Layout { size_t digest, fors_sub, fors_roots, msgs, ends, nodes; };
SignWs sign_ws(const Params& p, size_t count) {
  SignWs w;
  const u128 c = count, leaves = (u128)1 << p.hp;
  w.digest = w.take(c * kSgDigestBytes);
  w.fors_sub = w.take(p.a > kSgForsHeight ? c * ((u128)p.k << (p.a - kSgForsHeight)) * p.n : (u128)0);
  w.fors_roots = w.take(c * p.k * p.n);
  w.msgs = w.take(c * p.d * 4 * kSgMsgWords);
  w.ends = w.take(c * p.d * leaves * wots_len(p.n) * p.n);
  w.nodes = w.take(c * p.d * leaves * p.n);
  return w;
}

template <int NQ> psf_status sign_run_nq(SgArgs a, hipStream_t st) {
  const size_t c = a.count, tree_wgs = (c * a.p.d + (kSgLeaves >> a.p.hp) - 1) / (kSgLeaves >> a.p.hp);
  PSF_TRY(launch_chunked(k_sg_prf_msg<NQ>, c, a, st));
  PSF_TRY(launch_chunked(k_sg_digest<NQ>, c, a, st));
  PSF_TRY(launch_chunked(k_sg_fors<NQ>, c * a.fors_wgs * 256, a, st));
  if (a.p.a > kSgForsHeight) PSF_TRY(launch_chunked(k_sg_fors_top<NQ>, c * a.p.k, a, st));
  PSF_TRY(launch_chunked(k_sg_fors_pk<NQ>, c, a, st));
  PSF_TRY(launch_chunked(k_sg_chains<NQ>, c * a.p.d * a.leaves * a.len, a, st));
  PSF_TRY(launch_chunked(k_sg_leaf<NQ>, c * a.p.d * a.leaves, a, st));
  PSF_TRY(launch_chunked(k_sg_tree<NQ>, tree_wgs * 256, a, st));
  PSF_TRY(launch_chunked(k_sg_wots<NQ>, c * a.p.d * a.len, a, st));
  return PSF_OK;
}
struct SignIn { const uint8_t* sk; size_t sk_stride; const uint8_t* msg; size_t msg_len, msg_stride; const uint8_t* addrnd; };
psf_status sign_run(int device, const Params& p, size_t count, const SignIn& in, uint8_t* sig, void* ws, const SignWs& w, hipStream_t st) {
  PSF_TRY(use_device(device));
  const SgArgs a{0, count, in.sk_stride, in.msg_len, in.msg_stride, sig_bytes(p), in.addrnd ? p.n : in.sk_stride, p, wots_len(p.n), 1u << p.hp, fors_wgs(p), in.sk, in.msg,
                 in.addrnd ? in.addrnd : in.sk + 2 * p.n, sig,
                 at<uint8_t>(ws, w.digest), at<uint32_t>(ws, w.fors_sub), at<uint32_t>(ws, w.fors_roots), at<uint32_t>(ws, w.msgs), at<uint32_t>(ws, w.ends),
                 at<uint32_t>(ws, w.nodes)};
  if (p.n == 16) PSF_TRY(sign_run_nq<4>(a, st));
  else if (p.n == 24) PSF_TRY(sign_run_nq<6>(a, st));
  else PSF_TRY(sign_run_nq<8>(a, st));
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

// the header's order: param, count = 0, NULL pointers, strides, byte counts, the workspace, overlaps; then the instance limit
psf_status sign_check(int param, size_t count, const SignIn& in, uint8_t* sig, bool dev, const void* ws, size_t ws_bytes, Params* p, SignWs* w) {
  if (!set_of(param, p)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const size_t n = p->n;
  Buf b[4] = {{in.sk, 4 * n, in.sk_stride, false, false, 0}, {in.msg, in.msg_len, in.msg_stride, false, in.msg_len == 0, 0}, {in.addrnd, n, n, false, true, 0},
              {sig, sig_bytes(*p), sig_bytes(*p), true, false, 0}};
  PSF_TRY(check_null(b, 4));
  if ((in.sk_stride != 0 && in.sk_stride < 4 * n) || in.msg_stride < in.msg_len) return PSF_ERR_PARAM;
  if (in.msg_len > SIZE_MAX / 8 - 256) return PSF_ERR_PARAM;               // a block and 3 n + msg_len as a bit length
  *w = sign_ws(*p, count);
  PSF_TRY(check_rest(count, b, 4, *w, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

}  // namespace slh2
}  // namespace psf

using namespace psf;
using namespace psf::slh2;

extern "C" {

psf_status psf_slhdsa_sha2_sign_workspace_bytes(int param, size_t count, size_t* bytes) {
  Params p;
  if (!slh2::set_of(param, &p) || !bytes) return PSF_ERR_PARAM;
  const SignWs w = sign_ws(p, count);
  if (!w.ok) return PSF_ERR_PARAM;
  *bytes = w.total;
  return PSF_OK;
}

psf_status psf_slhdsa_sha2_sign_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len,
                                    size_t msg_stride, const uint8_t* d_addrnd, uint8_t* d_sig, void* d_ws, size_t ws_bytes, void* stream) {
  Params p;
  SignWs w{};
  const SignIn in{d_sk, sk_stride, d_msg, msg_len, msg_stride, d_addrnd};
  const psf_status rc = sign_check(param, count, in, d_sig, true, d_ws, ws_bytes, &p, &w);
  if (rc != PSF_OK || count == 0) return rc;
  return sign_run(device, p, count, in, d_sig, d_ws, w, (hipStream_t)stream);
}

psf_status psf_slhdsa_sha2_sign(int device, int param, size_t count, const uint8_t* sk, size_t sk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                                const uint8_t* addrnd, uint8_t* sig) {
  Params p;
  SignWs w{};
  const SignIn in{sk, sk_stride, msg, msg_len, msg_stride, addrnd};
  const psf_status rc = sign_check(param, count, in, sig, false, nullptr, 0, &p, &w);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  const size_t n = p.n, sig_len = sig_bytes(p);
  HostCall h;
  const SignIn din{h.in(sk, count, 4 * n, sk_stride, SECRET), sk_stride ? 4 * n : 0, h.in(msg, count, msg_len, msg_stride), msg_len, msg_len, h.in(addrnd, count, n, n, SECRET)};
  uint8_t* dsig = h.out(count * sig_len);
  void* dws = h.workspace(w.total);
  PSF_TRY(h.status());
  PSF_TRY(sign_run(device, p, count, din, dsig, dws, w, nullptr));
  return h.fetch(sig, dsig, count * sig_len);
}

}  // extern "C"
