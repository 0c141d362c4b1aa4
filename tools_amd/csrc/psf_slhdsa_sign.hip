// psf_slhdsa_sign.hip -- SLH-DSA signing on the device, batched: slh_sign_internal (FIPS 205 Algorithm 19) for the six SHAKE parameter sets, bytes in and
// bytes out, `count` instances per call.  FIPS 205's text is psf_slhdsa_core.hpp and psf_slhdsa_sign_core.hpp; this unit adds the kernels and the glue.
// Every layer's (tree address, leaf index) follows from the digest, so the d XMSS trees of a signature are built side by side in the same launches; only
// the WOTS+ MESSAGE of layer j waits for layer j - 1 (its root; the FORS public key for j = 0).  NW = n / 8 = 2, 3, 4.
//   k_sg_prf_msg       one lane per instance: R = PRF_msg(SK.prf, opt_rand, M) -> sig[0, n)
//   k_sg_digest        one lane per instance: 64 bytes of H_msg(R, PK.seed, PK.root, M) -> the workspace
//   k_sg_fors<NW>      one workgroup per 512 FORS leaves (one subtree of height 9 when a >= 9, else 2^(9 - a) whole trees): PRF and F per leaf in
//                      registers, the leaves in LDS, min(a, 9) levels of H; the revealed secret value and path slots 0 ... min(a, 9) - 1 -> the
//                      signature; the tree root (a <= 9) or subtree root (a > 9) -> the workspace
//   k_sg_fors_top<NW>  a > 9 only: one lane per (instance, tree): the 2^(a - 9) subtree roots reduced in place; path slots 10 ... a - 1; the tree root
//   k_sg_fors_pk<NW>   one lane per instance: T_k over the k roots -> the message of layer 0
//   k_sg_chains<NW>    one lane per (instance, layer, leaf, chain): PRF and the 15 steps of F; the chain END (public) -> the workspace
//   k_sg_leaf<NW>      one lane per (instance, layer, leaf): T_len over the len chain ends -> the leaf
//   k_sg_tree<NW>      one workgroup per (instance, layer): the 2^h' leaves in LDS, h' levels of H; the h' path nodes -> the signature; the root -> the
//                      message of layer j + 1
//   k_sg_wots<NW>      one lane per (instance, layer, chain): PRF and `digit` steps of F, recomputed -> the signature
// No secret leaves registers: the stores of every kernel write a value that the signature reveals or that a verifier recomputes from it (DESIGN.md
// "SLH-DSA: signing" goes through them one by one).  Every index, digit, branch and loop bound comes from the digest or a root.  Lane and byte indices
// are size_t; every stage goes through launch_chunked.
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_keccak_core.hpp"
#include "psf_slhdsa_api.hpp"
#include "psf_slhdsa_sign_core.hpp"

namespace psf {
namespace slh {

// `first`: the launches of one stage are chunks of at most 2^31 - 1 workgroups; lane g of the stage is first + its index in the launch, and workgroup
// first / 256 + blockIdx.x where a workgroup is the unit
struct SgArgs {
  size_t first, count, sk_stride, msg_len, msg_stride, sig_len, rnd_stride;
  Params p;
  uint32_t len, leaves, fors_wgs;
  const uint8_t* sk; const uint8_t* msg; const uint8_t* opt_rand;             // opt_rand of instance c at opt_rand + c rnd_stride: addrnd, or PK.seed in the key
  uint8_t* sig;
  uint64_t* digest; uint64_t* fors_sub; uint64_t* fors_roots; uint64_t* msgs; uint64_t* ends; uint64_t* nodes;
};
constexpr int kSgDigestWords = 8, kSgMsgWords = 4;                         // per instance: 64 bytes of H_msg; per (instance, layer): 32 bytes of message
constexpr uint32_t kSgLeaves = 512, kSgForsHeight = 9;                     // the leaves of one workgroup, FORS and XMSS (h' <= 9)

__device__ __forceinline__ const uint8_t* digest_of(const SgArgs& a, size_t inst) { return reinterpret_cast<const uint8_t*>(a.digest + inst * kSgDigestWords); }
__device__ __forceinline__ size_t fors_off(const SgArgs& a, uint32_t t) { return (size_t)a.p.n + (size_t)t * (a.p.a + 1) * a.p.n; }
__device__ __forceinline__ size_t xmss_off(const SgArgs& a, uint32_t layer) {
  return (size_t)(1 + a.p.k * (1 + a.p.a)) * a.p.n + (size_t)layer * (a.len + a.p.hp) * a.p.n;
}

__global__ __launch_bounds__(256) void k_sg_prf_msg(SgArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint8_t* sig = a.sig + c * a.sig_len;
  asm volatile("" : "+v"(sig));                                            // the lane's own pointer, formed before the sponge's unrolled reads take the scalar registers
  uint64_t r[4];
  prf_msg<kc::DevOps>(a.p.n, a.sk + c * a.sk_stride + a.p.n, a.opt_rand + c * a.rnd_stride, a.msg + c * a.msg_stride, a.msg_len, r);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (8 * (uint32_t)i < a.p.n) {                                         // n = 16, 24, 32: whole words
#pragma unroll
      for (int k = 0; k < 8; ++k) sig[8 * i + k] = (uint8_t)(r[i] >> (8 * k));
    }
}

__global__ __launch_bounds__(256) void k_sg_digest(SgArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint64_t d[kSgDigestWords];
  h_msg<kc::DevOps>(a.p.n, a.sig + c * a.sig_len, a.sk + c * a.sk_stride + 2 * a.p.n, a.msg + c * a.msg_stride, a.msg_len, d);
#pragma unroll
  for (int i = 0; i < kSgDigestWords; ++i) a.digest[c * kSgDigestWords + i] = d[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_fors(SgArgs a) {
  __shared__ uint64_t lds[kSgLeaves * NW];
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
  uint64_t seed[NW], sk_seed[NW];
  load_words<NW>(sk + 2 * a.p.n, seed);
  load_words<NW>(sk, sk_seed);
  const uint32_t top = a.p.a < kSgForsHeight ? a.p.a : kSgForsHeight;
#pragma clang loop unroll(disable)
  for (uint32_t j = tid; j < kSgLeaves; j += 256) {
    const uint32_t leaf = base + j, t = leaf >> a.p.a, x = leaf & ((1u << a.p.a) - 1);
    if (t < a.p.k) {                                                       // the last workgroup of an f set is partly empty
      const uint32_t idx = base_2b(dbyte, a.p.a, t);
      uint8_t* ts = sig + fors_off(a, t);
      uint64_t v[NW];
      fors_sk<NW, kc::DevOps>(seed, sk_seed, sp.idx_tree, sp.idx_leaf, leaf, v);
      if (x == idx) store_words<NW>(ts, v);                                // the one secret value the signature reveals
      fors_leaf<NW, kc::DevOps>(seed, sp.idx_tree, sp.idx_leaf, leaf, v, v);
      if (is_auth_node(idx, 0, x)) store_words<NW>(ts + a.p.n, v);
#pragma unroll
      for (int i = 0; i < NW; ++i) lds[j * NW + i] = v[i];
    }
  }
  __syncthreads();
  for (uint32_t z = 1; z <= top; ++z) {
    const uint32_t node = (base >> z) + tid, t = node >> (a.p.a - z);      // node `tid` of this workgroup at height z, in the index space of the k trees
    const bool act = tid < (kSgLeaves >> z) && t < a.p.k;
    uint64_t out[NW];
    if (act) {
      uint64_t l[NW], r[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) { l[i] = lds[2 * tid * NW + i]; r[i] = lds[(2 * tid + 1) * NW + i]; }
      fors_parent<NW, kc::DevOps>(seed, sp.idx_tree, sp.idx_leaf, z, node, l, r, out);
    }
    __syncthreads();
    if (act) {
#pragma unroll
      for (int i = 0; i < NW; ++i) lds[tid * NW + i] = out[i];
      const uint32_t x = node & ((1u << (a.p.a - z)) - 1);
      if (z < a.p.a) {
        if (is_auth_node(base_2b(dbyte, a.p.a, t), z, x)) store_words<NW>(sig + fors_off(a, t) + (size_t)(1 + z) * a.p.n, out);
        if (z == kSgForsHeight) {                                          // a > 9: the root of subtree x of tree t
#pragma unroll
          for (int i = 0; i < NW; ++i) a.fors_sub[(((inst * a.p.k + t) << (a.p.a - kSgForsHeight)) + x) * NW + i] = out[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) a.fors_roots[(inst * a.p.k + t) * NW + i] = out[i];
      }
    }
    __syncthreads();
  }
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_fors_top(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.p.k) return;
  const size_t inst = g / a.p.k;
  const uint32_t t = (uint32_t)(g - inst * a.p.k);
  const uint8_t* d = digest_of(a, inst);
  auto dbyte = [&](uint32_t i) { return d[i]; };
  const Split sp = digest_split(a.p, dbyte);
  const uint32_t idx = base_2b(dbyte, a.p.a, t);
  uint64_t seed[NW];
  load_words<NW>(a.sk + inst * a.sk_stride + 2 * a.p.n, seed);
  uint8_t* ts = a.sig + inst * a.sig_len + fors_off(a, t);
  uint64_t* sub = a.fors_sub + (g << (a.p.a - kSgForsHeight)) * NW;        // this tree's subtree roots, reduced in place: node i overwrites a child of node <= i
#pragma clang loop unroll(disable)
  for (uint32_t z = kSgForsHeight + 1; z <= a.p.a; ++z) {
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < (1u << (a.p.a - z)); ++i) {
      uint64_t l[NW], r[NW], out[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) { l[w] = sub[2 * i * NW + w]; r[w] = sub[(2 * i + 1) * NW + w]; }
      fors_parent<NW, kc::DevOps>(seed, sp.idx_tree, sp.idx_leaf, z, (t << (a.p.a - z)) + i, l, r, out);
#pragma unroll
      for (int w = 0; w < NW; ++w) sub[i * NW + w] = out[w];
      if (z < a.p.a) {
        if (is_auth_node(idx, z, i)) store_words<NW>(ts + (size_t)(1 + z) * a.p.n, out);
      } else {
#pragma unroll
        for (int w = 0; w < NW; ++w) a.fors_roots[g * NW + w] = out[w];
      }
    }
  }
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_fors_pk(SgArgs a) {
  const size_t c = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* d = digest_of(a, c);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  uint64_t seed[NW], out[NW];
  load_words<NW>(a.sk + c * a.sk_stride + 2 * a.p.n, seed);
  const uint64_t* roots = a.fors_roots + c * a.p.k * NW;
  fors_pk<NW, kc::DevOps>(seed, sp.idx_tree, sp.idx_leaf, a.p.k, [&](size_t w) { return roots[w]; }, out);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.msgs[c * a.p.d * kSgMsgWords + i] = out[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_chains(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per_layer = (size_t)a.leaves * a.len, per = a.p.d * per_layer;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), layer = r / (uint32_t)per_layer, r2 = r - layer * (uint32_t)per_layer, leaf = r2 / a.len, c = r2 - leaf * a.len;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint8_t* sk = a.sk + inst * a.sk_stride;
  uint64_t seed[NW], sk_seed[NW], v[NW];
  load_words<NW>(sk + 2 * a.p.n, seed);
  load_words<NW>(sk, sk_seed);
  wots_chain_end<NW, kc::DevOps>(seed, sk_seed, layer, layer_tree(a.p, sp, layer), leaf, c, v);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.ends[g * NW + i] = v[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_leaf(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.p.d * a.leaves;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), layer = r / a.leaves, leaf = r - layer * a.leaves;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  uint64_t seed[NW], out[NW];
  load_words<NW>(a.sk + inst * a.sk_stride + 2 * a.p.n, seed);
  const uint64_t* ends = a.ends + g * a.len * NW;
  wots_pk<NW, kc::DevOps>(seed, layer, layer_tree(a.p, sp, layer), leaf, [&](size_t w) { return ends[w]; }, out);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.nodes[g * NW + i] = out[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_tree(SgArgs a) {
  __shared__ uint64_t lds[kSgLeaves * NW];
  const uint32_t tid = threadIdx.x;
  const size_t wg = a.first / 256 + blockIdx.x;
  if (wg >= a.count * a.p.d) return;                                       // the whole workgroup
  const size_t inst = wg / a.p.d;
  const uint32_t layer = (uint32_t)(wg - inst * a.p.d);
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint64_t tree = layer_tree(a.p, sp, layer);
  const uint32_t idx = layer_leaf(a.p, sp, layer);
  uint64_t seed[NW];
  load_words<NW>(a.sk + inst * a.sk_stride + 2 * a.p.n, seed);
  uint8_t* auth = a.sig + inst * a.sig_len + xmss_off(a, layer) + (size_t)a.len * a.p.n;
  for (uint32_t t = tid; t < a.leaves * NW; t += 256) lds[t] = a.nodes[wg * a.leaves * NW + t];
  __syncthreads();
  for (uint32_t t = tid; t < a.leaves; t += 256) {
    if (is_auth_node(idx, 0, t)) {
      uint64_t v[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) v[i] = lds[t * NW + i];
      store_words<NW>(auth, v);
    }
  }
  for (uint32_t z = 1; z <= a.p.hp; ++z) {
    const bool act = tid < (a.leaves >> z);                                // at most 256: one node per thread
    uint64_t out[NW];
    if (act) {
      uint64_t l[NW], r[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) { l[i] = lds[2 * tid * NW + i]; r[i] = lds[(2 * tid + 1) * NW + i]; }
      xmss_parent<NW, kc::DevOps>(seed, layer, tree, z, tid, l, r, out);
    }
    __syncthreads();
    if (act) {
#pragma unroll
      for (int i = 0; i < NW; ++i) lds[tid * NW + i] = out[i];
      if (z < a.p.hp) {
        if (is_auth_node(idx, z, tid)) store_words<NW>(auth + (size_t)z * a.p.n, out);
      } else if (layer + 1 < a.p.d) {                                      // the root: what layer + 1 signs
#pragma unroll
        for (int i = 0; i < NW; ++i) a.msgs[(inst * a.p.d + layer + 1) * kSgMsgWords + i] = out[i];
      }
    }
    __syncthreads();
  }
}

template <int NW> __global__ __launch_bounds__(256) void k_sg_wots(SgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.p.d * a.len;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), layer = r / a.len, c = r - layer * a.len;
  const uint8_t* d = digest_of(a, inst);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint8_t* m1 = reinterpret_cast<const uint8_t*>(a.msgs + (inst * a.p.d + layer) * kSgMsgWords);
  const uint32_t digit = wots_digit(a.p.n, [&](uint32_t i) { return m1[i]; }, c);
  const uint8_t* sk = a.sk + inst * a.sk_stride;
  uint64_t seed[NW], sk_seed[NW], v[NW];
  load_words<NW>(sk + 2 * a.p.n, seed);
  load_words<NW>(sk, sk_seed);
  wots_sig_value<NW, kc::DevOps>(seed, sk_seed, layer, layer_tree(a.p, sp, layer), layer_leaf(a.p, sp, layer), c, digit, v);
  store_words<NW>(a.sig + inst * a.sig_len + xmss_off(a, layer) + (size_t)c * a.p.n, v);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
// workgroups of k_sg_fors per instance: k 2^(a - 9) subtrees, or the k trees 2^(9 - a) to a workgroup
uint32_t fors_wgs(const Params& p) {
  return p.a >= kSgForsHeight ? p.k << (p.a - kSgForsHeight) : (p.k + (1u << (kSgForsHeight - p.a)) - 1) >> (kSgForsHeight - p.a);
}
struct SignWs : Layout { size_t digest, fors_sub, fors_roots, msgs, ends, nodes; };
SignWs sign_ws(const Params& p, size_t count) {
  SignWs w;
  const u128 c = count, leaves = (u128)1 << p.hp;
  w.digest = w.take(c * 8 * kSgDigestWords);
  w.fors_sub = w.take(p.a > kSgForsHeight ? c * ((u128)p.k << (p.a - kSgForsHeight)) * p.n : (u128)0);
  w.fors_roots = w.take(c * p.k * p.n);
  w.msgs = w.take(c * p.d * 8 * kSgMsgWords);
  w.ends = w.take(c * p.d * leaves * wots_len(p.n) * p.n);
  w.nodes = w.take(c * p.d * leaves * p.n);
  return w;
}

template <int NW> psf_status sign_run_nw(SgArgs a, hipStream_t st) {
  const size_t c = a.count;
  PSF_TRY(launch_chunked(k_sg_prf_msg, c, a, st));
  PSF_TRY(launch_chunked(k_sg_digest, c, a, st));
  PSF_TRY(launch_chunked(k_sg_fors<NW>, c * a.fors_wgs * 256, a, st));
  if (a.p.a > kSgForsHeight) PSF_TRY(launch_chunked(k_sg_fors_top<NW>, c * a.p.k, a, st));
  PSF_TRY(launch_chunked(k_sg_fors_pk<NW>, c, a, st));
  PSF_TRY(launch_chunked(k_sg_chains<NW>, c * a.p.d * a.leaves * a.len, a, st));
  PSF_TRY(launch_chunked(k_sg_leaf<NW>, c * a.p.d * a.leaves, a, st));
  PSF_TRY(launch_chunked(k_sg_tree<NW>, c * a.p.d * 256, a, st));
  PSF_TRY(launch_chunked(k_sg_wots<NW>, c * a.p.d * a.len, a, st));
  return PSF_OK;
}
struct SignIn { const uint8_t* sk; size_t sk_stride; const uint8_t* msg; size_t msg_len, msg_stride; const uint8_t* addrnd; };
psf_status sign_run(int device, const Params& p, size_t count, const SignIn& in, uint8_t* sig, void* ws, const SignWs& w, hipStream_t st) {
  PSF_TRY(use_device(device));
  const SgArgs a{0, count, in.sk_stride, in.msg_len, in.msg_stride, sig_bytes(p), in.addrnd ? p.n : in.sk_stride, p, wots_len(p.n), 1u << p.hp, fors_wgs(p), in.sk, in.msg,
                 in.addrnd ? in.addrnd : in.sk + 2 * p.n, sig,
                 at<uint64_t>(ws, w.digest), at<uint64_t>(ws, w.fors_sub), at<uint64_t>(ws, w.fors_roots), at<uint64_t>(ws, w.msgs), at<uint64_t>(ws, w.ends),
                 at<uint64_t>(ws, w.nodes)};
  if (p.n == 16) PSF_TRY(sign_run_nw<2>(a, st));
  else if (p.n == 24) PSF_TRY(sign_run_nw<3>(a, st));
  else PSF_TRY(sign_run_nw<4>(a, st));
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
  if (in.msg_len > SIZE_MAX - 3 * n) return PSF_ERR_PARAM;
  *w = sign_ws(*p, count);
  PSF_TRY(check_rest(count, b, 4, *w, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

}  // namespace slh
}  // namespace psf

using namespace psf;
using namespace psf::slh;

extern "C" {

psf_status psf_slhdsa_sign_workspace_bytes(int param, size_t count, size_t* bytes) {
  Params p;
  if (!set_of(param, &p) || !bytes) return PSF_ERR_PARAM;
  const SignWs w = sign_ws(p, count);
  if (!w.ok) return PSF_ERR_PARAM;
  *bytes = w.total;
  return PSF_OK;
}

psf_status psf_slhdsa_sign_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                               const uint8_t* d_addrnd, uint8_t* d_sig, void* d_ws, size_t ws_bytes, void* stream) {
  Params p;
  SignWs w{};
  const SignIn in{d_sk, sk_stride, d_msg, msg_len, msg_stride, d_addrnd};
  const psf_status rc = sign_check(param, count, in, d_sig, true, d_ws, ws_bytes, &p, &w);
  if (rc != PSF_OK || count == 0) return rc;
  return sign_run(device, p, count, in, d_sig, d_ws, w, (hipStream_t)stream);
}

psf_status psf_slhdsa_sign(int device, int param, size_t count, const uint8_t* sk, size_t sk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
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
