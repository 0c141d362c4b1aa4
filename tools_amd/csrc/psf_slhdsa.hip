// psf_slhdsa.hip -- SLH-DSA (FIPS 205, August 2024) on the device, batched: slh_keygen_internal (Algorithm 18) and slh_verify_internal (Algorithm 20)
// for the six SHAKE parameter sets, bytes in and bytes out, `count` instances per call.  The sponge is psf_keccak_core.hpp; FIPS 205's own part is
// psf_slhdsa_core.hpp (F and H as one permutation over a block built in registers); this unit adds the kernels and the glue.  NW = n / 8 = 2, 3, 4.
//   k_kg_chains<NW>   KeyGen: one lane per (instance, leaf, chain) of the top XMSS tree: PRF and the 15 steps of F; the chain END (public) to the workspace
//   k_kg_leaf<NW>     KeyGen: one lane per (instance, leaf): T_len over the len chain ends -> the leaf
//   k_kg_tree<NW>     KeyGen: one workgroup per instance: the 2^h' leaves in LDS, h' levels of H; PK.root, pk and sk
//   k_vf_digest       Verify: one lane per instance: H_msg(R, PK.seed, PK.root, M), 64 bytes to the workspace
//   k_vf_fors<NW>     Verify: one lane per (instance, FORS tree): F of the secret value and the a steps up its path -> the root of the tree
//   k_vf_fors_pk<NW>  Verify: one lane per instance: T_k over the k roots -> the message of layer 0
//   k_vf_wots<NW>     Verify, once per layer: one lane per (instance, chain): the signature value walked 15 - digit steps -> the chain end
//   k_vf_xmss<NW>     Verify, once per layer: one lane per instance: T_len over the chain ends, the h' steps up the path; the last layer compares with PK.root
// One lane per unit of work and one Keccak state per lane throughout; lane and byte indices are size_t.  KeyGen's secrets (the WOTS+ secret values and
// the chain intermediates) exist in registers only; the workspace holds public values and the last operation of KeyGen clears it all the same.
// Verification has no secret (DESIGN.md "SLH-DSA").
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_keccak_core.hpp"
#include "psf_slhdsa_api.hpp"
#include "psf_slhdsa_core.hpp"

namespace psf {
namespace slh {

// ---- KeyGen ----------------------------------------------------------------------------------------------------------------------------------------------
// `first`: the launches of one stage are chunks of at most 2^31 - 1 workgroups; lane g of the stage is first + its index in the launch
struct KgArgs {
  size_t first, count;
  uint32_t n, len, leaves, layer;
  const uint8_t* sk_seed; const uint8_t* sk_prf; const uint8_t* pk_seed;
  uint64_t* ends; uint64_t* nodes;
  uint8_t* pk; uint8_t* sk;
};

template <int NW> __global__ __launch_bounds__(256) void k_kg_chains(KgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.leaves * a.len;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), leaf = r / a.len, c = r - leaf * a.len;
  uint64_t seed[NW], sk_seed[NW], v[NW];
  load_words<NW>(a.pk_seed + inst * a.n, seed);
  load_words<NW>(a.sk_seed + inst * a.n, sk_seed);
  wots_chain_end<NW, kc::DevOps>(seed, sk_seed, a.layer, 0, leaf, c, v);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.ends[g * NW + i] = v[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_kg_leaf(KgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.leaves) return;
  const size_t inst = g / a.leaves;
  const uint32_t leaf = (uint32_t)(g - inst * a.leaves);
  uint64_t seed[NW], out[NW];
  load_words<NW>(a.pk_seed + inst * a.n, seed);
  const uint64_t* ends = a.ends + g * a.len * NW;
  wots_pk<NW, kc::DevOps>(seed, a.layer, 0, leaf, [&](size_t w) { return ends[w]; }, out);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.nodes[g * NW + i] = out[i];
}

constexpr uint32_t kMaxLeaves = 512;                                       // h' <= 9

template <int NW> __global__ __launch_bounds__(256) void k_kg_tree(KgArgs a) {
  __shared__ uint64_t lds[kMaxLeaves * NW];
  const uint32_t tid = threadIdx.x;
  for (size_t inst = a.first + blockIdx.x; inst < a.count; inst += gridDim.x) {
    uint64_t seed[NW];
    load_words<NW>(a.pk_seed + inst * a.n, seed);
    for (uint32_t t = tid; t < a.leaves * NW; t += 256) lds[t] = a.nodes[inst * a.leaves * NW + t];
    __syncthreads();
    uint32_t z = 0;
    for (uint32_t width = a.leaves / 2; width >= 1; width /= 2) {
      ++z;
      const bool act = tid < width;                                        // width <= 256: one node per thread
      uint64_t out[NW];
      if (act) {
        uint64_t l[NW], r[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) { l[i] = lds[2 * tid * NW + i]; r[i] = lds[(2 * tid + 1) * NW + i]; }
        xmss_parent<NW, kc::DevOps>(seed, a.layer, 0, z, tid, l, r, out);
      }
      __syncthreads();
      if (act) {
#pragma unroll
        for (int i = 0; i < NW; ++i) lds[tid * NW + i] = out[i];
      }
      __syncthreads();
    }
    // pk = PK.seed || PK.root, sk = SK.seed || SK.prf || PK.seed || PK.root
    uint8_t* pk = a.pk + inst * 2 * a.n;
    uint8_t* sk = a.sk + inst * 4 * a.n;
    if (tid < a.n) {
      const uint8_t s = a.pk_seed[inst * a.n + tid];
      pk[tid] = s;
      sk[2 * a.n + tid] = s;
      sk[tid] = a.sk_seed[inst * a.n + tid];
      sk[a.n + tid] = a.sk_prf[inst * a.n + tid];
      const uint8_t rb = (uint8_t)(lds[tid >> 3] >> (8 * (tid & 7)));
      pk[a.n + tid] = rb;
      sk[3 * a.n + tid] = rb;
    }
    __syncthreads();
  }
}

// ---- Verify ----------------------------------------------------------------------------------------------------------------------------------------------
struct VfArgs {
  size_t count, pk_stride, msg_len, msg_stride, sig_len;
  Params p;
  uint32_t len, layer, last;
  const uint8_t* pk; const uint8_t* msg; const uint8_t* sig;
  uint64_t* digest; uint64_t* roots; uint64_t* node; uint64_t* ends;
  uint8_t* ok;
};
constexpr int kDigestWords = 8, kNodeWords = 4;                            // per instance in the workspace: 64 bytes of H_msg, 32 bytes of the current node

__global__ __launch_bounds__(256) void k_vf_digest(VfArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint64_t d[kDigestWords];
  h_msg<kc::DevOps>(a.p.n, a.sig + c * a.sig_len, a.pk + c * a.pk_stride, a.msg + c * a.msg_stride, a.msg_len, d);
#pragma unroll
  for (int i = 0; i < kDigestWords; ++i) a.digest[c * kDigestWords + i] = d[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_vf_fors(VfArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.p.k) return;
  const size_t c = g / a.p.k;
  const uint32_t t = (uint32_t)(g - c * a.p.k);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(a.digest + c * kDigestWords);
  auto dbyte = [&](uint32_t i) { return d[i]; };
  const Split sp = digest_split(a.p, dbyte);
  uint64_t seed[NW], node[NW];
  load_words<NW>(a.pk + c * a.pk_stride, seed);
  fors_root<NW, kc::DevOps>(seed, sp.idx_tree, sp.idx_leaf, a.p.a, t, base_2b(dbyte, a.p.a, t), a.sig + c * a.sig_len + a.p.n + (size_t)t * (a.p.a + 1) * a.p.n, node);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.roots[g * NW + i] = node[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_vf_fors_pk(VfArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* d = reinterpret_cast<const uint8_t*>(a.digest + c * kDigestWords);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  uint64_t seed[NW], out[NW];
  load_words<NW>(a.pk + c * a.pk_stride, seed);
  const uint64_t* roots = a.roots + c * a.p.k * NW;
  fors_pk<NW, kc::DevOps>(seed, sp.idx_tree, sp.idx_leaf, a.p.k, [&](size_t w) { return roots[w]; }, out);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.node[c * kNodeWords + i] = out[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_vf_wots(VfArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.len) return;
  const size_t c = g / a.len;
  const uint32_t ch = (uint32_t)(g - c * a.len);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(a.digest + c * kDigestWords);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint8_t* m1 = reinterpret_cast<const uint8_t*>(a.node + c * kNodeWords);
  const uint32_t digit = wots_digit(a.p.n, [&](uint32_t i) { return m1[i]; }, ch);
  uint64_t seed[NW], v[NW];
  load_words<NW>(a.pk + c * a.pk_stride, seed);
  const uint8_t* xs = a.sig + c * a.sig_len + (size_t)(1 + a.p.k * (1 + a.p.a)) * a.p.n + (size_t)a.layer * (a.len + a.p.hp) * a.p.n;
  load_words<NW>(xs + (size_t)ch * a.p.n, v);
  wots_chain_from_sig<NW, kc::DevOps>(seed, a.layer, layer_tree(a.p, sp, a.layer), layer_leaf(a.p, sp, a.layer), ch, digit, v);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.ends[g * NW + i] = v[i];
}

template <int NW> __global__ __launch_bounds__(256) void k_vf_xmss(VfArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* d = reinterpret_cast<const uint8_t*>(a.digest + c * kDigestWords);
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint64_t tree = layer_tree(a.p, sp, a.layer);
  const uint32_t leaf = layer_leaf(a.p, sp, a.layer);
  uint64_t seed[NW], node[NW];
  const uint8_t* pk = a.pk + c * a.pk_stride;
  load_words<NW>(pk, seed);
  const uint64_t* ends = a.ends + c * a.len * NW;
  wots_pk<NW, kc::DevOps>(seed, a.layer, tree, leaf, [&](size_t w) { return ends[w]; }, node);
  const uint8_t* xs = a.sig + c * a.sig_len + (size_t)(1 + a.p.k * (1 + a.p.a)) * a.p.n + (size_t)a.layer * (a.len + a.p.hp) * a.p.n;
  xmss_root<NW, kc::DevOps>(seed, a.layer, tree, leaf, a.p.hp, xs + (size_t)a.len * a.p.n, node);
#pragma unroll
  for (int i = 0; i < NW; ++i) a.node[c * kNodeWords + i] = node[i];
  if (a.last) {
    uint64_t root[NW], diff = 0;
    load_words<NW>(pk + a.p.n, root);
#pragma unroll
    for (int i = 0; i < NW; ++i) diff |= root[i] ^ node[i];
    a.ok[c] = diff == 0 ? 1 : 0;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
bool set_of(int param, Params* p) {
  if (param < 0 || param >= kSets) return false;
  *p = kParams[param];
  return true;
}

struct KeygenWs : Layout { size_t ends, nodes; };
struct VerifyWs : Layout { size_t digest, roots, node, ends; };
KeygenWs keygen_ws(const Params& p, size_t count) {
  KeygenWs w;
  const u128 c = count, leaves = (u128)1 << p.hp;
  w.ends = w.take(c * leaves * wots_len(p.n) * p.n);
  w.nodes = w.take(c * leaves * p.n);
  return w;
}
VerifyWs verify_ws(const Params& p, size_t count) {
  VerifyWs w;
  const u128 c = count;
  w.digest = w.take(c * 8 * kDigestWords);
  w.roots = w.take(c * p.k * p.n);
  w.node = w.take(c * 8 * kNodeWords);
  w.ends = w.take(c * wots_len(p.n) * p.n);
  return w;
}
Layout ws_need(const Params& p, size_t count, int op) {
  if (op == PSF_SLHDSA_OP_KEYGEN) return keygen_ws(p, count);
  return verify_ws(p, count);
}

template <int NW> psf_status keygen_run_nw(KgArgs a, hipStream_t st) {
  PSF_TRY(launch_chunked(k_kg_chains<NW>, a.count * a.leaves * a.len, a, st));
  PSF_TRY(launch_chunked(k_kg_leaf<NW>, a.count * a.leaves, a, st));
  a.first = 0;
  hipLaunchKernelGGL(k_kg_tree<NW>, dim3((unsigned)a.count), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status keygen_run(int device, const Params& p, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk, uint8_t* sk,
                      void* ws, const KeygenWs& w, hipStream_t st) {
  PSF_TRY(use_device(device));
  const KgArgs a{0, count, p.n, wots_len(p.n), 1u << p.hp, p.d - 1, sk_seed, sk_prf, pk_seed, at<uint64_t>(ws, w.ends), at<uint64_t>(ws, w.nodes), pk, sk};
  if (p.n == 16) PSF_TRY(keygen_run_nw<2>(a, st));
  else if (p.n == 24) PSF_TRY(keygen_run_nw<3>(a, st));
  else PSF_TRY(keygen_run_nw<4>(a, st));
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

template <int NW> psf_status verify_run_nw(VfArgs a, hipStream_t st) {
  const dim3 per_inst(blocks_of(a.count, 256)), tb(256);
  hipLaunchKernelGGL(k_vf_digest, per_inst, tb, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_vf_fors<NW>, dim3(blocks_of(a.count * a.p.k, 256)), tb, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_vf_fors_pk<NW>, per_inst, tb, 0, st, a);
  HIP_TRY(hipGetLastError());
  for (uint32_t j = 0; j < a.p.d; ++j) {                                  // layer j signs the root of layer j - 1
    a.layer = j;
    a.last = j + 1 == a.p.d;
    hipLaunchKernelGGL(k_vf_wots<NW>, dim3(blocks_of(a.count * a.len, 256)), tb, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vf_xmss<NW>, per_inst, tb, 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return PSF_OK;
}
struct VerifyIn { const uint8_t* pk; size_t pk_stride; const uint8_t* msg; size_t msg_len, msg_stride; const uint8_t* sig; };
psf_status verify_run(int device, const Params& p, size_t count, const VerifyIn& in, uint8_t* ok, void* ws, const VerifyWs& w, hipStream_t st) {
  PSF_TRY(use_device(device));
  const VfArgs a{count, in.pk_stride, in.msg_len, in.msg_stride, sig_bytes(p), p, wots_len(p.n), 0, 0, in.pk, in.msg, in.sig,
                 at<uint64_t>(ws, w.digest), at<uint64_t>(ws, w.roots), at<uint64_t>(ws, w.node), at<uint64_t>(ws, w.ends), ok};
  if (p.n == 16) return verify_run_nw<2>(a, st);
  if (p.n == 24) return verify_run_nw<3>(a, st);
  return verify_run_nw<4>(a, st);
}

// ---- argument checks of the entry points: the header's order -------------------------------------------------------------------------------------------
struct Checked { Params p; Layout need; };
psf_status keygen_check(int param, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk, uint8_t* sk, bool dev,
                        const void* ws, size_t ws_bytes, Checked* ck) {
  if (!set_of(param, &ck->p)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const size_t n = ck->p.n;
  Buf b[5] = {{sk_seed, n, n, false, false, 0}, {sk_prf, n, n, false, false, 0}, {pk_seed, n, n, false, false, 0}, {pk, 2 * n, 2 * n, true, false, 0},
              {sk, 4 * n, 4 * n, true, false, 0}};
  PSF_TRY(check_null(b, 5));
  ck->need = ws_need(ck->p, count, PSF_SLHDSA_OP_KEYGEN);
  PSF_TRY(check_rest(count, b, 5, ck->need, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}
psf_status verify_check(int param, size_t count, const VerifyIn& in, uint8_t* ok, bool dev, const void* ws, size_t ws_bytes, Checked* ck) {
  if (!set_of(param, &ck->p)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  const size_t n = ck->p.n;
  Buf b[4] = {{in.pk, 2 * n, in.pk_stride, false, false, 0}, {in.msg, in.msg_len, in.msg_stride, false, in.msg_len == 0, 0},
              {in.sig, sig_bytes(ck->p), sig_bytes(ck->p), false, false, 0}, {ok, 1, 1, true, false, 0}};
  PSF_TRY(check_null(b, 4));
  if ((in.pk_stride != 0 && in.pk_stride < 2 * n) || in.msg_stride < in.msg_len) return PSF_ERR_PARAM;
  if (in.msg_len > SIZE_MAX - 3 * n) return PSF_ERR_PARAM;
  ck->need = ws_need(ck->p, count, PSF_SLHDSA_OP_VERIFY);
  PSF_TRY(check_rest(count, b, 4, ck->need, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

}  // namespace slh
}  // namespace psf

using namespace psf;
using namespace psf::slh;

extern "C" {

psf_status psf_slhdsa_sizes(int param, size_t* pk, size_t* sk, size_t* sig) {
  Params p;
  if (!set_of(param, &p)) return PSF_ERR_PARAM;
  if (pk) *pk = 2 * (size_t)p.n;
  if (sk) *sk = 4 * (size_t)p.n;
  if (sig) *sig = sig_bytes(p);
  return PSF_OK;
}

psf_status psf_slhdsa_workspace_bytes(int param, size_t count, int op, size_t* bytes) {
  Params p;
  if (!set_of(param, &p) || (op != PSF_SLHDSA_OP_KEYGEN && op != PSF_SLHDSA_OP_VERIFY) || !bytes) return PSF_ERR_PARAM;
  const Layout need = ws_need(p, count, op);
  if (!need.ok) return PSF_ERR_PARAM;
  *bytes = need.total;
  return PSF_OK;
}

psf_status psf_slhdsa_keygen_dev(int device, int param, size_t count, const uint8_t* d_sk_seed, const uint8_t* d_sk_prf, const uint8_t* d_pk_seed, uint8_t* d_pk,
                                 uint8_t* d_sk, void* d_ws, size_t ws_bytes, void* stream) {
  Checked ck{};
  const psf_status rc = keygen_check(param, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, true, d_ws, ws_bytes, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  return keygen_run(device, ck.p, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, d_ws, keygen_ws(ck.p, count), (hipStream_t)stream);
}

psf_status psf_slhdsa_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                                 const uint8_t* d_sig, uint8_t* d_ok, void* d_ws, size_t ws_bytes, void* stream) {
  Checked ck{};
  const VerifyIn in{d_pk, pk_stride, d_msg, msg_len, msg_stride, d_sig};
  const psf_status rc = verify_check(param, count, in, d_ok, true, d_ws, ws_bytes, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  return verify_run(device, ck.p, count, in, d_ok, d_ws, verify_ws(ck.p, count), (hipStream_t)stream);
}

psf_status psf_slhdsa_keygen(int device, int param, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk, uint8_t* sk) {
  Checked ck{};
  const psf_status rc = keygen_check(param, count, sk_seed, sk_prf, pk_seed, pk, sk, false, nullptr, 0, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  const size_t n = ck.p.n;
  HostCall h;
  const uint8_t *dseed = h.in(sk_seed, count, n, n, SECRET), *dprf = h.in(sk_prf, count, n, n, SECRET), *dpseed = h.in(pk_seed, count, n, n);
  uint8_t *dpk = h.out(2 * count * n), *dsk = h.out(4 * count * n, SECRET);
  void* dws = h.workspace(ck.need.total);
  PSF_TRY(h.status());
  PSF_TRY(keygen_run(device, ck.p, count, dseed, dprf, dpseed, dpk, dsk, dws, keygen_ws(ck.p, count), nullptr));
  PSF_TRY(h.fetch(pk, dpk, 2 * count * n));
  return h.fetch(sk, dsk, 4 * count * n);
}

psf_status psf_slhdsa_verify(int device, int param, size_t count, const uint8_t* pk, size_t pk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                             const uint8_t* sig, uint8_t* ok) {
  Checked ck{};
  const VerifyIn in{pk, pk_stride, msg, msg_len, msg_stride, sig};
  const psf_status rc = verify_check(param, count, in, ok, false, nullptr, 0, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  PSF_TRY(use_device(device));
  const size_t n = ck.p.n, sig_len = sig_bytes(ck.p);
  HostCall h;
  const VerifyIn din{h.in(pk, count, 2 * n, pk_stride), pk_stride ? 2 * n : 0, h.in(msg, count, msg_len, msg_stride), msg_len, msg_len, h.in(sig, count, sig_len, sig_len)};
  uint8_t* dok = h.out(count);
  void* dws = h.workspace(ck.need.total);
  PSF_TRY(h.status());
  PSF_TRY(verify_run(device, ck.p, count, din, dok, dws, verify_ws(ck.p, count), nullptr));
  return h.fetch(ok, dok, count);
}

}  // extern "C"
