// psf_slhdsa_sha2.hip -- SLH-DSA (FIPS 205, August 2024) on the device for the six SHA-2 parameter sets, batched: slh_keygen_internal (Algorithm 18) and
// slh_verify_internal (Algorithm 20), bytes in and bytes out, `count` instances per call.  The hashes are psf_sha2_core.hpp; section 11.2 and the WOTS+ /
// XMSS / FORS steps over it are psf_slhdsa_sha2_core.hpp (F, PRF and H as ONE compression past the PK.seed midstate, over a block built in registers); this
// unit adds the kernels and the glue.  The stage split is psf_slhdsa.hip's.  NQ = n / 4 = 4, 6, 8: a node is NQ big-endian 32-bit words, in registers
// and in the workspace alike.
//   k_kg_chains<NQ>   KeyGen: one lane per (instance, leaf, chain) of the top XMSS tree: PRF and the 15 steps of F; the chain END (public) to the workspace
//   k_kg_leaf<NQ>     KeyGen: one lane per (instance, leaf): T_len over the len chain ends -> the leaf
//   k_kg_tree<NQ>     KeyGen: one workgroup per instance: the 2^h' leaves in LDS, h' levels of H; PK.root, pk and sk
//   k_vf_digest<NQ>   Verify: one lane per instance: H_msg(R, PK.seed, PK.root, M), the first 64 bytes of the mask to the workspace
//   k_vf_fors<NQ>     Verify: one lane per (instance, FORS tree): F of the secret value and the a steps up its path -> the root of the tree
//   k_vf_fors_pk<NQ>  Verify: one lane per instance: T_k over the k roots -> the message of layer 0
//   k_vf_wots<NQ>     Verify, once per layer: one lane per (instance, chain): the signature value walked 15 - digit steps -> the chain end
//   k_vf_xmss<NQ>     Verify, once per layer: one lane per instance: T_len over the chain ends, the h' steps up the path; the last layer compares with PK.root
// Every lane makes the midstate(s) its stage needs from PK.seed at kernel entry, once: one compression beside the 16 of a KeyGen chain.  One lane per
// unit of work and one hash state per lane throughout; lane and byte indices are size_t.  KeyGen's secrets (the WOTS+ secret values and the chain
// intermediates) exist in registers only; the workspace holds public values and the last operation of KeyGen clears it all the same.  Verification has
// no secret (DESIGN.md "SLH-DSA: the SHA-2 sets").
#include "psf_call.hpp"
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_slhdsa_sha2_api.hpp"
#include "psf_slhdsa_sha2_core.hpp"

namespace psf {
namespace slh2 {

using Dev = sha2::DevOps;

// ---- KeyGen ----------------------------------------------------------------------------------------------------------------------------------------------
// `first`: the launches of one stage are chunks of at most 2^31 - 1 workgroups; lane g of the stage is first + its index in the launch
struct KgArgs {
  size_t first, count;
  uint32_t n, len, leaves, layer;
  const uint8_t* sk_seed; const uint8_t* sk_prf; const uint8_t* pk_seed;
  uint32_t* ends; uint32_t* nodes;
  uint8_t* pk; uint8_t* sk;
};

template <int NQ> __global__ __launch_bounds__(256) void k_kg_chains(KgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.leaves * a.len;
  if (g >= a.count * per) return;
  const size_t inst = g / per;
  const uint32_t r = (uint32_t)(g - inst * per), leaf = r / a.len, c = r - leaf * a.len;
  Mid<NQ> mid;
  mid_f<NQ, Dev>(a.pk_seed + inst * a.n, mid);
  uint32_t sk_seed[NQ], v[NQ];
  load_be<NQ>(a.sk_seed + inst * a.n, sk_seed);
  wots_chain_end<NQ, Dev>(mid, sk_seed, a.layer, 0, leaf, c, v);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.ends[g * NQ + i] = v[i];
}

template <int NQ> __global__ __launch_bounds__(256) void k_kg_leaf(KgArgs a) {
  const size_t g = a.first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.leaves) return;
  const size_t inst = g / a.leaves;
  const uint32_t leaf = (uint32_t)(g - inst * a.leaves);
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.pk_seed + inst * a.n, mid);
  uint32_t out[NQ];
  const uint32_t* ends = a.ends + g * a.len * NQ;
  wots_pk<NQ, Dev>(mid, a.layer, 0, leaf, [&](size_t w) { return ends[w]; }, out);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.nodes[g * NQ + i] = out[i];
}

constexpr uint32_t kMaxLeaves = 512;                                       // h' <= 9

template <int NQ> __global__ __launch_bounds__(256) void k_kg_tree(KgArgs a) {
  __shared__ uint32_t lds[kMaxLeaves * NQ];
  const uint32_t tid = threadIdx.x;
  const size_t inst = blockIdx.x;                                          // one workgroup per instance: the grid is `count` (at most 2^31 - 1)
  if (inst >= a.count) return;
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.pk_seed + inst * a.n, mid);
  for (uint32_t t = tid; t < a.leaves * NQ; t += 256) lds[t] = a.nodes[inst * a.leaves * NQ + t];
  __syncthreads();
  uint32_t z = 0;
  for (uint32_t width = a.leaves / 2; width >= 1; width /= 2) {
    ++z;
    const bool act = tid < width;                                        // width <= 256: one node per thread
    const uint32_t node = act ? tid : 0;                                   // an idle thread hashes node 0 again and drops it: no branch around the hash
    uint32_t out[NQ], l[NQ], r[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) { l[i] = lds[2 * node * NQ + i]; r[i] = lds[(2 * node + 1) * NQ + i]; }
    xmss_parent<NQ, Dev>(mid, a.layer, 0, z, node, l, r, out);
    __syncthreads();
    if (act) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) lds[tid * NQ + i] = out[i];
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
    const uint8_t rb = (uint8_t)byte_of(lds, tid);
    pk[a.n + tid] = rb;
    sk[3 * a.n + tid] = rb;
  }
}

// ---- Verify ----------------------------------------------------------------------------------------------------------------------------------------------
struct VfArgs {
  size_t count, pk_stride, msg_len, msg_stride, sig_len;
  Params p;
  uint32_t len, layer, last;
  const uint8_t* pk; const uint8_t* msg; const uint8_t* sig;
  uint8_t* digest; uint32_t* roots; uint32_t* node; uint32_t* ends;
  uint8_t* ok;
};
constexpr int kDigestBytes = 64, kNodeWords = 8;                           // per instance in the workspace: 64 bytes of H_msg, 32 bytes of the current node

template <int NQ> __global__ __launch_bounds__(256) void k_vf_digest(VfArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  uint8_t* out = a.digest + c * kDigestBytes;
  if constexpr (NQ == 4) h_msg_256<Dev>(a.sig + c * a.sig_len, a.pk + c * a.pk_stride, a.msg + c * a.msg_stride, a.msg_len, out);
  else h_msg_512<Dev>(a.p.n, a.sig + c * a.sig_len, a.pk + c * a.pk_stride, a.msg + c * a.msg_stride, a.msg_len, out);
}

template <int NQ> __global__ __launch_bounds__(256) void k_vf_fors(VfArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.p.k) return;
  const size_t c = g / a.p.k;
  const uint32_t t = (uint32_t)(g - c * a.p.k);
  const uint8_t* d = a.digest + c * kDigestBytes;
  auto dbyte = [&](uint32_t i) { return d[i]; };
  const Split sp = digest_split(a.p, dbyte);
  Mid<NQ> mid;
  mid_fh<NQ, Dev>(a.pk + c * a.pk_stride, mid);
  uint32_t node[NQ];
  fors_root<NQ, Dev>(mid, sp.idx_tree, sp.idx_leaf, a.p.a, t, base_2b(dbyte, a.p.a, t), a.sig + c * a.sig_len + a.p.n + (size_t)t * (a.p.a + 1) * a.p.n, node);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.roots[g * NQ + i] = node[i];
}

template <int NQ> __global__ __launch_bounds__(256) void k_vf_fors_pk(VfArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* d = a.digest + c * kDigestBytes;
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  Mid<NQ> mid;
  mid_h<NQ, Dev>(a.pk + c * a.pk_stride, mid);
  uint32_t out[NQ];
  const uint32_t* roots = a.roots + c * a.p.k * NQ;
  fors_pk<NQ, Dev>(mid, sp.idx_tree, sp.idx_leaf, a.p.k, [&](size_t w) { return roots[w]; }, out);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.node[c * kNodeWords + i] = out[i];
}

template <int NQ> __global__ __launch_bounds__(256) void k_vf_wots(VfArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count * a.len) return;
  const size_t c = g / a.len;
  const uint32_t ch = (uint32_t)(g - c * a.len);
  const uint8_t* d = a.digest + c * kDigestBytes;
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint32_t* m1 = a.node + c * kNodeWords;
  const uint32_t digit = wots_digit(a.p.n, [&](uint32_t i) { return byte_of(m1, i); }, ch);
  Mid<NQ> mid;
  mid_f<NQ, Dev>(a.pk + c * a.pk_stride, mid);
  uint32_t v[NQ];
  const uint8_t* xs = a.sig + c * a.sig_len + (size_t)(1 + a.p.k * (1 + a.p.a)) * a.p.n + (size_t)a.layer * (a.len + a.p.hp) * a.p.n;
  load_be<NQ>(xs + (size_t)ch * a.p.n, v);
  wots_chain_from_sig<NQ, Dev>(mid, a.layer, layer_tree(a.p, sp, a.layer), layer_leaf(a.p, sp, a.layer), ch, digit, v);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.ends[g * NQ + i] = v[i];
}

template <int NQ> __global__ __launch_bounds__(256) void k_vf_xmss(VfArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.count) return;
  const uint8_t* d = a.digest + c * kDigestBytes;
  const Split sp = digest_split(a.p, [&](uint32_t i) { return d[i]; });
  const uint64_t tree = layer_tree(a.p, sp, a.layer);
  const uint32_t leaf = layer_leaf(a.p, sp, a.layer);
  const uint8_t* pk = a.pk + c * a.pk_stride;
  Mid<NQ> mid;
  mid_h<NQ, Dev>(pk, mid);
  uint32_t node[NQ];
  const uint32_t* ends = a.ends + c * a.len * NQ;
  wots_pk<NQ, Dev>(mid, a.layer, tree, leaf, [&](size_t w) { return ends[w]; }, node);
  const uint8_t* xs = a.sig + c * a.sig_len + (size_t)(1 + a.p.k * (1 + a.p.a)) * a.p.n + (size_t)a.layer * (a.len + a.p.hp) * a.p.n;
  xmss_root<NQ, Dev>(mid, a.layer, tree, leaf, a.p.hp, xs + (size_t)a.len * a.p.n, node);
#pragma unroll
  for (int i = 0; i < NQ; ++i) a.node[c * kNodeWords + i] = node[i];
  if (a.last) {
    uint32_t root[NQ], diff = 0;
    load_be<NQ>(pk + a.p.n, root);
#pragma unroll
    for (int i = 0; i < NQ; ++i) diff |= root[i] ^ node[i];
    a.ok[c] = diff == 0 ? 1 : 0;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
bool set_of(int param, Params* p) {                                       // PSF_SLHDSA_SHA2_*: the SHAKE sets' (n, h, d, h', a, k, m), a numbering of its own
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
  w.digest = w.take(c * kDigestBytes);
  w.roots = w.take(c * p.k * p.n);
  w.node = w.take(c * 4 * kNodeWords);
  w.ends = w.take(c * wots_len(p.n) * p.n);
  return w;
}
Layout ws_need(const Params& p, size_t count, int op) {
  if (op == PSF_SLHDSA_OP_KEYGEN) return keygen_ws(p, count);
  return verify_ws(p, count);
}

template <int NQ> psf_status keygen_run_nq(KgArgs a, hipStream_t st) {
  PSF_TRY(launch_chunked(k_kg_chains<NQ>, a.count * a.leaves * a.len, a, st));
  PSF_TRY(launch_chunked(k_kg_leaf<NQ>, a.count * a.leaves, a, st));
  a.first = 0;
  hipLaunchKernelGGL(k_kg_tree<NQ>, dim3((unsigned)a.count), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}
psf_status keygen_run(int device, const Params& p, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk, uint8_t* sk,
                      void* ws, const KeygenWs& w, hipStream_t st) {
  PSF_TRY(use_device(device));
  const KgArgs a{0, count, p.n, wots_len(p.n), 1u << p.hp, p.d - 1, sk_seed, sk_prf, pk_seed, at<uint32_t>(ws, w.ends), at<uint32_t>(ws, w.nodes), pk, sk};
  if (p.n == 16) PSF_TRY(keygen_run_nq<4>(a, st));
  else if (p.n == 24) PSF_TRY(keygen_run_nq<6>(a, st));
  else PSF_TRY(keygen_run_nq<8>(a, st));
  HIP_TRY(hipMemsetAsync(ws, 0, w.total, st));
  return PSF_OK;
}

template <int NQ> psf_status verify_run_nq(VfArgs a, hipStream_t st) {
  const dim3 per_inst(blocks_of(a.count, 256)), tb(256);
  hipLaunchKernelGGL(k_vf_digest<NQ>, per_inst, tb, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_vf_fors<NQ>, dim3(blocks_of(a.count * a.p.k, 256)), tb, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_vf_fors_pk<NQ>, per_inst, tb, 0, st, a);
  HIP_TRY(hipGetLastError());
  for (uint32_t j = 0; j < a.p.d; ++j) {                                  // layer j signs the root of layer j - 1
    a.layer = j;
    a.last = j + 1 == a.p.d;
    hipLaunchKernelGGL(k_vf_wots<NQ>, dim3(blocks_of(a.count * a.len, 256)), tb, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vf_xmss<NQ>, per_inst, tb, 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return PSF_OK;
}
struct VerifyIn { const uint8_t* pk; size_t pk_stride; const uint8_t* msg; size_t msg_len, msg_stride; const uint8_t* sig; };
psf_status verify_run(int device, const Params& p, size_t count, const VerifyIn& in, uint8_t* ok, void* ws, const VerifyWs& w, hipStream_t st) {
  PSF_TRY(use_device(device));
  const VfArgs a{count, in.pk_stride, in.msg_len, in.msg_stride, sig_bytes(p), p, wots_len(p.n), 0, 0, in.pk, in.msg, in.sig,
                 at<uint8_t>(ws, w.digest), at<uint32_t>(ws, w.roots), at<uint32_t>(ws, w.node), at<uint32_t>(ws, w.ends), ok};
  if (p.n == 16) return verify_run_nq<4>(a, st);
  if (p.n == 24) return verify_run_nq<6>(a, st);
  return verify_run_nq<8>(a, st);
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
  if (in.msg_len > SIZE_MAX / 8 - 256) return PSF_ERR_PARAM;               // 3 n + msg_len as a bit length
  ck->need = ws_need(ck->p, count, PSF_SLHDSA_OP_VERIFY);
  PSF_TRY(check_rest(count, b, 4, ck->need, dev, ws, ws_bytes));
  return grid_fits(count) ? PSF_OK : PSF_ERR_UNSUPPORTED;
}

}  // namespace slh2
}  // namespace psf

using namespace psf;
using namespace psf::slh2;

extern "C" {

psf_status psf_slhdsa_sha2_sizes(int param, size_t* pk, size_t* sk, size_t* sig) {
  Params p;
  if (!slh2::set_of(param, &p)) return PSF_ERR_PARAM;
  if (pk) *pk = 2 * (size_t)p.n;
  if (sk) *sk = 4 * (size_t)p.n;
  if (sig) *sig = sig_bytes(p);
  return PSF_OK;
}

psf_status psf_slhdsa_sha2_workspace_bytes(int param, size_t count, int op, size_t* bytes) {
  Params p;
  if (!slh2::set_of(param, &p) || (op != PSF_SLHDSA_OP_KEYGEN && op != PSF_SLHDSA_OP_VERIFY) || !bytes) return PSF_ERR_PARAM;
  const Layout need = ws_need(p, count, op);
  if (!need.ok) return PSF_ERR_PARAM;
  *bytes = need.total;
  return PSF_OK;
}

psf_status psf_slhdsa_sha2_keygen_dev(int device, int param, size_t count, const uint8_t* d_sk_seed, const uint8_t* d_sk_prf, const uint8_t* d_pk_seed,
                                      uint8_t* d_pk, uint8_t* d_sk, void* d_ws, size_t ws_bytes, void* stream) {
  Checked ck{};
  const psf_status rc = keygen_check(param, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, true, d_ws, ws_bytes, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  return keygen_run(device, ck.p, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, d_ws, keygen_ws(ck.p, count), (hipStream_t)stream);
}

psf_status psf_slhdsa_sha2_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len,
                                      size_t msg_stride, const uint8_t* d_sig, uint8_t* d_ok, void* d_ws, size_t ws_bytes, void* stream) {
  Checked ck{};
  const VerifyIn in{d_pk, pk_stride, d_msg, msg_len, msg_stride, d_sig};
  const psf_status rc = verify_check(param, count, in, d_ok, true, d_ws, ws_bytes, &ck);
  if (rc != PSF_OK || count == 0) return rc;
  return verify_run(device, ck.p, count, in, d_ok, d_ws, verify_ws(ck.p, count), (hipStream_t)stream);
}

psf_status psf_slhdsa_sha2_keygen(int device, int param, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk,
                                  uint8_t* sk) {
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

psf_status psf_slhdsa_sha2_verify(int device, int param, size_t count, const uint8_t* pk, size_t pk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
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
