// psfp.hip -- PSFPerturbation behind the C ABI of include/psf_mi355x.h (mp_perturbation.rs:57-62, :193-403).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <string>
#include <thread>
#include <atomic>
#include <mutex>
#include <functional>
#include <vector>
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_kernels.hpp"
#include "psf_stream_kernels.hpp"
#include "psf_gpv_kernels.hpp"
#include "psf_np_kernels.hpp"
#include "psf_chol_kernels.hpp"
#include "psf_gemm_kernels.hpp"
#include "psf_hostpipe.hpp"
#include "psf_ntt_api.hpp"

// PSF_KEYGEN_TIMING=1: wall time of the phases of key generation on stderr (each mark drains the device first; off, a mark is one branch)
struct KeygenClock {
  bool on; const char* what; std::chrono::steady_clock::time_point t0, last;
  explicit KeygenClock(const char* w) : on(psf_exp_env("PSF_KEYGEN_TIMING") != nullptr), what(w) { if (on) { hipDeviceSynchronize(); t0 = last = std::chrono::steady_clock::now(); } }
  void mark(const char* phase) {
    if (!on) return;
    hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[keygen %s] %-28s %8.2f ms (at %8.2f)\n", what, phase, std::chrono::duration<double, std::milli>(now - last).count(), std::chrono::duration<double, std::milli>(now - t0).count());
    last = now;
  }
};

#define PSFP_FLAG_NO_PERTURB 1u   // internal: handle used as the Z_q / f_a engine of PSFGPV(Ring); no sqrt(Sigma_2) buffers
// PSFP_FLAG_STRUCTURED_SQRT (2u) is public: include/psf_mi355x.h

using namespace psf;

static inline unsigned grid_for(size_t total, unsigned block = 256, unsigned cap = 256 * 16) {
  size_t g = (total + block - 1) / block;
  if (g < 1) g = 1;
  return (unsigned)(g > cap ? cap : g);
}
// Rule of the handle (include/psf_mi355x.h, "Asynchronous calls"): an entry point that rewrites key material or reuses the handle's per-batch buffers first waits
// for the asynchronous samp_p calls in flight (psfp_wait) and returns their status if one failed -- they run on a non-blocking stream and would otherwise read a
// half-replaced key or share dP / dX / dV / the failure words with the new call.
#define PSFP_QUIESCE(h) do { const psf_status rw__ = psfp_wait(h); if (rw__ != PSF_OK) return rw__; } while (0)

struct TimingSlot { std::string name; Event e0, e1; };

// The work buffers of a batch: a struct of their own, so that ensure_batch releases them in one assignment before it allocates the larger ones
// (released in this order).  Bcap = 0: nothing usable, the next call starts over.
struct psfp_batch {
  DevArr<double> dDt, dX; DevArr<int32_t> dP;
  DevArr<int8_t> dP8;                         // three digit planes of P, [K_pad/16][ld][16] each
  DevArr<uint64_t> dV;
  DevArr<int8_t> dZlo, dZhi;
  DevArr<int8_t> dD8;                         // five digit planes of d_2 2^32 (structured mode), [ldr/16][ld][16] each
  DevArr<int32_t> dPf; DevArr<int8_t> dP8f;   // scratch of f_a (kept apart from the samp_p intermediates)
  DevArr<uint64_t> dPart;                     // per-split residues of the int8-MFMA Z_q product
  DevArr<uint64_t> dU; DevArr<int64_t> dE; DevArr<uint8_t> dOk;
  size_t Bcap = 0;
};

struct psfp_handle : psfp_batch {
  ~psfp_handle() { hp.quiesce(); }            // transport first: the prewarm thread and both call slots' workers are joined before any member is released
  psfp_params prm;
  size_t n, k, mb, w, m;
  uint64_t q, two64, two31;
  bool wide;            // q >= 2^31: two 31-bit limbs
  bool has_key = false;      // A, R and sqrt(Sigma_2) installed
  NormBound dom = {{0, 0, 0}};   // floor(s^2 m r^2): check_domain's bound in exact integers (domain_bound_exact), fixed by the parameters
  bool has_pub = false;      // A installed (f_a, check_domain, samp_d work; samp_p needs has_key)
  bool has_R = false;        // R installed (compute_sqrt_sigma_2 can complete the key; samp_p also needs has_pub)
  // key material
  DevArr<uint64_t> dA;         // n x m
  DevArr<int8_t> dR;           // mb x ldr
  size_t ldr = 0;
  DevArr<double> dLt;          // chunk stream of sqrt(Sigma_2) (structured mode: of L_1, the m_bar x m_bar block)
  size_t M_pad = 0, nbi = 0, nkb = 0;
  // structured sqrt(Sigma_2) (PSFP_FLAG_STRUCTURED_SQRT): x_top = L_1 d_1 - g R d_2, x_bot = h d_2
  bool structured = false;
  size_t mL = 0, nbiL = 0;     // order of the stored triangular factor (m, or m_bar) and its row blocks
  DevArr<int8_t> dR8;          // R tile-packed (k_pack_R8: 4 KiB tiles of 64 rows x 64 columns, contiguous) for k_recombine_mfma_big and k_rd2_mfma, mb_pad x ldr
  bool r8_valid = false;       // dR8 follows dR (ensure_R8)
  bool r8_pending = false;     // the pack has been enqueued on r8_stream and is not known to have completed: other streams wait for evR8
  Event evR8; hipStream_t r8_stream = nullptr;      // r8_stream: not owned (the stream of the call that packed)
  // compact copies of the key for calls with a handful of preimages, where reading A and R once IS the time of their stages (psf_stream_kernels.hpp):
  // R as two bits per entry (k_recombine_small2; only a {-1, 0, 1} trapdoor has one), A as 32-bit words (k_syndrome_small32; q <= 2^32)
  DevArr<uint32_t> dR2, dA32; DevArr<int> dR2bad; PinArr<int> hR2bad; Event evSmall;
  DevArr<uint32_t> dA32T;      // A transposed, [coordinate][row], 32-bit: the fused tail of k_trmm_stream_fused (q <= 2^32, n a multiple of 8)
  DevArr<uint64_t> dPartF;     // its partial residues, [task][row][preimage] (grown to the call's tasks)
  int small_state = 0;         // 0: stale (the key changed); 1: being built (evSmall); 2: usable; 3: usable, R is not ternary (A32 only)
  double g_const = 0, h_const = 0;
  // gadget tables
  DevArr<int32_t> dRng;
  DevArr<int32_t> dSk; DevArr<double> dGso, dNorm2; DevArr<SampleZParams> dSz;
  DevArr<uint64_t> dGvec;
  DevArr<int8_t> dA8; int NA = 0; size_t n_pad = 0, K_pad = 0;   // balanced base-256 digit planes of A
  ZqConsts zc;
  std::vector<int64_t> hSk; std::vector<double> hGso;
  SampleZParams szR, szSR;
  DevArr<uint32_t> dSzTab; uint32_t szF = 0;      // table screen of the rounding sampler (psf_rng.hpp, k_perturb_round_tab); szF = 0: none (wide words, or the table would not fit)
  // batch work buffers: psfp_batch
  size_t ld = 0, mb_pad = 0;
  DevArr<int> dFail;                          // four words: [0] sampler failure, [1] some |z| > 127, [2] some |p| >= 2^15 (run_samp_p)
  int zq_split_cap = 1;                       // K splits dPart has room for
  bool gadget_queue = true;   // task-queue gadget sampler (PSF_GADGET_QUEUE=0: lock-step kernel)
  HostPipe hp;                // host-pointer calls (psfp_samp_p / psfp_samp_p_async and their PSFGPV / ring forms): psf_hostpipe.hpp
  uint32_t normals_ncf = 0;   // layout of dDt after the last samp_p: 0 = chunk stream, else the compact stream with this many column fragments
  hipStream_t last_stream = nullptr;      // not owned (the caller's, or hp.compute)
  Stream side; Event evSide;      // psfp_trap_gen: A is computed on this low-priority stream beside the factorisation of Sigma_2
  // timing
  bool timing = false;
  std::vector<TimingSlot> slots;
  // psfp_samp_p_multi: this handle's window inside the last call (host clock, ms since the call began)
  double multi_launched_ms = -1.0, multi_done_ms = -1.0;
  int last_plan[PSFP_PLAN_FIELDS] = {0}; bool has_last_plan = false;      // the forms of the last samp_p pass that ran (psfp_get_last_plan)
};

// The compact copies follow the key without ever blocking a call: the first small call after a key change launches the two packers on its stream and goes on with
// the full-size matrices; a later call finds their event complete and switches over.
static void ensure_small_copies(psfp_handle* h, hipStream_t st) {
  if ((h->prm.flags & PSFP_FLAG_NO_PERTURB) || h->small_state >= 2) return;
  if (h->small_state == 1) {
    if (hipEventQuery(h->evSmall) == hipSuccess) h->small_state = *h->hR2bad ? 3 : 2;
    return;
  }
  const size_t ng = h->ldr / 16;
  if (!h->dR2) {
    if (h->dR2.alloc(h->mb * ng) != hipSuccess || h->dR2bad.alloc(1) != hipSuccess ||
        h->hR2bad.alloc(1) != hipSuccess || hipEventCreateWithFlags(h->evSmall.put(), hipEventDisableTiming) != hipSuccess) { h->small_state = 4; return; }
    if (h->q <= (1ull << 32) && h->dA32.alloc(h->n * h->m) != hipSuccess) { h->small_state = 4; return; }
    if (h->q <= (1ull << 32) && h->n % 8 == 0 && h->dA32T.alloc(h->n * h->m) != hipSuccess) (void)hipGetLastError();
  }
  hipMemsetAsync(h->dR2bad, 0, sizeof(int), st);
  hipLaunchKernelGGL(k_pack_R2, dim3(grid_for(h->mb * ng, 256, 256 * 32)), dim3(256), 0, st, h->dR, h->ldr, h->mb, h->dR2, h->dR2bad);
  if (h->dA32) hipLaunchKernelGGL(k_narrow_A32, dim3(grid_for(h->n * h->m, 256, 256 * 32)), dim3(256), 0, st, h->dA, h->n * h->m, h->dA32);
  if (h->dA32T) hipLaunchKernelGGL(k_transpose_A32, dim3((unsigned)((h->m + 31) / 32), (unsigned)((h->n + 31) / 32)), dim3(256), 0, st, h->dA, h->n, h->m, h->dA32T);
  hipMemcpyAsync(h->hR2bad, h->dR2bad, sizeof(int), hipMemcpyDeviceToHost, st);
  hipEventRecord(h->evSmall, st);
  h->small_state = 1;
}

// the tile-packed copy of R, rebuilt on `st` when R has changed since
// (as the compact copies above: the stream that packs is ordered behind the pack by itself; every OTHER stream that reads dR8 before the pack is known to have
// completed waits for its event -- back-to-back device-pointer calls on different non-blocking streams)
static void ensure_R8(psfp_handle* h, hipStream_t st) {
  if (!h->dR8) return;
  if (!h->r8_valid) {
    hipLaunchKernelGGL(k_pack_R8, dim3(grid_for(h->mb_pad * h->ldr, 256, 256 * 64)), dim3(256), 0, st, h->dR, h->ldr, h->mb, h->w, h->mb_pad, h->ldr, h->dR8);
    h->r8_valid = true;
    h->r8_pending = false;
    if (!h->evR8 && hipEventCreateWithFlags(h->evR8.put(), hipEventDisableTiming) != hipSuccess) { h->evR8.detach(); hipStreamSynchronize(st); return; }
    if (hipEventRecord(h->evR8, st) != hipSuccess) { hipStreamSynchronize(st); return; }
    h->r8_pending = true; h->r8_stream = st;
    return;
  }
  if (!h->r8_pending) return;
  if (hipEventQuery(h->evR8) == hipSuccess) { h->r8_pending = false; return; }
  if (st != h->r8_stream) hipStreamWaitEvent(st, h->evR8, 0);
}

static size_t gadget_lds_bytes(size_t k) { return k * k * 8 + k * 8 + k * sizeof(SampleZParams) + k * k * 4 + k * 256 * 4; }

// K splits of the Z_q product for `ncols` preimages: at most 256 K-steps each (int32 exactness of the digit-class sums), and enough workgroups to
// fill the chip -- a single call (one preimage) has 8 row tiles x 1 column tile, so its K range is cut as finely as 4 K-steps per split.  The
// residues are exact integers mod q: the number of splits changes no bit.
static int zq_plan(const psfp_handle* h, size_t ncols, int cap) {
  const int nks = (int)(h->K_pad / 64);
  int splits = (nks + 255) / 256;
  const size_t tiles = ((ncols + 63) / 64) * (h->n_pad / 64);
  const int min_ks = tiles * 8 >= 2048 ? 16 : 4;
  while (splits < cap && tiles * splits < 2048 && nks / (splits + 1) >= min_ks) ++splits;
  return splits;
}

// the K splits the Z_q product may take with buffers of leading dimension ld: the partial residues of every split live in dPart, [split][n_pad][ld]
static int zq_split_cap_for(const psfp_handle* h, size_t ld) {
  const int nks = (int)(h->K_pad / 64);
  const size_t per_split = h->n_pad * ld * sizeof(uint64_t);
  int cap = (int)(((size_t)256 << 20) / per_split);                 // small batches take up to 64 splits, within 256 MB
  if (cap > 64) cap = 64;
  const int legacy = zq_plan(h, ld, 8);
  if (cap < legacy) cap = legacy;
  return cap > nks ? nks : cap;
}

static psf_status ensure_batch(psfp_handle* h, size_t B) {
  if (B <= h->Bcap) return PSF_OK;
  HIP_TRY(hipDeviceSynchronize());
  static_cast<psfp_batch&>(*h) = psfp_batch{};      // every buffer of the smaller batch is released before the first of the larger is allocated
  const size_t ld = round_up(B, TR_BN);
  h->ld = ld;
  if (!(h->prm.flags & PSFP_FLAG_NO_PERTURB)) {
    HIP_TRY(h->dDt.alloc(ld / TR_BN * h->nkb * TR_CHUNK + TS_SLACK_DOUBLES));   // slack: k_trmm_stream reads past the diagonal
    HIP_TRY(h->dX.alloc(h->M_pad * ld));
    HIP_TRY(h->dP.alloc(h->M_pad * ld));
    HIP_TRY(h->dP8.alloc(3 * h->K_pad * ld));
    HIP_TRY(h->dV.alloc(h->n * ld));
    HIP_TRY(h->dZlo.alloc(h->ldr * ld + RS_SLACK_SLOTS * 128 * ld));      // [ldr/16][ld][16] (+ the slots k_recombine_wg's ring reads past the last K group)
    HIP_TRY(h->dZhi.alloc(h->ldr * ld + RS_SLACK_SLOTS * 128 * ld));
    HIP_TRY(hipMemset(h->dZlo, 0, h->ldr * ld));
    HIP_TRY(hipMemset(h->dZhi, 0, h->ldr * ld));
    HIP_TRY(hipMemset(h->dP, 0, h->M_pad * ld * sizeof(int32_t)));
    if (h->structured) {
      HIP_TRY(h->dD8.alloc(kFixPlanes * h->ldr * ld));
      HIP_TRY(hipMemset(h->dD8, 0, kFixPlanes * h->ldr * ld));
    }
  }
  HIP_TRY(h->dPf.alloc(h->M_pad * ld));
  HIP_TRY(h->dP8f.alloc(3 * h->K_pad * ld));
  h->zq_split_cap = zq_split_cap_for(h, ld);      // K splits of the Z_q product (zq_plan)
  HIP_TRY(h->dPart.alloc((size_t)h->zq_split_cap * h->n_pad * ld));
  HIP_TRY(h->dU.alloc(B * h->n));
  HIP_TRY(h->dE.alloc(B * h->m));
  HIP_TRY(h->dOk.alloc(B));
  // The clears above run on the null stream; the calls that follow may run on non-blocking streams (the host-pointer path's compute stream, a caller's stream), which do
  // not wait for it -- without this barrier a clear could land AFTER the first kernels had written the same buffer (found in round 5 by tools/host_vs_device_fuzz.py: one
  // whole-batch mismatch in 240 000 first calls, small keys whose product finishes within the clear of dP)
  HIP_TRY(hipDeviceSynchronize());
  h->Bcap = B;
  return PSF_OK;
}

struct ScopedTimer {
  psfp_handle* h; hipStream_t st; size_t idx; bool on;
  ScopedTimer(psfp_handle* h_, hipStream_t st_, const char* name) : h(h_), st(st_), on(h_->timing) {
    if (!on) return;
    TimingSlot s; s.name = name;
    hipEventCreate(s.e0.put()); hipEventCreate(s.e1.put());
    hipEventRecord(s.e0, st);
    h->slots.push_back(std::move(s));
    idx = h->slots.size() - 1;
  }
  ~ScopedTimer() { if (on) hipEventRecord(h->slots[idx].e1, st); }
};

#ifdef TRMM_CLOCK_PROBE
extern "C" void psf_debug_trmm_clk(unsigned long long* out, int reset) {
  if (out) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trmm_clk), sizeof(unsigned long long) * 4);
  if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; hipMemcpyToSymbol(HIP_SYMBOL(g_trmm_clk), z, sizeof(z)); }
}
#endif

extern "C" {

const char* psf_status_string(psf_status s) {
  switch (s) {
    case PSF_OK: return "ok";
    case PSF_ERR_PARAM: return "invalid parameter";
    case PSF_ERR_NOT_PD: return "Sigma_2 is not positive definite";
    case PSF_ERR_DOMAIN: return "sigma is not in the domain";
    case PSF_ERR_MODULUS: return "the modulus is too large, the value is potentially not representable";
    case PSF_ERR_NO_SOLUTION: return "the linear system has no solution";
    case PSF_ERR_NO_KEY: return "no key material installed";
    case PSF_ERR_HIP: return "HIP runtime error";
    case PSF_ERR_UNSUPPORTED: return "unsupported parameter combination";
    case PSF_ERR_SAMPLER: return "rejection sampler exceeded its attempt cap or an intermediate left its range";
    default: return "unknown status";
  }
}

psf_status psf_device_info(int device, char* name, size_t name_len, int* compute_units) {
  const psf_status ud = use_device(device);
  if (ud != PSF_OK) return ud;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (name && name_len) { std::strncpy(name, prop.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
  if (compute_units) *compute_units = prop.multiProcessorCount;
  return PSF_OK;
}

psf_status psf_gadget_params_default(uint64_t n, uint64_t q, psf_gadget_params* out) { return gadget_params_default(n, q, out); }
psf_status psf_gadget_params_ring_default(uint64_t n, uint64_t q, psf_gadget_params* out) { return gadget_params_ring_default(n, q, out); }

psf_status psf_gen_gadget_vec(uint64_t k, uint64_t base, int64_t* out) {
  if (k < 1 || !out) return PSF_ERR_PARAM;
  const auto g = gen_gadget_vec(k, base);
  std::memcpy(out, g.data(), k * sizeof(int64_t));
  return PSF_OK;
}
psf_status psf_gen_gadget_mat(uint64_t n, uint64_t k, uint64_t base, int64_t* out) {
  if (n < 1 || k < 1 || !out) return PSF_ERR_PARAM;
  const auto G = gen_gadget_mat(n, k, base);
  std::memcpy(out, G.data(), G.size() * sizeof(int64_t));
  return PSF_OK;
}
psf_status psf_short_basis_gadget(const psf_gadget_params* gp, int64_t* out) {
  if (!gp || !out || gp->n < 1 || gp->k < 1) return PSF_ERR_PARAM;
  const auto S = short_basis_gadget(*gp);
  std::memcpy(out, S.data(), S.size() * sizeof(int64_t));
  return PSF_OK;
}
psf_status psf_gen_short_basis_for_trapdoor(const psf_gadget_params* gp, const uint64_t* tag, const uint64_t* A, const int8_t* R, int64_t* out) {
  if (!gp || !A || !R || !out) return PSF_ERR_PARAM;
  std::vector<int64_t> S;
  const psf_status rc = gen_short_basis_for_trapdoor(*gp, tag, A, R, S);
  if (rc != PSF_OK) return rc;
  std::memcpy(out, S.data(), S.size() * sizeof(int64_t));
  return PSF_OK;
}
psf_status psf_rot_minus_matrix(const int64_t* mat, size_t rows, size_t cols, int64_t* out) {
  if (!mat || !out || rows < 1 || cols < 1) return PSF_ERR_PARAM;
  rot_minus_matrix(mat, rows, cols, out);
  return PSF_OK;
}

psf_status psf_find_solution_gadget_mat(int device, const uint64_t* value, size_t rows, size_t cols, uint64_t q, uint64_t k,
                                        uint64_t base, int64_t* out) {
  if (!value || !out || q <= 1 || k < 1 || base < 2) return PSF_ERR_PARAM;
  if (gadget_too_short(base, k, q)) return PSF_ERR_MODULUS;   // gadget_classical.rs:170-172
  if (rows * cols == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  DevBuf dv, dout;
  HIP_TRY(dv.alloc(rows * cols * sizeof(uint64_t)));
  HIP_TRY(dout.alloc(k * rows * cols * sizeof(int64_t)));
  HIP_TRY(dv.upload(value, rows * cols * sizeof(uint64_t)));
  hipLaunchKernelGGL(k_digits, dim3(grid_for(rows * cols)), dim3(256), 0, 0, dv.as<uint64_t>(), rows, cols, q, (uint32_t)k, base, dout.as<int64_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(dout.download(out, k * rows * cols * sizeof(int64_t)));
  return PSF_OK;
}

// ------------------------------------------------------------------------------------------------------------
static psf_status psfp_init(psfp_handle* h, const psfp_params* prm);

// The screen table of one s (psf_rng.hpp "table screen"): for every candidate index and every bin of delta = ceil(c) - c the 16-bit bounds between which an
// attempt has to be settled exactly.  rho is monotone on either side of a = 0 and a = (idx - ceil(6 s) + delta) / s changes sign only at integers, so the
// extremes over a bin are at its ends; the bins overlap by 1e-9 (the kernel's delta carries one rounding) and the floors get one unit of slack on either side.
static bool build_sz_table(const SampleZParams& sp, std::vector<uint32_t>& T, uint32_t* F_out) {
  if (sp.sh != 16 || sp.n_int < 2) return false;
  uint32_t F = 64;
  while (F >= 8 && (size_t)sp.n_int * F * sizeof(uint32_t) > 40 * 1024) F >>= 1;
  if (F < 8) return false;
  T.assign((size_t)sp.n_int * F, 0);
  auto rs_at = [&](double idx, double delta) {
    const double a = (idx - (double)sp.c6 + delta) * sp.inv_s;
    return det_exp(-3.14159265358979323846 * (a * a)) * 65536.0;
  };
  for (uint32_t idx = 0; idx < sp.n_int; ++idx)
    for (uint32_t b = 0; b < F; ++b) {
      double d0 = (double)b / F - 1e-9, d1 = (double)(b + 1) / F + 1e-9;
      if (d0 < 0.0) d0 = 0.0;
      if (d1 > 1.0) d1 = 1.0;
      const double r0 = rs_at((double)idx, d0), r1 = rs_at((double)idx, d1);
      double lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;
      if ((double)idx - (double)sp.c6 + d0 <= 0.0 && (double)idx - (double)sp.c6 + d1 >= 0.0) hi = 65536.0;      // a = 0 inside the bin
      long long A = (long long)std::floor(lo) - 1, R = (long long)std::floor(hi) + 1;
      if (A < 0) A = 0;
      if (R > 65535) R = 65535;
      T[(size_t)idx * F + b] = ((uint32_t)R << 16) | (uint32_t)A;
    }
  *F_out = F;
  return true;
}

psf_status psfp_create(const psfp_params* prm, psfp_handle** out) {
  if (!prm || !out) return PSF_ERR_PARAM;
  const psf_gadget_params& gp = prm->gp;
  if (gp.n < 1 || gp.k < 1 || gp.base < 2 || gp.q <= 1 || gp.q >= (1ull << 62) || gp.m_bar < 1) return PSF_ERR_PARAM;
  if (!(prm->r > 0.0) || !(prm->s > 0.0)) return PSF_ERR_PARAM;
  if (gp.k > 64) return PSF_ERR_UNSUPPORTED;
  {  // every in-domain coordinate obeys |e_i| <= ||e|| <= s r sqrt(m) (mp_perturbation.rs:396-402); the int8 digit planes of the
     // Z_q products (f_a, syndrome) cover |.| < 2^23, so larger domains are refused here instead of being truncated later
    const double m_all = (double)gp.m_bar + (double)gp.n * (double)gp.k;
    if (!(prm->s * prm->r * std::sqrt(m_all) < 8388607.0)) return PSF_ERR_UNSUPPORTED;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || prm->device < 0 || prm->device >= count) {
    std::fprintf(stderr, "[psf_mi355x] no usable HIP device %d (found %d); this library has no CPU fallback\n", prm->device, count);
    return PSF_ERR_HIP;
  }
  HIP_TRY(hipSetDevice(prm->device));
  psfp_handle* h = new psfp_handle();
  const psf_status rc = psfp_init(h, prm);
  if (rc != PSF_OK) { psfp_destroy(h); return rc; }      // whatever was allocated before the failure is released
  *out = h;
  return PSF_OK;
}

static psf_status psfp_init(psfp_handle* h, const psfp_params* prm) {
  const psf_gadget_params& gp = prm->gp;
  h->prm = *prm;
  h->n = gp.n; h->k = gp.k; h->mb = gp.m_bar; h->w = gp.n * gp.k; h->m = h->mb + h->w; h->q = gp.q;
  h->dom = domain_bound_exact(prm->s, prm->r, h->m);
  h->two64 = (uint64_t)((((u128)1) << 64) % gp.q);
  h->two31 = (uint64_t)((1ull << 31) % gp.q);
  h->wide = gp.q >= (1ull << 31);
  h->M_pad = round_up(h->m, TR_BM);
  h->nbi = h->M_pad / TR_BM;
  h->nkb = h->M_pad / TR_BK;
  h->structured = (prm->flags & PSFP_FLAG_STRUCTURED_SQRT) != 0 && !(prm->flags & PSFP_FLAG_NO_PERTURB);
  h->mL = h->structured ? h->mb : h->m;
  h->nbiL = round_up(h->mL, TR_BM) / TR_BM;
  h->ldr = round_up(h->w, 64);          // K of the int8 MFMA product, zero padded
  h->mb_pad = round_up(h->mb, 256);        // rows of R as allocated (zero below m_bar): the 256-row tiles of k_recombine_mfma_big read them all
  h->n_pad = round_up(h->n, 64);
  h->K_pad = round_up(h->m, 64);
  {  // number of balanced base-256 digits so that the top digit of any a < q fits an int8
    uint64_t bound = gp.q - 1;
    h->NA = 1;
    while (bound > 127) { bound = (bound + 128) >> 8; ++h->NA; }
    h->zc.q = gp.q; h->zc.two64 = h->two64;
    uint64_t pw = 1 % gp.q;
    h->zc.inv_q = 1.0 / (double)gp.q;
    for (int c = 0; c < 12; ++c) { h->zc.pw[c] = pw; h->zc.pwd[c] = (double)pw; pw = mulmod_u64(pw, 256 % gp.q, gp.q); }
  }
  HIP_TRY(h->dA8.alloc((size_t)h->NA * h->n_pad * h->K_pad));
  h->szR = make_sample_z_params(prm->r);
  {
    std::vector<uint32_t> T;
    uint32_t F = 0;
    if (!(prm->flags & PSFP_FLAG_NO_PERTURB) && build_sz_table(h->szR, T, &F)) {
      HIP_TRY(h->dSzTab.alloc(T.size()));
      HIP_TRY(hipMemcpy(h->dSzTab, T.data(), T.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      h->szF = F;
    }
  }
  h->szSR = make_sample_z_params(prm->s * prm->r);                    // mp_perturbation.rs:266
  HIP_TRY(h->dA.alloc(h->n * h->m));
  HIP_TRY(h->dR.alloc(h->mb_pad * h->ldr + 4096));      // (+ what k_recombine_wg's ring reads past the last row)
  HIP_TRY(hipMemset(h->dR, 0, h->mb_pad * h->ldr));
  if (!(prm->flags & PSFP_FLAG_NO_PERTURB)) HIP_TRY(h->dLt.alloc(tr_total_chunks(h->nbiL) * TR_CHUNK + TS_SLACK_DOUBLES));
  if (!(prm->flags & PSFP_FLAG_NO_PERTURB)) HIP_TRY(h->dR8.alloc(h->mb_pad * h->ldr));      // tile-packed copy of R: k_recombine_mfma_big, k_rd2_mfma
  HIP_TRY(h->dFail.alloc(4));
  HIP_TRY(hipMemset(h->dFail, 0, 4 * sizeof(int)));
  {
    int lo_prio = 0, hi_prio = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
    HIP_TRY(hipStreamCreateWithPriority(h->side.put(), hipStreamNonBlocking, lo_prio));
  }
  HIP_TRY(hipEventCreateWithFlags(h->evSide.put(), hipEventDisableTiming));
  // gadget part of the trapdoor: (S, S~) of mp_perturbation.rs:233-234, block form
  h->hSk = short_basis_gadget_block(gp);
  std::vector<double> norm2;
  gso_columns(h->hSk, h->k, h->hGso, norm2);
  const double sG = prm->r * std::sqrt((double)(gp.base * gp.base + 1));   // mp_perturbation.rs:180
  std::vector<SampleZParams> sz(h->k);
  for (size_t i = 0; i < h->k; ++i) sz[i] = make_sample_z_params(sG / std::sqrt(norm2[i]));
  std::vector<int32_t> sk32(h->hSk.begin(), h->hSk.end());
  std::vector<int32_t> rng(4 * h->k);
  for (size_t col = 0; col < h->k; ++col) {        // non-zero row ranges of b~_col and b_col (zeros are exact: they can be skipped)
    int glo = (int)h->k, ghi = -1, slo = (int)h->k, shi = -1;
    for (size_t r = 0; r < h->k; ++r) {
      if (h->hGso[r * h->k + col] != 0.0) { if ((int)r < glo) glo = (int)r; ghi = (int)r; }
      if (h->hSk[r * h->k + col] != 0) { if ((int)r < slo) slo = (int)r; shi = (int)r; }
    }
    rng[col] = glo; rng[h->k + col] = ghi; rng[2 * h->k + col] = slo; rng[3 * h->k + col] = shi;
  }
  HIP_TRY(h->dRng.alloc(rng.size()));
  HIP_TRY(hipMemcpy(h->dRng, rng.data(), rng.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  const auto gvec = gen_gadget_vec_mod(h->k, gp.base, gp.q);
  HIP_TRY(h->dSk.alloc(sk32.size()));
  HIP_TRY(h->dGso.alloc(h->hGso.size()));
  HIP_TRY(h->dNorm2.alloc(h->k));
  HIP_TRY(h->dSz.alloc(h->k));
  HIP_TRY(h->dGvec.alloc(h->k));
  HIP_TRY(hipMemcpy(h->dSk, sk32.data(), sk32.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->dGso, h->hGso.data(), h->hGso.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->dNorm2, norm2.data(), h->k * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->dSz, sz.data(), h->k * sizeof(SampleZParams), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->dGvec, gvec.data(), h->k * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_mfma), hipFuncAttributeMaxDynamicSharedMemorySize, RC_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_mfma_big), hipFuncAttributeMaxDynamicSharedMemorySize, RCB_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_small<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_small<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_small<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_small2<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_small2<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_small2<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rd2_mfma), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * (1 + kFixPlanes) * 4096));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gadget), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gadget_lds_bytes(h->k)));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_wg<1, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RW_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_wg<2, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RW_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_wg<3, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RW_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_recombine_wg<4, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RW_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_trmm_stream_wg32<TSW_H, TSW_NBUF, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TSW32_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_trmm_stream_wg32<TSW_H, TSW_NBUF, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TSW32_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_trmm_stream_wg<TSW64_H, TSW64_NBUF, 0, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TSW_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_trmm_stream_wg<TSW64_H, TSW64_NBUF, 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TSW_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gadget_queue<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gadget_queue_lds_bytes(h->k)));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gadget_queue<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gadget_queue_lds_bytes(h->k)));
  if (const char* env = psf_exp_env("PSF_GADGET_QUEUE")) h->gadget_queue = std::atoi(env) != 0;
  for (int64_t v : h->hSk) if (v > 32767 || v < -32768) h->gadget_queue = false;      // the queue kernel keeps S_k in int16
  return PSF_OK;
}

// A key whose batches will cross PCIe (m >= 8192: a preimage is >= 64 KiB) gets the batch-independent part of the host-pointer machinery -- streams, the DMA path,
// one slot's pinned rings -- when the key is installed, next to a factorisation that takes a quarter of a second, instead of inside the first samp_p call
// (PSF_HOST_PREWARM=0: on first use, as for small keys).
static void hp_prewarm(psfp_handle* h) {
  if (h->m < 8192) return;
  if (const char* env = psf_exp_env("PSF_HOST_PREWARM")) if (std::atoi(env) == 0) return;
  if (h->hp.hp_warm.joinable()) h->hp.hp_warm.join();
  try {
    h->hp.hp_warm = std::thread([h]() { if (hipSetDevice(h->prm.device) == hipSuccess) (void)hp_ensure(h->hp, h->prm.device, 0, 0, 0, true); });      // beside the factorisation, not behind it
  } catch (...) { }                                         // no thread: on first use then
}
void psfp_destroy(psfp_handle* h) {
  if (!h) return;
  hipSetDevice(h->prm.device);
  delete h;
}

size_t psfp_m(const psfp_handle* h) { return h ? h->m : 0; }

// Sigma_2 assembly (dense lower) + Cholesky + repack.  mp_perturbation.rs:111-139.
// Structured mode factors Sigma_2 = c [[alpha I - kappa R R^t, -kappa R], [-kappa R^t, beta I]]  (c = r^2 / 2 pi, kappa = b^2 + 1, alpha = s^2 - 1,
// beta = alpha - kappa) as B B^t with B = [[L_1 / sqrt c, -kappa R / sqrt beta], [0, sqrt beta I]] sqrt c, where L_1 is the Cholesky factor of
// c (alpha I - kappa (alpha / beta) R R^t): only that m_bar x m_bar block is assembled, factored and stored.
// Cholesky of Sigma_2 directly on the key's chunk stream (psf_chol_kernels.hpp, "Cholesky directly on the key's chunk stream"): no dense m x m matrix.
// factor + invert one 128 x 128 diagonal block (k_chol_diag_inv)
static void launch_chol_diag(hipStream_t st, double* P, size_t ld, size_t off, int nb, double* dLi, int* dinfo, size_t report_base) {
  hipLaunchKernelGGL(k_chol_diag_inv, dim3(1), dim3(256), CH_DIAG_LDS, st, P, ld, off, nb, dLi, dinfo, report_base);
}
static bool prepare_chol_diag() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_chol_diag_inv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CH_DIAG_LDS) == hipSuccess;
}

// dS_dense: nullptr, or Sigma_2 already assembled as a dense m x m matrix (lower triangle; the hybrid of build_sqrt_sigma2): the panels are then copied out of it
// instead of being assembled one by one -- R R^t on the int8 matrix cores takes 5.5 ms for the whole of C3's Sigma_2 at once and 76 ms in 121 panel-sized pieces.
static psf_status build_sqrt_sigma2_stream(psfp_handle* h, double nf_r2, double s2, double b2p1, const double* d_sig, const double* dS_dense = nullptr) {
  const size_t m = h->mL;
  const int nbi = (int)h->nbiL;
  const int nP = (nbi + 1) / 2;                                       // panels of two column blocks (256 columns)
  const size_t PW = 2 * TR_BM;                                        // leading dimension of a panel buffer
  const size_t prow = (size_t)nbi * TR_BM;                            // its rows (panel 0 needs them all)
  // K splits of the update.  One workgroup occupies a CU (356 registers per lane), so a launch runs in rounds of 256 workgroups, each as long as one split
  // plus its epilogue (the 128 x 256 partial tile goes to the workspace and is read back by the reduce: about 1.5 units' worth of time, a unit being two
  // chunks = 32 columns of L).  The split count minimises rounds x (units per split + 1.5) over at most 4096 workgroups: without it the middle panels of a large key, whose 257..511 row
  // blocks are just over one round, leave up to half of the chip idle.
  auto splits_for = [](int wgs, int units) {
    if (wgs <= 0 || units <= 1) return 1;
    int best = 1; double best_cost = 1e300;
    for (int sp = 1; sp <= units && sp <= 64; ++sp) {
      if (sp > 1 && (size_t)wgs * sp > 4096) break;                    // workspace: 256 KB per workgroup, 1 GB at most
      const double cost = (double)(((size_t)wgs * sp + 255) / 256) * ((double)((units + sp - 1) / sp) + 1.5);
      if (cost < best_cost * 0.999) { best_cost = cost; best = sp; }
    }
    return best;
  };
  size_t ws_doubles = 0;
  for (int J = 1; J < nP; ++J) {
    const int nrb = nbi - 2 * J, head = nrb < 2 ? nrb : 2;
    const size_t a = (size_t)splits_for(head, 8 * J) * head * TR_BM * PW;
    const size_t b = nrb > 2 ? (size_t)splits_for(nrb - 2, 8 * J) * (size_t)(nrb - 2) * TR_BM * PW : 0;
    if (a > ws_doubles) ws_doubles = a;
    if (b > ws_doubles) ws_doubles = b;
  }
  DevArr<double> dPn[2], dLi, dWs; DevArr<int> dinfo;                 // (released on every return, in reverse: streams, events, buffers)
  Event evSig[2], evPack[2], evHead, evDiag;
  Stream sm, ss, sd;                                                  // factorisation / Sigma_2 panels (one panel ahead) / the diagonal blocks' chain (look-ahead)
  GemmWorkspace w, w2;                                                // the in-panel products have K = 128: never cut
  bool lookahead = true;
  if (const char* e = psf_exp_env("PSF_CHOL_LOOKAHEAD")) lookahead = std::atoi(e) != 0;
  bool ok = gemm_prepare() == hipSuccess && prepare_chol_diag() &&
            dPn[0].alloc(prow * PW) == hipSuccess && dPn[1].alloc(prow * PW) == hipSuccess &&
            dLi.alloc(2 * CH_NB * CH_NB) == hipSuccess && (!ws_doubles || dWs.alloc(ws_doubles) == hipSuccess) &&
            dinfo.alloc(1) == hipSuccess && hipMemset(dinfo, 0, sizeof(int)) == hipSuccess &&
            hipMemset(dPn[0], 0, prow * PW * sizeof(double)) == hipSuccess && hipMemset(dPn[1], 0, prow * PW * sizeof(double)) == hipSuccess;
  for (Stream* st : {&sm, &ss, &sd}) ok = ok && hipStreamCreateWithFlags(st->put(), hipStreamNonBlocking) == hipSuccess;
  for (Event* ev : {&evSig[0], &evSig[1], &evPack[0], &evPack[1], &evHead, &evDiag}) ok = ok && hipEventCreateWithFlags(ev->put(), hipEventDisableTiming) == hipSuccess;
  if (!ok) return PSF_ERR_HIP;
  if (hipStreamSynchronize(nullptr) != hipSuccess) return PSF_ERR_HIP;      // R, the dense Sigma_2 (and k_pack_R8) were produced on the default stream (not a device-wide wait: psfp_trap_gen computes A on a side stream meanwhile)
  // Sigma_2 restricted to panel J (rows off.., columns off..off+255), dense with leading dimension 256; it does not depend on the factorisation, so it
  // is assembled one panel ahead on its own stream into the other of two panel buffers
  auto sigma_panel = [&](int J) {
    const size_t off = (size_t)J * PW;
    const size_t cols = m - off < PW ? m - off : PW;
    const dim3 sg((unsigned)((cols + 63) / 64), (unsigned)((m - off + 63) / 64));
    if (dS_dense) {
      hipLaunchKernelGGL(k_chol_copy_panel, dim3(grid_for((m - off) * cols, 256, 4096)), dim3(256), 0, ss, dS_dense, m, m, off, cols, dPn[J & 1], PW);
    } else {
      hipLaunchKernelGGL(k_sigma2_rrt, sg, dim3(256), 3 * 2 * 4096, ss, h->dR, h->ldr, h->mb, m, nf_r2, s2, b2p1, d_sig, dPn[J & 1], PW, off, off);
      hipLaunchKernelGGL(k_sigma2, sg, dim3(256), 0, ss, h->dR, h->ldr, h->mb, h->w, m, nf_r2, s2, b2p1, d_sig, dPn[J & 1], PW, off, off, 1);
    }
    hipEventRecord(evSig[J & 1], ss);
  };
  sigma_panel(0);
  for (int J = 0; J < nP; ++J) {
    const size_t off = (size_t)J * PW;
    const int ncb = 2 * J + 1 < nbi ? 2 : 1;                          // column blocks of this panel
    const int nrb = nbi - 2 * J;                                      // its row blocks
    const size_t nb0 = m - off < (size_t)TR_BM ? m - off : (size_t)TR_BM;
    const size_t below0 = m - off - nb0;                              // rows under the first diagonal block
    const size_t nb1 = ncb == 2 ? (below0 < (size_t)TR_BM ? below0 : (size_t)TR_BM) : 0;
    const size_t below1 = ncb == 2 ? below0 - nb1 : 0;                // rows under the second diagonal block
    double* P = dPn[J & 1];
    if (J + 1 < nP) {
      if (J >= 1) hipStreamWaitEvent(ss, evPack[(J + 1) & 1], 0);     // the buffer's previous panel (J - 1) has been packed
      sigma_panel(J + 1);
    }
    hipStreamWaitEvent(sm, evSig[J & 1], 0);
    auto update = [&](int rb0, int count) {                            // P -= L[rows of the panel, columns < off] L[panel's row blocks, columns < off]^t
      const int sp = splits_for(count, 8 * J);
      const size_t stride = (size_t)count * TR_BM * PW;               // doubles per split in the workspace
      const size_t first = (size_t)rb0 * TR_BM * PW;
      hipLaunchKernelGGL(k_chol_update_big, dim3((unsigned)count, (unsigned)sp), dim3(256), 0, sm, h->dLt, J, nbi, rb0, 8 * J, dWs - first, stride);
      hipLaunchKernelGGL(k_chol_panel_reduce, dim3(grid_for(stride, 256, 2048)), dim3(256), 0, sm, P + first, dWs, stride, sp, (size_t)0, stride);
    };
    if (J > 0) {
      const int head = nrb < 2 ? nrb : 2;
      update(0, head);                                                // the two row blocks that hold the diagonal blocks (cut finely along K), then the rest
      if (lookahead) hipEventRecord(evHead, sm);
      else if (nrb > 2) update(2, nrb - 2);
    } else if (lookahead) hipEventRecord(evHead, sm);
    double* const Li0 = dLi;
    double* const Li1 = lookahead ? dLi + (size_t)CH_NB * CH_NB : dLi;
    if (lookahead) {
      // Round 6: the two diagonal blocks of the panel need only the HEAD of the update.  Their chain -- factor + invert block (0,0), L10 = P10 L00^-t, P11 -= L10 L10^t,
      // factor + invert block (1,1): two single-workgroup kernels and two 128^3 products, 0.6 ms of pure latency per panel -- runs on a second stream while the rest
      // of the update (the rows below, ~1 ms of matrix work per panel in the middle of the factorisation) occupies the chip; the panel's triangular solves wait for both.
      hipStreamWaitEvent(sd, evHead, 0);
      launch_chol_diag(sd, P, PW, (size_t)0, (int)nb0, Li0, dinfo, off);
      if (ncb == 2) {
        launch_gemm<true>(sd, GemmArgs{P + TR_BM * PW, PW, Li0, (size_t)CH_NB, P + TR_BM * PW, PW, nb1, nb0, nb0, 1.0, 0.0, nullptr, nullptr, 0}, w2);
        launch_gemm<true>(sd, GemmArgs{P + TR_BM * PW, PW, P + TR_BM * PW, PW, P + TR_BM * PW + TR_BM, PW, nb1, nb1, (size_t)TR_BM, -1.0, 1.0, nullptr, nullptr, 0}, w2);
        launch_chol_diag(sd, P, PW, (size_t)TR_BM, (int)nb1, Li1, dinfo, off + TR_BM);
      }
      hipEventRecord(evDiag, sd);
      if (J > 0 && nrb > 2) update(2, nrb - 2);
      hipStreamWaitEvent(sm, evDiag, 0);
      if (below1) {                                                   // the rows under both diagonal blocks: solve, take column block 0 out of column block 1, solve
        double* const Pr = P + 2 * TR_BM * PW;
        launch_gemm<true>(sm, GemmArgs{Pr, PW, Li0, (size_t)CH_NB, Pr, PW, below1, nb0, nb0, 1.0, 0.0, nullptr, nullptr, 0}, w);
        launch_gemm<true>(sm, GemmArgs{Pr, PW, P + TR_BM * PW, PW, Pr + TR_BM, PW, below1, nb1, (size_t)TR_BM, -1.0, 1.0, nullptr, nullptr, 0}, w);
        launch_gemm<true>(sm, GemmArgs{Pr + TR_BM, PW, Li1, (size_t)CH_NB, Pr + TR_BM, PW, below1, nb1, nb1, 1.0, 0.0, nullptr, nullptr, 0}, w);
      }
    } else {
    // inside the panel: factor + invert the first diagonal block, solve its rows below, take its contribution out of the second column block, the same again
    launch_chol_diag(sm, P, PW, (size_t)0, (int)nb0, dLi, dinfo, off);
    if (below0)
      launch_gemm<true>(sm, GemmArgs{P + TR_BM * PW, PW, dLi, (size_t)CH_NB, P + TR_BM * PW, PW, below0, nb0, nb0, 1.0, 0.0, nullptr, nullptr, 0}, w);
    if (ncb == 2) {
      launch_gemm<true>(sm, GemmArgs{P + TR_BM * PW, PW, P + TR_BM * PW, PW, P + TR_BM * PW + TR_BM, PW, below0, nb1, (size_t)TR_BM, -1.0, 1.0, nullptr, nullptr, 0}, w);
      launch_chol_diag(sm, P, PW, (size_t)TR_BM, (int)nb1, dLi, dinfo, off + TR_BM);
      if (below1)
        launch_gemm<true>(sm, GemmArgs{P + 2 * TR_BM * PW + TR_BM, PW, dLi, (size_t)CH_NB, P + 2 * TR_BM * PW + TR_BM, PW, below1, nb1, nb1, 1.0, 0.0, nullptr, nullptr, 0}, w);
    }
    }
    hipLaunchKernelGGL(k_chol_pack_panel, dim3(grid_for((size_t)nrb * ncb * 8 * TR_CHUNK, 256, 4096)), dim3(256), 0, sm, P, J, ncb, nbi, m, h->dLt);
    hipEventRecord(evPack[J & 1], sm);
  }
  hipError_t ce = hipStreamSynchronize(sm);
  if (ce == hipSuccess) ce = hipStreamSynchronize(ss);
  if (ce == hipSuccess) ce = hipStreamSynchronize(sd);
  if (ce == hipSuccess) ce = hipGetLastError();
  int info = -1;
  if (ce == hipSuccess) ce = hipMemcpy(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost);
  if (ce != hipSuccess) return PSF_ERR_HIP;
  return info != 0 ? PSF_ERR_NOT_PD : PSF_OK;                         // mp_perturbation.rs:109-110
}

static psf_status build_sqrt_sigma2(psfp_handle* h, double s_cov, const double* d_sigma_packed = nullptr) {
  const double TWO_PI = 6.283185307179586476925;
  const double nf_r2 = (1.0 / TWO_PI) * (h->prm.r * h->prm.r);
  const double s2 = s_cov * s_cov;
  double b2p1 = (double)(h->prm.gp.base * h->prm.gp.base + 1);
  const size_t m = h->mL;
  if (h->structured) {
    const double kappa = b2p1, alpha = s2 - 1.0, beta = alpha - kappa;
    if (!(beta > 0.0)) return PSF_ERR_NOT_PD;
    b2p1 = kappa * (alpha / beta);                                   // the R R^t block of the Schur-complemented top-left corner
    h->g_const = (std::sqrt(nf_r2) * kappa) / std::sqrt(beta);
    h->h_const = std::sqrt(nf_r2 * beta);
    ensure_R8(h, nullptr);
  }
  // Cholesky on the key's chunk stream (build_sqrt_sigma2_stream).  Above 16 GB (m >= 46 341) Sigma_2 is assembled there panel by panel, no dense matrix (C5: 10.1 s
  // against 21.1 s for a dense left-looking form, and 121 GB less memory); below, the hybrid (round 6): Sigma_2 dense AT ONCE, the factorisation on the chunk stream
  // (k_chol_update_big: 64 TFLOP/s against the 44 of the LDS-staged GEMM of the dense form), panels copied out of the dense matrix.  PSF_CHOL=stream (experiments
  // build): the stream form at every size.
  const char* ce = psf_exp_env("PSF_CHOL");
  const bool stream = ce ? !std::strcmp(ce, "stream") : m * m * sizeof(double) > (16ull << 30);
  if (stream) return build_sqrt_sigma2_stream(h, nf_r2, s2, b2p1, d_sigma_packed);
  DevBuf dense;
  HIP_TRY(dense.alloc(m * m * sizeof(double)));
  HIP_TRY(dense.zero(m * m * sizeof(double)));
  double* dS = dense.as<double>();
  const unsigned tiles = (unsigned)((m + 63) / 64);
  // the R R^t block on the int8 matrix cores, everything else (the rows from m_bar on) in k_sigma2
  hipLaunchKernelGGL(k_sigma2_rrt, dim3(tiles, tiles), dim3(256), 3 * 2 * 4096, 0, h->dR, h->ldr, h->mb, m, nf_r2, s2, b2p1, d_sigma_packed, dS, m, (size_t)0, (size_t)0);
  hipLaunchKernelGGL(k_sigma2, dim3(tiles, tiles), dim3(256), 0, 0, h->dR, h->ldr, h->mb, h->w, m, nf_r2, s2, b2p1, d_sigma_packed, dS, m, (size_t)0, (size_t)0, 1);
  HIP_TRY(hipGetLastError());
  return build_sqrt_sigma2_stream(h, nf_r2, s2, b2p1, d_sigma_packed, dS);
}

// A[:, m_bar:] = G - A_bar R  (gadget_classical.rs:66): the one product still on the limb kernel (setup path, R in int8)
static void launch_zq_trapdoor(psfp_handle* h, const uint64_t* d_tag = nullptr, hipStream_t st = nullptr) {
  dim3 grid((unsigned)((h->w + 63) / 64), (unsigned)((h->n + 63) / 64));
  if (h->wide)
    hipLaunchKernelGGL((k_zq_matmul<int8_t, true>), grid, dim3(256), 0, st, (int)ZQ_TRAPDOOR, h->dA, h->m, (size_t)0, h->n, h->mb, h->dR, h->ldr, h->w,
                       h->q, h->two64, h->two31, (const uint64_t*)nullptr, h->dA, h->m, h->mb, h->dGvec, (uint64_t)h->k, d_tag);
  else
    hipLaunchKernelGGL((k_zq_matmul<int8_t, false>), grid, dim3(256), 0, st, (int)ZQ_TRAPDOOR, h->dA, h->m, (size_t)0, h->n, h->mb, h->dR, h->ldr, h->w,
                       h->q, h->two64, h->two31, (const uint64_t*)nullptr, h->dA, h->m, h->mb, h->dGvec, (uint64_t)h->k, d_tag);
}

static void split_A(psfp_handle* h, hipStream_t st = nullptr) {
  hipLaunchKernelGGL(k_split_A, dim3(grid_for(h->n_pad * h->K_pad)), dim3(256), 0, st, h->dA, h->m, h->n, h->m, h->n_pad, h->K_pad, h->NA, h->dA8);
}

// A_bar <- U(Z_q^{n x m_bar}), R <- PlusMinusOneZero, A = [A_bar | G - A_bar R] (gen_trapdoor, gadget_classical.rs:56-68, tag = I)
// side: nullptr, or a non-blocking stream on which A = [A_bar | G - A_bar R] and its digit planes are computed while the caller goes on with R alone (the
// factorisation of Sigma_2 needs R, not A: psfp_trap_gen); the caller synchronises `side` before anything reads A
static psf_status gen_A_R(psfp_handle* h, uint64_t seed, hipStream_t side = nullptr) {
  if (gadget_too_short(h->prm.gp.base, h->k, h->q)) return PSF_ERR_MODULUS;
  // mp_perturbation.rs:222 / gpv.rs:84 ; gadget_classical.rs:62-64
  hipLaunchKernelGGL(k_sample_abar, dim3(grid_for(h->n * h->mb)), dim3(256), 0, 0, seed, h->n, h->mb, h->m, h->q, h->dA);
  h->r8_valid = false; h->small_state = 0;
  hipLaunchKernelGGL(k_sample_R, dim3(grid_for(h->mb * h->ldr)), dim3(256), 0, 0, seed, h->mb, h->w, h->ldr, h->dR);
  if (side) {
    HIP_TRY(hipEventRecord(h->evSide, nullptr));
    HIP_TRY(hipStreamWaitEvent(side, h->evSide, 0));
  }
  // gadget_classical.rs:66
  launch_zq_trapdoor(h, nullptr, side);
  HIP_TRY(hipGetLastError());
  split_A(h, side);
  return PSF_OK;
}

// gen_trapdoor (gadget_classical.rs:56-68) as a free function: caller-supplied A_bar and tag H; R <- PlusMinusOneZero from `seed` (the stream
// psfp_trap_gen uses) or, with R_in, the caller's own draw from whatever TrapdoorDistribution it uses (`params.distribution.sample(...)`,
// gadget_classical.rs:62-64 -- a trait object in the reference, trapdoor_distribution.rs:21-48); A = [A_bar | H G - A_bar R] on the device
static psf_status gen_trapdoor_core(int device, const psf_gadget_params* gp, const uint64_t* a_bar, const uint64_t* tag, uint64_t seed, const int64_t* R_in,
                                    uint64_t* A, int8_t* R_out) {
  if (!gp || !a_bar || !A) return PSF_ERR_PARAM;
  psfp_params prm;
  prm.gp = *gp; prm.r = 1.0; prm.s = 1.0; prm.device = device; prm.flags = PSFP_FLAG_NO_PERTURB;
  psfp_handle* h = nullptr;
  psf_status rc = psfp_create(&prm, &h);
  if (rc != PSF_OK) return rc;
  if (gadget_too_short(gp->base, h->k, h->q)) { psfp_destroy(h); return PSF_ERR_MODULUS; }
  DevBuf dtag;
  auto fail = [&](psf_status st) { psfp_destroy(h); return st; };
  if (hipMemcpy2D(h->dA, h->m * sizeof(uint64_t), a_bar, h->mb * sizeof(uint64_t), h->mb * sizeof(uint64_t), h->n, hipMemcpyHostToDevice) != hipSuccess) return fail(PSF_ERR_HIP);
  if (tag) {
    if (dtag.alloc(h->n * h->n * sizeof(uint64_t)) != hipSuccess || dtag.upload(tag, h->n * h->n * sizeof(uint64_t)) != hipSuccess) return fail(PSF_ERR_HIP);
  }
  if (R_in) {
    // the trapdoor lives in int8 on the device (operand of the int8 matrix cores in e = p + [R; I] z and of the dot4 assembly of Sigma_2)
    std::vector<int8_t> r8(h->mb * h->w);
    for (size_t i = 0; i < r8.size(); ++i) {
      if (R_in[i] > 127 || R_in[i] < -127) return fail(PSF_ERR_UNSUPPORTED);
      r8[i] = (int8_t)R_in[i];
    }
    h->r8_valid = false; h->small_state = 0;
    if (hipMemset(h->dR, 0, h->mb_pad * h->ldr) != hipSuccess) return fail(PSF_ERR_HIP);
    if (hipMemcpy2D(h->dR, h->ldr, r8.data(), h->w, h->w, h->mb, hipMemcpyHostToDevice) != hipSuccess) return fail(PSF_ERR_HIP);
  } else {
    h->r8_valid = false; h->small_state = 0;
    hipLaunchKernelGGL(k_sample_R, dim3(grid_for(h->mb * h->ldr)), dim3(256), 0, 0, seed, h->mb, h->w, h->ldr, h->dR);    // gadget_classical.rs:62-64
  }
  launch_zq_trapdoor(h, dtag.as<uint64_t>());                                                                                            // :66
  if (hipGetLastError() != hipSuccess) return fail(PSF_ERR_HIP);
  if (hipMemcpy(A, h->dA, h->n * h->m * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return fail(PSF_ERR_HIP);
  if (R_out && hipMemcpy2D(R_out, h->w, h->dR, h->ldr, h->w, h->mb, hipMemcpyDeviceToHost) != hipSuccess) return fail(PSF_ERR_HIP);
  return fail(PSF_OK);
}
psf_status psf_gen_trapdoor(int device, const psf_gadget_params* gp, const uint64_t* a_bar, const uint64_t* tag, uint64_t seed, uint64_t* A, int8_t* R) {
  if (!R) return PSF_ERR_PARAM;
  return gen_trapdoor_core(device, gp, a_bar, tag, seed, nullptr, A, R);
}
psf_status psf_gen_trapdoor_with_r(int device, const psf_gadget_params* gp, const uint64_t* a_bar, const uint64_t* tag, const int64_t* R, uint64_t* A) {
  if (!R) return PSF_ERR_PARAM;
  return gen_trapdoor_core(device, gp, a_bar, tag, 0, R, A, nullptr);
}

// contiguous shares of `total` rows for `world` workers: the first total % world workers get one row more
psf_status psf_shard_range(size_t total, int world, int rank, size_t* first, size_t* count) {
  if (world < 1 || rank < 0 || rank >= world || !first || !count) return PSF_ERR_PARAM;
  const size_t base = total / (size_t)world, rem = total % (size_t)world;
  *count = base + ((size_t)rank < rem ? 1 : 0);
  *first = (size_t)rank * base + ((size_t)rank < rem ? (size_t)rank : rem);
  return PSF_OK;
}

psf_status psfp_trap_gen(psfp_handle* h, uint64_t seed) {
  if (!h) return PSF_ERR_PARAM;
  if (h->prm.flags & PSFP_FLAG_NO_PERTURB) return PSF_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  KeygenClock kc("psfp");
  // A = [A_bar | G - A_bar R] (13 ms at C3) on the handle's low-priority stream beside the factorisation of Sigma_2, which needs R alone
  const psf_status rcg = gen_A_R(h, seed, h->side);
  if (rcg != PSF_OK) return rcg;
  kc.mark("A_bar, R (A on the side stream)");
  h->has_pub = h->has_R = true;
  const psf_status rc = build_sqrt_sigma2(h, h->prm.s);            // mp_perturbation.rs:227-231
  HIP_TRY(hipStreamSynchronize(h->side));
  if (rc != PSF_OK) { h->has_key = false; return rc; }
  kc.mark("sqrt(Sigma_2)");
  h->has_key = true;
  hp_prewarm(h);
  kc.mark("prewarm (returns at once)");
  return PSF_OK;
}

psf_status psfp_compute_sqrt_sigma_2(psfp_handle* h, double s_cov) {
  if (!h || !(s_cov > 0.0)) return PSF_ERR_PARAM;
  if (!h->has_R || (h->prm.flags & PSFP_FLAG_NO_PERTURB)) return PSF_ERR_NO_KEY;
  // The structured factor's constants g, h depend on the covariance parameter, and an exported key carries only L_1: psfp_load_key rebuilds them from
  // the handle's s.  A factor for another s_cov would therefore be paired with the wrong constants after an export / load round trip, silently; refused.
  if (h->structured && s_cov != h->prm.s) return PSF_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  const psf_status rc = build_sqrt_sigma2(h, s_cov);
  h->has_key = rc == PSF_OK;
  return rc;
}

// compute_sqrt_sigma_2 with a general covariance (mp_perturbation.rs:111: `mat_sigma: &MatQ` is any symmetric matrix, used as a full matrix at :125-126)
psf_status psfp_compute_sqrt_sigma_2_dense(psfp_handle* h, const double* sigma_lower_packed) {
  if (!h || !sigma_lower_packed) return PSF_ERR_PARAM;
  if (!h->has_R || (h->prm.flags & PSFP_FLAG_NO_PERTURB)) return PSF_ERR_NO_KEY;
  if (h->structured) return PSF_ERR_UNSUPPORTED;           // the structured factor exists for Sigma = s^2 I only
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  DevBuf dsg;
  const size_t np = h->m * (h->m + 1) / 2;
  HIP_TRY(dsg.alloc(np * sizeof(double)));
  HIP_TRY(dsg.upload(sigma_lower_packed, np * sizeof(double)));
  const psf_status rc = build_sqrt_sigma2(h, 0.0, dsg.as<double>());
  h->has_key = rc == PSF_OK;
  return rc;
}

psf_status psfp_load_key(psfp_handle* h, const uint64_t* A, const int8_t* R, const double* Lp) {
  if (!h || !A || (!R && Lp)) return PSF_ERR_PARAM;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  h->has_key = h->has_R = h->has_pub = false;
  HIP_TRY(hipMemcpy(h->dA, A, h->n * h->m * sizeof(uint64_t), hipMemcpyHostToDevice));
  split_A(h);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  h->has_pub = true;
  if (!R) return PSF_OK;                                    // public key only: the verifier's handle (f_a, check_domain, samp_d)
  h->r8_valid = false; h->small_state = 0;
  HIP_TRY(hipMemset(h->dR, 0, h->mb_pad * h->ldr));
  HIP_TRY(hipMemcpy2D(h->dR, h->ldr, R, h->w, h->w, h->mb, hipMemcpyHostToDevice));
  h->has_R = true;
  if (h->prm.flags & PSFP_FLAG_NO_PERTURB) return PSF_OK;
  if (!Lp) {                                                // trapdoor without its factor: recompute it as trap_gen does (mp_perturbation.rs:227-231)
    const psf_status rc = build_sqrt_sigma2(h, h->prm.s);
    h->has_key = rc == PSF_OK;
    return rc;
  }
  DevBuf dp;
  const size_t np = h->mL * (h->mL + 1) / 2;
  HIP_TRY(dp.alloc(np * sizeof(double)));
  HIP_TRY(dp.upload(Lp, np * sizeof(double)));
  hipLaunchKernelGGL(k_repack_L<true>, dim3(grid_for(tr_total_chunks(h->nbiL) * TR_CHUNK)), dim3(256), 0, 0, dp.as<double>(), (size_t)0, h->mL, h->dLt, h->nbiL);
  if (h->structured) {      // the constants of the structured factor follow from (r, s): the same expressions as build_sqrt_sigma2
    const double nf_r2 = (1.0 / 6.283185307179586476925) * (h->prm.r * h->prm.r), kappa = (double)(h->prm.gp.base * h->prm.gp.base + 1);
    const double alpha = h->prm.s * h->prm.s - 1.0, beta = alpha - kappa;
    if (!(beta > 0.0)) return PSF_ERR_NOT_PD;
    h->g_const = (std::sqrt(nf_r2) * kappa) / std::sqrt(beta);
    h->h_const = std::sqrt(nf_r2 * beta);
    ensure_R8(h, nullptr);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  h->has_key = true;
  hp_prewarm(h);
  return PSF_OK;
}

// (A, R) without a factor: what PSFPerturbation::compute_sqrt_sigma_2 (mp_perturbation.rs:111) needs installed -- it is a pure function of mat_r and
// mat_sigma in the reference, so A may be NULL (the handle's public matrix, if any, stays).  No Sigma_2 is assembled and nothing is factored here
// (psfp_load_key(A, R, NULL) runs a full Cholesky with the handle's s); samp_p answers PSF_ERR_NO_KEY until psfp_compute_sqrt_sigma_2(_dense) has run.
psf_status psfp_load_trapdoor(psfp_handle* h, const uint64_t* A, const int8_t* R) {
  if (!h || !R) return PSF_ERR_PARAM;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  h->has_key = h->has_R = false;
  if (A) {
    h->has_pub = false;
    HIP_TRY(hipMemcpy(h->dA, A, h->n * h->m * sizeof(uint64_t), hipMemcpyHostToDevice));
    split_A(h);
    HIP_TRY(hipGetLastError());
    h->has_pub = true;
  }
  h->r8_valid = false; h->small_state = 0;
  HIP_TRY(hipMemset(h->dR, 0, h->mb_pad * h->ldr));
  HIP_TRY(hipMemcpy2D(h->dR, h->ldr, R, h->w, h->w, h->mb, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  h->has_R = true;
  return PSF_OK;
}

psf_status psfp_export_key(const psfp_handle* h, uint64_t* A, int8_t* R, double* Lp) {
  if (!h) return PSF_ERR_PARAM;
  if (!h->has_pub || ((R || Lp) && !h->has_R) || (Lp && !h->has_key)) return PSF_ERR_NO_KEY;
  HIP_TRY(hipSetDevice(h->prm.device));
  if (A) HIP_TRY(hipMemcpy(A, h->dA, h->n * h->m * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (R) HIP_TRY(hipMemcpy2D(R, h->w, h->dR, h->ldr, h->w, h->mb, hipMemcpyDeviceToHost));
  if (Lp) {
    DevBuf dp;
    const size_t np = h->mL * (h->mL + 1) / 2;
    HIP_TRY(dp.alloc(np * sizeof(double)));
    hipLaunchKernelGGL(k_unpack_L, dim3(grid_for(np)), dim3(256), 0, 0, h->dLt, (size_t)0, np, dp.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(dp.download(Lp, np * sizeof(double)));
  }
  return PSF_OK;
}

// rows [row0, row0 + nrows) of the factor, packed (row i: i + 1 entries): keys of tens of GB are read back in pieces
psf_status psfp_export_sqrt_sigma2_rows(const psfp_handle* h, size_t row0, size_t nrows, double* out) {
  if (!h || (nrows && !out) || row0 + nrows > h->mL || (h->prm.flags & PSFP_FLAG_NO_PERTURB)) return PSF_ERR_PARAM;
  if (!h->has_key) return PSF_ERR_NO_KEY;
  if (nrows == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  const size_t first = row0 * (row0 + 1) / 2, total = (row0 + nrows) * (row0 + nrows + 1) / 2 - first;
  DevBuf dp;
  HIP_TRY(dp.alloc(total * sizeof(double)));
  hipLaunchKernelGGL(k_unpack_L, dim3(grid_for(total)), dim3(256), 0, 0, h->dLt, first, total, dp.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(dp.download(out, total * sizeof(double)));
  return PSF_OK;
}

psf_status psfp_export_gadget_basis(const psfp_handle* h, int64_t* Sk, double* gso) {
  if (!h) return PSF_ERR_PARAM;
  if (Sk) std::memcpy(Sk, h->hSk.data(), h->hSk.size() * sizeof(int64_t));
  if (gso) std::memcpy(gso, h->hGso.data(), h->hGso.size() * sizeof(double));
  return PSF_OK;
}

// ---- the hot path -------------------------------------------------------------------------------------------
// One samp_p call (mp_perturbation.rs:304-336): plan_samp_p makes every form choice (the experiment switches of this path are read there and in plan_zq only),
// prepare_samp_p runs the side effects the plan names, each once, and the stage launchers enqueue what the plan says on `st`, each stage for the whole batch.
static bool small_usable(const psfp_handle* h) { return h->small_state == 2 || h->small_state == 3; }
static const auto by_cols = [](size_t b, auto k1, auto k2, auto k4) { return b == 1 ? k1 : b == 2 ? k2 : k4; };      // the <1, 2, 4> instantiation for b preimages

struct ZqPlan {      // out = (syndrome) U - A P  or  (f_a) A P over ncols preimages
  enum Form : uint8_t { SMALL, SMALL32, MFMA } form = MFMA;      // A streamed once as 64-bit words / as its compact 32-bit copy; P's digit planes on the int8 matrix cores
  int splits = 1, ks = 0;                                         // K splits (SMALL: of SYN_KLEN columns; MFMA: of ks K-steps)
  bool fold128 = false, pow2 = false, wave_combine = true;        // k_zq_mfma's template arguments; the splits summed by one wave per output (k_zq_combine_wave)
};

// (split_cap: h->zq_split_cap, or what ensure_batch would make it -- the plan query)
static ZqPlan plan_zq(const psfp_handle* h, size_t ncols, bool syndrome, int split_cap = -1) {
  ZqPlan z;
  if (split_cap < 0) split_cap = h->zq_split_cap;
  if (syndrome) {  // a handful of preimages: A streamed once as 64-bit words (k_syndrome_small; PSF_SYNDROME_SMALL = largest batch it serves, 0: never)
    size_t small_max = 1;                                             // measured at C3: 39 vs 48 us at one preimage, 52 vs 50 at two, 81 vs 50 at four (64-bit multiply-adds)
    if (const char* e = psf_exp_env("PSF_SYNDROME_SMALL")) small_max = std::min<size_t>((size_t)std::atol(e), 4);
    z.splits = (int)((h->m + SYN_KLEN - 1) / SYN_KLEN);
    if (ncols <= small_max && z.splits <= split_cap && z.splits <= 64) {
      z.form = h->dA32 && small_usable(h) ? ZqPlan::SMALL32 : ZqPlan::SMALL;
      return z;
    }
  }
  const int nks = (int)(h->K_pad / 64);
  z.splits = zq_plan(h, ncols, split_cap);
  z.ks = (nks + z.splits - 1) / z.splits;
  z.fold128 = z.ks <= 32;                                             // short splits (few preimages): one 128-bit fold per output; long ones: the per-class fold
  if (const char* e = psf_exp_env("PSF_ZQ_FOLD128")) z.fold128 = std::atoi(e) != 0;
  // a power-of-two modulus covered by the digits of A: the classes from NA on vanish mod q (pw[NA] = 0) and their digit pairs are skipped
  z.pow2 = (h->q & (h->q - 1)) == 0 && h->NA <= 8 && h->zc.pw[h->NA] == 0;
  z.wave_combine = z.splits >= 16 && h->n * ncols <= 16384;          // a single call: few outputs, many splits -- one wave per output
  return z;
}

static void launch_zq(psfp_handle* h, hipStream_t st, const ZqPlan& z, int mode, const int32_t* P, int8_t* P8, size_t ncols, const uint64_t* U, uint64_t* out, size_t ldo) {
  const size_t ld = h->ld;
  if (z.form == ZqPlan::MFMA) {
    const size_t cw = std::min(round_up(ncols, 64), ld);            // the product works on 64-column tiles
    hipLaunchKernelGGL(k_split_P, dim3(grid_for(h->K_pad / 16 * cw, 256, 256 * 64)), dim3(256), 0, st, P, h->m, ld, h->K_pad / 16, P8, h->dFail, (size_t)0, cw);
    const dim3 grid((unsigned)((ncols + 63) / 64), (unsigned)(h->n_pad / 64), (unsigned)z.splits);
    auto fp = [&](auto k_tt, auto k_tf, auto k_ft, auto k_ff) { return z.fold128 ? (z.pow2 ? k_tt : k_tf) : (z.pow2 ? k_ft : k_ff); };      // <NA, fold128, pow2>
#define ZQM(NA_) case NA_: hipLaunchKernelGGL(fp(k_zq_mfma<NA_, true, true>, k_zq_mfma<NA_, true, false>, k_zq_mfma<NA_, false, true>, k_zq_mfma<NA_, false, false>), grid, dim3(256), \
                                              2 * (NA_ + 3) * 4096, st, h->dA8, h->n_pad, h->K_pad, P8, ld, z.ks, h->zc, (int)h->wide, h->dPart, (size_t)0, h->dFail); break;
    switch (h->NA) { ZQM(1) ZQM(2) ZQM(3) ZQM(4) ZQM(5) ZQM(6) ZQM(7) ZQM(8) default: break; }
#undef ZQM
  } else {      // 16 rows per workgroup
    const dim3 grid((unsigned)z.splits, (unsigned)((h->n + 15) / 16));
    if (z.form == ZqPlan::SMALL32)
      hipLaunchKernelGGL(by_cols(ncols, k_syndrome_small32<1>, k_syndrome_small32<2>, k_syndrome_small32<4>), grid, dim3(512), 0, st, h->dA32, h->n, h->m, P, ld, ncols, h->q, 16,
                         h->dPart, h->n_pad, (size_t)0);
    else
      hipLaunchKernelGGL(by_cols(ncols, k_syndrome_small<1>, k_syndrome_small<2>, k_syndrome_small<4>), grid, dim3(512), 0, st, h->dA, h->n, h->m, P, ld, ncols, h->q, 16,
                         h->dPart, h->n_pad, (size_t)0);
  }
  hipLaunchKernelGGL(z.wave_combine ? k_zq_combine_wave<false> : k_zq_combine, dim3(z.wave_combine ? (unsigned)((h->n * ncols + 3) / 4) : grid_for(h->n * ncols, 256, 256 * 32)),
                     dim3(256), 0, st, mode, h->dPart, z.splits, h->n, h->n_pad, ld, ncols, h->q, U, out, ldo, (size_t)0);
}

struct SampCall {      // what one samp_p pass is told by its caller: passed down from the entry point, nothing of it stays on the handle
  bool keep_fail = false;                                    // dFail[0..3] are not cleared at the head of the pass (the slices of one host call; batch 1 and later of a many-call)
  bool whole_batch = false;                                  // a stage export wants the intermediates of the whole batch: no one-launch form, the straight host path, no cuts
  const HostStage* before_u = nullptr;                       // host path: stages the targets; run_samp_p calls it in front of the first stage that reads them (hp_async owns it)
  const std::chrono::steady_clock::time_point* launched = nullptr;      // psfp_samp_p_multi: the call's start, against which the first enqueued pass stamps multi_launched_ms
};

struct SampPlan {      // every form choice of one samp_p call, with the launch parameters the choices fix
  size_t nbj = 0;                                            // 128-column blocks of the rows of this pass
  bool one_launch = false;                                   // k_samp_p_small: the whole call
  int bc = 0; uint32_t ncf = 0, nseg = 0; size_t nwaves = 0;  // normals: dense stream of bc preimages; layout code (h->normals_ncf; 0 = chunk stream); positions per wave, waves
  enum Product : uint8_t { TASKS, TILES64, TILES32, TILES96, BIG } product = BIG;      // x = sqrt(Sigma_2) d
  int RT = 2, NB = 1, ncg = 1;                               // TASKS: RT 16-row tiles x NB fragments per wave; column groups of 16 NB preimages
  bool compact = false; int GR = 8, GC = 4;                  // the streaming kernels read the compact normals stream; BIG: super-tile of an XCD's 32 resident workgroups
  bool tail = false; int tail_ntask = 0, tail_rt = 2;        // rounding and the shares of A p in one launch behind the product (k_round_syndrome_small)
  enum Round : uint8_t { ROUND_TAB, ROUND_TAB_ROW, ROUND_LEAN, ROUND_WAVE } round = ROUND_WAVE;
  uint32_t seg = 0; size_t rwaves = 0;                       // rounding: samples per wave, waves
  ZqPlan syn;                                                // v = u - A p without the fused tail
  enum Gadget : uint8_t { G_WAVE, G_ROW, G_QUAD, G_QUEUE, G_LOCKSTEP } gadget = G_LOCKSTEP;
  bool k32 = false; int gq_p = 0;                            // G_ROW, G_QUAD: the k <= 32 instantiation (else k <= 64); G_QUEUE: problems per wave
  enum Recombine : uint8_t { R_SMALL, R_SMALL2, R_WG, R_TILES } recombine = R_TILES;
  size_t rc_lds = 0; unsigned rc_wgs = 0; int nbf = 0;       // R_SMALL(2): LDS, workgroups; R_WG: fragments of 16 preimages per column group
  bool rc_big = false; int rsplits = 1, kps = 0;             // R_TILES: the 256 x 256 tiles first; k_recombine_mfma over rsplits pieces of kps K-steps
  bool small_copies = false, r8 = false;                     // prepare_samp_p: ensure_small_copies, ensure_R8
};

struct BatchDims { size_t nbj; int zq_split_cap; };      // what ensure_batch derives from B and the plan reads

// The forms of a pass over B preimages, from the handle as it stands at the start of the call (after ensure_batch; psfp_query_plan hands in what ensure_batch would leave)
static SampPlan plan_samp_p(const psfp_handle* h, size_t B, const SampCall& call, const BatchDims* bd = nullptr) {
  SampPlan p;
  const size_t m = h->m;
  const size_t nbj = p.nbj = bd ? bd->nbj : round_up(B, TR_BN) / TR_BN;
  // small parameter sets, few preimages (the reference's own benchmarks: n = 8, one call; benches/psf.rs:51-66): the whole call in ONE launch, one
  // workgroup per preimage (k_samp_p_small).  PSF_FUSED_MAX = largest batch it serves (0: never).  Stage exports need the intermediates: not here.
  size_t fused_max = 64;
  if (const char* e = psf_exp_env("PSF_FUSED_MAX")) fused_max = (size_t)std::atol(e);
  p.one_launch = !h->structured && !call.whole_batch && h->gadget_queue && m <= (size_t)FS_MAX_M && h->n <= 64 && B <= fused_max;
  if (p.one_launch) return p;
  // Small batches (one samp_p call of the reference is ONE preimage, psf.rs:48-80): the streaming product, bound by reading the factor once, fed by
  // the compact normals stream.  PSF_TRMM_STREAM_MAX = largest batch it serves (0 switches it off); PSF_TRMM_STREAM_SHAPE = "RT,NB" forces a tile
  // shape (and turns the shared tiles off), PSF_COMPACT_D=0 the chunk-stream layout of the normals (experiments; same bits).
  // measured at C3: the streaming forms win up to 1472 preimages and again at 1537 ... 1728 (round 6, tools/tail_ab.py k_trmm_f64: k_trmm_f64_big costs 22.2-22.5 ms for anything
  // between 1025 and 1536 preimages and 27.2 up to 2048, the 64 x 64 tiles ~0.97 ms per round of 256 workgroups: 16.5 ms at 1152, 18.6 at 1280, 21.8 at 1472, 23.8 at 1600, 26.9 at 1792)
  bool stream = B <= 1472 || (B >= 1537 && B <= 1728) || (h->mL < 16384 && B <= 2048);      // (a small factor: k_trmm_f64_big is a fixed 0.23 ms at m = 932 whatever the batch, the
                                                                                            // tiles 0.04 ms at 1100 ... 2048 preimages: no reason to leave them before the stream's limit)
  // (PSF_TRMM_STREAM_MAX <= 2048 = 128 column fragments: beyond, the over-read of the compact normals stream would leave TS_SLACK_DOUBLES)
  if (const char* e = psf_exp_env("PSF_TRMM_STREAM_MAX")) stream = B <= std::min<size_t>((size_t)std::atol(e), 2048);
  const char* shape = psf_exp_env("PSF_TRMM_STREAM_SHAPE");
  // tile shape per wave (RT 16-row tiles x NB fragments of 16 preimages) and workgroup form, from tools/probe_stream.hip at the C3 shape
  // (profiles/r04_probe_stream.log): <= 16 preimages the launch is bound by reading the factor, beyond that by the longest MFMA chain
  p.NB = B <= 16 ? 1 : B <= 64 ? 2 : 4;
  // more than wg_min preimages: 64 x 64 tiles whose four waves share the operands through LDS (k_trmm_stream_wg); PSF_STREAM_WG=0 keeps the one-wave tasks,
  // PSF_STREAM_WG=<B> moves the threshold (experiments build; same bits)
  size_t wg_min = 33;
  if (const char* e = psf_exp_env("PSF_STREAM_WG")) wg_min = std::atol(e) > 0 ? (size_t)std::atol(e) : (size_t)-1;
  size_t wg_max = 64;            // measured at C3 (tools/stream_wg_ab.py): 0.91-0.96 against 1.26 ms at 33 ... 64 preimages; 241 workgroups on 256 CUs, each as long as its pair of
                                 // chains: 0.87 ms would be the matrix pipe's time on 241 CUs.  Beyond 64 preimages the forms tried (column groups of 64 with one or two
                                 // workgroups per CU, column groups of 128 on halves of eight waves) end within 5 % of the one-wave tasks: PSF_STREAM_WG_MAX (<= 64)
  if (const char* e = psf_exp_env("PSF_STREAM_WG_MAX")) wg_max = std::min<size_t>((size_t)std::atol(e), 64);
  // Beyond 128 preimages with an ODD number of column groups of 64 (129-192, 257-320, ... 897-960): the same tiles, the column groups of a tile group on one XCD -- the
  // one-wave tasks take as long as for the next even count there (192 preimages cost what 256 do: their eight-wave workgroups hold 4 + 4 tasks, column groups of a
  // tile group side by side), the tiles' workgroups are all of one length: 2.8-2.9 against 3.7-3.9 ms at 129-192, 4.8 / 5.9 at 320, 6.6 / 7.9 at 448, 8.6 / 9.9 at 576,
  // 14.5 / 15.9 at 960; with an even count the two forms tie (1.96 / 1.94 at 128, 7.70 / 7.69 at 512, 15.5 / 15.0 at 1024).  PSF_STREAM_WG192=0 keeps the one-wave
  // tasks, "lo:hi" forces the tiles for every batch size in the range (experiments build; same bits)
  // a small factor (m < 16 384: few tile groups, the launch lasts one chain): the tiles' waves hold 2 x 2 MFMA tiles against the one-wave tasks' 2 x 4 -- half the chain
  // (m = 932: 0.035 against 0.061 ms at 97 ... 1024 preimages, whatever the parity): the tiles from 65 preimages on
  const bool small_factor = h->mL < 16384;
  bool wg192 = stream && ((B > 128 && B <= 960 && (((B + 63) / 64) & 1) != 0) || B > 1088 || (small_factor && B > 64)) && !shape;      // (1025-1088: 15.9 against 16.5)
  if (const char* e = psf_exp_env("PSF_STREAM_WG192")) {
    long lo = 0, hi = 0;
    wg192 = std::sscanf(e, "%ld:%ld", &lo, &hi) == 2 && lo >= 65 && hi <= 2048 && stream && B >= (size_t)lo && B <= (size_t)hi && !shape;
  }
  const bool wg = stream && ((B >= wg_min && B <= wg_max) || wg192) && !shape;
  // 17 ... 32 preimages: 64 x 32 tiles of the same ring (k_trmm_stream_wg32); PSF_STREAM_WG32=0 keeps the one-wave tasks (experiments build; same bits)
  const char* e32 = psf_exp_env("PSF_STREAM_WG32");
  const bool wg32 = stream && !wg && B >= 17 && B <= 32 && !shape && !(e32 && std::atoi(e32) == 0);
  // 65 ... 96 preimages: the first 64 on the 64 x 64 tiles, the rest on the 64 x 32 tiles, two launches over one normals stream of six fragments (0.94 + 0.65 ms against 1.80 for
  // the one-wave tasks, which pay for 128 columns); PSF_STREAM_WG96=0 keeps those (experiments build; same bits)
  const char* e96 = psf_exp_env("PSF_STREAM_WG96");
  const bool wg96 = stream && !wg && !small_factor && B >= 65 && B <= 96 && !shape && !(e96 && std::atoi(e96) == 0);
  if (wg) p.NB = 4;                    // column groups of 64 preimages (halves of four waves)
  if (wg32 || wg96) p.NB = 2;          // (wg96: three column groups of 32 = the six fragments of the stream)
  if (shape) std::sscanf(shape, "%d,%d", &p.RT, &p.NB);
  if (!(p.NB == 1 || p.NB == 2 || p.NB == 4 || p.NB == 8)) p.NB = 1;
  p.ncg = (int)((B + 16 * (size_t)p.NB - 1) / (16 * (size_t)p.NB));
  const char* ecd = psf_exp_env("PSF_COMPACT_D");
  p.compact = stream && !h->structured && !(ecd && std::atoi(ecd) == 0);
  // <= 16 preimages in one fragment: the dense stream of bc = 1, 2, 4, 8, 16 preimages (PSF_COMPACT_D=1 keeps the fragment stream)
  if (p.compact && p.NB == 1 && p.ncg == 1 && !(ecd && std::atoi(ecd) == 1)) { p.bc = 1; while ((size_t)p.bc < B) p.bc <<= 1; }
  p.ncf = p.bc ? 0x100u + (uint32_t)p.bc : p.compact ? (uint32_t)(p.ncg * p.NB) : 0u;
  const size_t npos = p.bc ? h->nkb * 4 * 4 * (size_t)p.bc : p.ncf ? h->nkb * 4 * (size_t)p.ncf * 64 : nbj * h->nkb * TR_CHUNK;
  p.nseg = nr_segment(npos);
  if (const char* e = psf_exp_env("PSF_NR_SEG")) { const long v = std::atol(e); if (v >= 64 && v <= NR_SEG && v % 64 == 0) p.nseg = (uint32_t)v; }      // positions per wave (experiments)
  p.nwaves = (npos + p.nseg - 1) / p.nseg;
  if (!stream) {                 // k_trmm_f64_big: one workgroup per CU, accumulators in AccVGPRs
    p.product = SampPlan::BIG;   // super-tile of an XCD's 32 resident workgroups; PSF_TRMM_GR x PSF_TRMM_GC for experiments (product = 32)
    // below 4096 preimages, or with a number of 128-column blocks that is not a multiple of four: 16 x 2 -- the grid is padded to whole super-columns, and 8 x 4 pays for up
    // to three empty column blocks (round 6, tools/tail_ab.py: 34.9 -> 32.3 ms at 2176, 47.8 -> 44.1 at 3200, 27.2 -> 26.3 at 2048; 51.9 against 52.5 at 4096: 8 x 4 stays there)
    if (B < 4096 || nbj % 4 != 0) { p.GR = 16; p.GC = 2; }
    if (const char* e1 = psf_exp_env("PSF_TRMM_GR")) if (const char* e2 = psf_exp_env("PSF_TRMM_GC")) { p.GR = std::atoi(e1); p.GC = std::atoi(e2); }
    if (p.GR < 1 || p.GC < 1 || p.GR * p.GC != 32) { p.GR = 8; p.GC = 4; }
  } else p.product = wg96 ? SampPlan::TILES96 : wg32 ? SampPlan::TILES32 : wg ? SampPlan::TILES64 : SampPlan::TASKS;
  // One or two preimages: rounding and syndrome in ONE launch behind the product (k_round_syndrome_small, psf_stream_kernels.hpp) once the transposed compact copy
  // of A is there (built beside the first small calls after a key change, as the other compact copies)
  if (stream && p.bc && B <= 2 && p.RT == 2 && p.NB == 1 && !h->structured && h->szR.sh == 16 && !(h->prm.flags & PSFP_FLAG_NO_PERTURB)) {
    p.small_copies = true;
    const char* fe = psf_exp_env("PSF_FUSED_TAIL");
    if (h->dA32T && small_usable(h) && !(fe && std::atoi(fe) == 0)) {
      // (tail_rt: 16-row tiles of x per wave; two: 27 + 10 us against 34 + 14 with one, tools/fused_tail_ab.sh)
      if (const char* e = psf_exp_env("PSF_FUSED_RT")) p.tail_rt = std::atoi(e) == 1 ? 1 : 2;
      p.tail_ntask = ((int)((h->mL + 15) / 16) + p.tail_rt - 1) / p.tail_rt;      // one wave per tail_rt 16-row tiles of x
      p.tail = true;                                                               // (if prepare_samp_p finds room for its residues)
    }
  }
  p.r8 = h->structured;          // x_top -= g R d_2 reads the tile-packed R
  // p_i <- D_{Z,r,x_i}
  const char* renv = psf_exp_env("PSF_ROUND");                 // "wave": the round-2 kernel (comparison arm; same bits)
  if (h->szR.sh == 16 && !(renv && !std::strcmp(renv, "wave"))) {
    p.seg = prl_segment(m * B);
    if (const char* e = psf_exp_env("PSF_PRL_SEG")) { const long v = std::atol(e); if (v >= 64 && v <= PRL_SEG && v % 64 == 0) p.seg = (uint32_t)v; }      // samples per wave (experiments)
    p.round = SampPlan::ROUND_LEAN;
    if (h->szF && !(renv && !std::strcmp(renv, "lean"))) {     // the table screen ("lean": the fp32 screen of rounds 3-4, comparison arm; same bits)
      // a segment that is one row of the [coordinate][preimage] matrix never wraps: the sample's position is its offset (no division per sample)
      if (B % 64 == 0 && B >= 1024 && B <= (size_t)PRL_SEG && (size_t)p.seg > B) p.seg = (uint32_t)B;      // (short rows: every workgroup loads the table, 0.14 against 0.09 ms at 64 preimages)
      p.round = (size_t)p.seg == B ? SampPlan::ROUND_TAB_ROW : SampPlan::ROUND_TAB;
    }
    p.rwaves = (m * B + p.seg - 1) / p.seg;
  } else p.rwaves = (m * B + PR_SEG - 1) / PR_SEG;
  // mp_perturbation.rs:318 -- v = u - A p (the Z_q product unless the fused tail left the shares of A p)
  p.syn = plan_zq(h, B, true, bd ? bd->zq_split_cap : -1);
  p.small_copies |= p.syn.form != ZqPlan::MFMA;
  // mp_perturbation.rs:321-326 -- z <- D_{Lambda_v(G), r sqrt(b^2+1)}
  const size_t nB = h->n * B;
  const char* genv = psf_exp_env("PSF_GADGET_WAVE");            // max n B served by the one-wave-per-problem kernel (0: never)
  const size_t wave_max = genv ? (size_t)std::atol(genv) : 2048;    // measured at C3 (n = 512): 45 / 44 / 55 us at 1 / 2 / 4 preimages (a row per problem: 58); 91 against 58 at 8
  const char* genvq = psf_exp_env("PSF_GADGET_QUAD");          // max n B served by the four-lanes-per-problem kernel (0: never)
  const size_t quad_max = genvq ? (size_t)std::atol(genvq) : 98304;      // measured at C3 (tools/gadget_mid_ab.py): 0.092 / 0.092 / 0.12 / 0.24 ms at 16 / 32 / 64 / 128 preimages against
                                                                            // 0.12 / 0.18 / 0.33 / 0.35; 0.39 against 0.33 (queue kernel) at 256
  const char* genvr = psf_exp_env("PSF_GADGET_ROW");           // max n B served by the sixteen-lanes-per-problem form of k_gadget_quad (0: never)
  const size_t row_max = genvr ? (size_t)std::atol(genvr) : 10240;      // measured at C3 (tools/tail_ab.py k_gadget): 0.058 / 0.071 / 0.088 ms at 8 / 16 / 24 preimages against 0.091 (one
                                                                          // wave per problem at 8, a quad per problem at 16 and 24); 0.107 against 0.091 at 32
  p.k32 = h->k <= 32;
  if (!h->gadget_queue) p.gadget = SampPlan::G_LOCKSTEP;
  else if (nB <= wave_max) p.gadget = SampPlan::G_WAVE;              // a single call / a handful of preimages: the chain of k draws is the launch time
  else if (nB <= row_max && h->k <= 64) p.gadget = SampPlan::G_ROW;  // a few thousand problems: a DPP row per problem, one round per draw
  else if (nB <= quad_max && h->k <= 64) p.gadget = SampPlan::G_QUAD;      // tens to a few hundred preimages: a quad per problem
  else {
    p.gadget = SampPlan::G_QUEUE;
    p.gq_p = gq_problems_for((uint32_t)h->k, nB);
    if (const char* e = psf_exp_env("PSF_GQ_P")) { const int v = std::atoi(e); if (v >= 1 && v <= 128 && (v & (v - 1)) == 0) p.gq_p = v; }      // problems per wave (experiments)
  }
  // mp_perturbation.rs:328-335 -- e = p + [R; I] z
  // a handful of preimages: R streamed once by one wave per row (PSF_RECOMBINE_SMALL = largest batch it serves, 0: never)
  size_t small_max = 4;
  if (const char* e = psf_exp_env("PSF_RECOMBINE_SMALL")) small_max = std::min<size_t>((size_t)std::atol(e), 4);
  p.rc_lds = 32 * (h->ldr / 16) * B;
  // 5 ... 448 preimages: 64 x 64 tiles over all of K, operands through an LDS-DMA ring, no atomics (k_recombine_wg); PSF_RECOMBINE_STREAM=0: the tiled kernel below
  // (experiments build; same rows): 0.067 against 0.091 ms at 16, 0.081 against 0.155 at 64 preimages of C3 (tools/tail_ab.py)
  size_t rs_max = 448;      // column groups of 64 preimages beyond 64 (blockIdx.y; R comes from L2 / the Infinity Cache for all but the first): 0.157 -> 0.107 ms at 65, 0.266 -> 0.115 at 128,
                            // 0.247 -> 0.174 at 192, 0.238 -> 0.210 at 256, 0.353 -> 0.299 at 384; 0.248 -> 0.390 at 512 (the 256 x 256 tiles), 0.575 -> 0.729 at 1000 preimages
  if (const char* e = psf_exp_env("PSF_RECOMBINE_STREAM")) rs_max = (size_t)std::min<long>(std::atol(e), 1024);
  if (B <= small_max && p.rc_lds <= 150 * 1024) {
    p.recombine = h->small_state == 2 ? SampPlan::R_SMALL2 : SampPlan::R_SMALL;
    p.rc_wgs = (unsigned)std::min<size_t>((h->mb + 7) / 8, p.rc_lds > 64 * 1024 ? 256 : 512);
    p.small_copies = true;
  } else if (B <= rs_max && h->ldr % 128 == 0 && h->mb >= 64) {
    p.recombine = SampPlan::R_WG;
    p.nbf = B > 64 ? 4 : (int)((B + 15) / 16);      // (four waves at 33 ... 64 preimages: 0.147 against 0.081 ms)
  } else {
    // one digit plane (decided on the device by the gadget kernel): 256 x 256 tiles; otherwise, or for shapes the big tile does not fit, the 128 x 128 kernel
    // (beyond 448 preimages also for batches that are not multiples of 256: the last tile is ragged -- its loads of z past the batch stay inside the planes or their slack,
    // the stores are masked -- and still cheaper than the 128 x 128 kernel: 0.437 -> 0.29 ms at 704, 0.548 -> 0.30 at 832 preimages)
    p.recombine = SampPlan::R_TILES;
    p.rc_big = (B % 256 == 0 || B > rs_max) && h->mb >= 512 && (h->ldr / 64) % 2 == 0;
    p.r8 = p.r8 || p.rc_big;
    // few preimages: cut K over blockIdx.z (an even number of K steps each, at least 8) until ~2048 workgroups; the partial sums are added into a zeroed E
    const unsigned tiles = (unsigned)((B + 127) / 128) * (unsigned)((h->mb + 127) / 128);
    const int nks = (int)(h->ldr / 64);
    p.kps = nks;
    if (!p.rc_big && tiles < 1024 && nks >= 16) {
      const int splits = (int)(2048 / tiles);
      p.kps = std::max((nks + splits - 1) / splits, 8);
      p.kps += p.kps & 1;
      p.rsplits = (nks + p.kps - 1) / p.kps;
    }
  }
  return p;
}

// psfp_query_plan / psfp_get_last_plan: the form choices in the order of include/psf_mi355x.h (PSFP_PLAN_*)
static_assert(SampPlan::BIG == PSFP_PRODUCT_BIG && SampPlan::TILES96 == PSFP_PRODUCT_TILES96 && SampPlan::TILES64 == PSFP_PRODUCT_TILES64 && SampPlan::ROUND_WAVE == PSFP_ROUND_WAVE &&
              SampPlan::ROUND_TAB_ROW == PSFP_ROUND_TAB_ROW && ZqPlan::MFMA == PSFP_ZQ_MFMA && ZqPlan::SMALL32 == PSFP_ZQ_SMALL32 && SampPlan::G_LOCKSTEP == PSFP_GADGET_LOCKSTEP &&
              SampPlan::G_QUAD == PSFP_GADGET_QUAD && SampPlan::R_TILES == PSFP_RECOMBINE_TILES && SampPlan::R_SMALL2 == PSFP_RECOMBINE_SMALL2 && PSFP_PLAN_RSPLITS == 22,
              "the enumerators of include/psf_mi355x.h follow SampPlan");
static void plan_fields(const SampPlan& p, int* f) {
  const int v[PSFP_PLAN_FIELDS] = {p.one_launch, p.product, p.RT, p.NB, p.ncg, p.bc, p.compact, p.GR, p.GC, p.tail, p.round, p.syn.form, p.syn.splits, p.syn.fold128, p.syn.pow2,
                                   p.syn.wave_combine, p.gadget, p.k32, p.gq_p, p.recombine, p.nbf, p.rc_big, p.rsplits};
  std::memcpy(f, v, sizeof(v));
}

// The side effects a plan names, each once per call: the compact copies (built beside the call; a later call's plan finds them usable), room for the fused
// tail's partial residues, the tile-packed R
static void prepare_samp_p(psfp_handle* h, hipStream_t st, SampPlan& p) {
  if (p.small_copies) ensure_small_copies(h, st);
  if (p.tail) {
    const size_t need = (size_t)p.tail_ntask * h->n * 2;
    if (h->dPartF.grow(need) != hipSuccess) (void)hipGetLastError();
    p.tail = h->dPartF != nullptr;      // (no room: the syndrome stage takes the Z_q product)
  }
  if (p.r8) ensure_R8(h, st);
}

// mp_perturbation.rs:315 -- d <- N(0,1)^m
static void normals_stage(psfp_handle* h, hipStream_t st, const SampPlan& p, uint64_t seed, uint64_t first_index, size_t B) {
  ScopedTimer t(h, st, "k_normals");
  const NormalsFixed fx = h->structured ? NormalsFixed{h->mb, h->dD8, h->ldr * h->ld, h->ld, h->dX, h->h_const} : NormalsFixed{0, nullptr, 0, 0, nullptr, 0.0};
  hipLaunchKernelGGL(k_normals_wave, dim3((unsigned)((p.nwaves + 3) / 4)), dim3(256), 0, st, seed, first_index, h->m, B, h->nkb, p.nbj, h->dDt, h->dFail, fx, p.ncf, p.nseg);
}

// x = sqrt(Sigma_2) d   (structured: the m_bar x m_bar block L_1 d_1; rows from m_bar on already hold x_bot = h d_2)
static void product_stage(psfp_handle* h, hipStream_t st, const SampPlan& p, size_t B) {
  ScopedTimer t(h, st, "k_trmm_f64");
  const size_t row_hi = h->structured ? h->mb : h->M_pad;
  if (p.product == SampPlan::BIG) {      // k_trmm_f64_big: one workgroup per CU, accumulators in AccVGPRs
    hipLaunchKernelGGL(k_trmm_f64_big, dim3(tr_grid_size(((int)h->nbiL + 1) / 2, (int)p.nbj, p.GR, p.GC)), dim3(256), 0, st, h->dLt, h->dDt, h->dX, (int)h->nbiL, (int)p.nbj,
                       h->nkb, h->ld, p.GR, p.GC, row_hi);
    return;
  }
  auto geom = [&](int rt, int ncg, int bc) { StreamGeom g; g.ntile = ((int)((h->mL + 15) / 16) + rt - 1) / rt; g.ncg = ncg; g.ntask = g.ntile * ncg; g.bc = bc; return g; };
  auto go = [&](auto kern, const StreamGeom& g, unsigned grid, unsigned block, size_t lds) { hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, h->dLt, h->dDt, h->dX, g, h->nkb, h->ld, row_hi); };
  auto cd = [&](auto k0, auto k1) { return p.compact ? k1 : k0; };      // the chunk stream / the compact stream of the normals
  const auto wg64 = cd(k_trmm_stream_wg<TSW64_H, TSW64_NBUF, 0, 2>, k_trmm_stream_wg<TSW64_H, TSW64_NBUF, 1, 2>);
  const auto wg32 = cd(k_trmm_stream_wg32<TSW_H, TSW_NBUF, 0>, k_trmm_stream_wg32<TSW_H, TSW_NBUF, 1>);
  StreamGeom g = geom(4, p.product == SampPlan::TILES96 ? 1 : p.ncg, 0);      // the tiles: 64 rows, a workgroup per pair of tasks
  const unsigned nwg = (unsigned)((g.ntask + 1) / 2);
  if (p.product == SampPlan::TILES96) {      // two launches over one stream of six fragments: columns 0-63 on the 64 x 64 tiles, 64-95 on the 64 x 32 tiles
    g.ncf = 6;
    go(wg64, g, nwg, 512, TSW_LDS);
    g.cf_base = 4;
    go(wg32, g, nwg, 512, TSW32_LDS);
  } else if (p.product == SampPlan::TILES32) go(wg32, g, nwg, 512, TSW32_LDS);
  // column groups of 64 preimages: one workgroup of 2 x 4 waves per CU, rounds of four k-steps; several groups: those of a tile group on one XCD
  else if (p.product == SampPlan::TILES64) go(wg64, g, p.ncg > 1 ? 8 * ((nwg + 7) / 8) : nwg, 512, TSW_LDS);
  else {
    auto ts = [&](auto kern, int rt, int half) { const StreamGeom gt = geom(rt, p.ncg, p.bc); go(kern, gt, (unsigned)((gt.ntask + 2 * half - 1) / (2 * half)), 128 * half, 0); };
#define TS_GO(rt, nb, pd, half) ts(cd(k_trmm_stream<rt, nb, pd, half, 0>, k_trmm_stream<rt, nb, pd, half, 1>), rt, half)
    if (p.bc && p.RT == 2 && p.NB == 1) ts(k_trmm_stream<2, 1, 12, 2, 2>, 2, 2);
    else if (p.bc && p.NB == 1) ts(k_trmm_stream<1, 1, 8, 4, 2>, 1, 4);
    else if (p.RT == 2 && p.NB == 1) TS_GO(2, 1, 12, 2);
    else if (p.RT == 2 && p.NB == 2 && B <= 32) TS_GO(2, 2, 8, 2);
    else if (p.RT == 2 && p.NB == 2) TS_GO(2, 2, 16, 4);
    else if (p.RT == 2 && p.NB == 4) TS_GO(2, 4, 8, 4);
    else if (p.RT == 4 && p.NB == 2) TS_GO(4, 2, 10, 4);
    else if (p.RT == 1 && p.NB == 8) TS_GO(1, 8, 8, 4);
    else if (p.RT == 1 && p.NB == 4) TS_GO(1, 4, 8, 4);
    else if (p.RT == 1 && p.NB == 2) TS_GO(1, 2, 8, 4);
    else TS_GO(1, 1, 8, 4);
#undef TS_GO
  }
}

// p_i <- D_{Z,r,x_i}
static void round_stage(psfp_handle* h, hipStream_t st, const SampPlan& p, uint64_t seed, uint64_t first_index, size_t B) {
  const size_t ld = h->ld, m = h->m;
  if (p.tail) {      // and every 16-row tile's share of A p
    ScopedTimer t(h, st, "k_round+A p");
    StreamGeom g;
    g.ntile = p.tail_ntask; g.ncg = 1; g.ntask = p.tail_ntask; g.bc = p.bc;
    const StreamFuse fz{seed, first_index, m, h->szR, h->dP, ld, h->dA32T, h->n, h->q, h->dPartF, h->dFail};
    hipLaunchKernelGGL(p.tail_rt == 1 ? k_round_syndrome_small<1> : k_round_syndrome_small<2>, dim3((unsigned)((g.ntask + 3) / 4)), dim3(256), 0, st, h->dX, ld,
                       h->structured ? h->mb : h->M_pad, g, fz);
    return;
  }
  ScopedTimer t(h, st, "k_perturb_round");
  const dim3 grid((unsigned)((p.rwaves + 3) / 4));
  switch (p.round) {
    case SampPlan::ROUND_TAB:
    case SampPlan::ROUND_TAB_ROW:
      hipLaunchKernelGGL(p.round == SampPlan::ROUND_TAB_ROW ? k_perturb_round_tab<true> : k_perturb_round_tab<false>, grid, dim3(256), (size_t)h->szR.n_int * h->szF * sizeof(uint32_t),
                         st, seed, first_index, m, B, ld, h->dX, h->szR, h->dP, h->dFail, p.seg, SzTable{h->dSzTab, h->szF, h->szR.n_int});
      break;
    case SampPlan::ROUND_LEAN:
      hipLaunchKernelGGL(k_perturb_round_lean, grid, dim3(256), 0, st, seed, first_index, m, B, ld, h->dX, h->szR, h->dP, h->dFail, p.seg);
      break;
    case SampPlan::ROUND_WAVE:
      hipLaunchKernelGGL(k_perturb_round_wave, grid, dim3(256), 0, st, seed, first_index, m, B, ld, h->dX, h->szR, h->dP, h->dFail);
      break;
  }
}

// mp_perturbation.rs:318 -- v = u - A p
static void syndrome_stage(psfp_handle* h, hipStream_t st, const SampPlan& p, size_t B, const uint64_t* d_u) {
  ScopedTimer t(h, st, "k_zq_matmul(syndrome)");
  if (p.tail)      // the tasks of the product left their shares of A p in dPartF: summed and taken from u, one wave per output
    hipLaunchKernelGGL((k_zq_combine_wave<true>), dim3((unsigned)((h->n * B + 3) / 4)), dim3(256), 0, st, ZQ_SYNDROME, h->dPartF, p.tail_ntask, h->n, h->n, (size_t)p.bc, B, h->q, d_u, h->dV, h->ld, (size_t)0);
  else launch_zq(h, st, p.syn, ZQ_SYNDROME, h->dP, h->dP8, B, d_u, h->dV, h->ld);
}

// mp_perturbation.rs:321-326 -- z <- D_{Lambda_v(G), r sqrt(b^2+1)}
static void gadget_stage(psfp_handle* h, hipStream_t st, const SampPlan& p, uint64_t seed, uint64_t first_index, size_t B) {
  const size_t ld = h->ld, nB = h->n * B;
  ScopedTimer t(h, st, "k_gadget");
  const GadgetTablesQ tq{h->dSk, h->dGso, h->dNorm2, h->dSz, h->dRng};
  auto go = [&](auto kern, dim3 grid, size_t lds, auto tables, auto... extra) {
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, seed, first_index, (uint32_t)h->n, (uint32_t)h->k, h->q, h->prm.gp.base, B, ld, h->dV, tables, h->dZlo, h->dZhi, h->dFail, extra...);
  };
  switch (p.gadget) {
    case SampPlan::G_WAVE: go(k_gadget_wave, dim3((unsigned)((nB + 3) / 4)), 0, tq); break;
    case SampPlan::G_ROW: go(p.k32 ? k_gadget_quad<2, 16> : k_gadget_quad<4, 16>, dim3((unsigned)((nB + 15) / 16)), 0, tq); break;
    case SampPlan::G_QUAD: go(p.k32 ? k_gadget_quad<8> : k_gadget_quad<16>, dim3((unsigned)((nB + 63) / 64)), 0, tq); break;
    case SampPlan::G_QUEUE:      // GQ_WAVES * gq_p problems per workgroup
      go(p.gq_p == 128 ? k_gadget_queue<true> : k_gadget_queue<false>, dim3((unsigned)((nB + (size_t)GQ_WAVES * p.gq_p - 1) / ((size_t)GQ_WAVES * p.gq_p))),
         gadget_queue_lds_bytes(h->k, p.gq_p), tq, p.gq_p);
      break;
    case SampPlan::G_LOCKSTEP:
      go(k_gadget, dim3((unsigned)((B + 255) / 256), (unsigned)h->n), gadget_lds_bytes(h->k), GadgetTables{h->dSk, h->dGso, h->dNorm2, h->dSz});
      break;
  }
}

// mp_perturbation.rs:328-335 -- e = p + [R; I] z
static void recombine_stage(psfp_handle* h, hipStream_t st, const SampPlan& p, size_t B, int64_t* d_e) {
  const size_t ld = h->ld, m = h->m;
  ScopedTimer t(h, st, "k_recombine");
  auto bottom = [&](size_t cols, int zero_top) {      // the rows from m_bar on (z itself); zero_top: also zero the top part for the split-K form
    hipLaunchKernelGGL(k_recombine_bottom, dim3((unsigned)((B + 63) / 64), (unsigned)((cols + 63) / 64)), dim3(256), 0, st, h->mb, h->w, h->dZlo, h->dZhi, ld, h->dP, B, d_e, m, zero_top);
  };
  switch (p.recombine) {
    case SampPlan::R_SMALL2:
      hipLaunchKernelGGL(by_cols(B, k_recombine_small2<1>, k_recombine_small2<2>, k_recombine_small2<4>), dim3(p.rc_wgs), dim3(512), p.rc_lds, st, h->dR2, h->ldr, h->mb, h->w,
                         h->dZlo, h->dZhi, ld, h->dP, B, d_e, m);
      break;
    case SampPlan::R_SMALL:
      hipLaunchKernelGGL(by_cols(B, k_recombine_small<1>, k_recombine_small<2>, k_recombine_small<4>), dim3(p.rc_wgs), dim3(512), p.rc_lds, st, h->dR, h->ldr, h->mb, h->w,
                         h->dZlo, h->dZhi, ld, h->dP, B, d_e, m);
      break;
    case SampPlan::R_WG: {
      bottom(h->w, 0);
      hipLaunchKernelGGL((p.nbf == 1 ? k_recombine_wg<1, 4> : p.nbf == 2 ? k_recombine_wg<2, 8> : p.nbf == 3 ? k_recombine_wg<3, 8> : k_recombine_wg<4, 8>),
                         dim3((unsigned)((h->mb + 63) / 64), (unsigned)((B + 63) / 64)), dim3(64 * (p.nbf == 1 ? 4 : 8)), RW_LDS, st, h->dR, h->ldr, h->mb, (int)(h->ldr / 128),
                         h->dZlo, h->dZhi, ld, h->dFail, h->dP, B, d_e, m);
      break;
    }
    case SampPlan::R_TILES:
      if (p.rc_big) {
        const unsigned nbx = (unsigned)((B + 255) / 256), nby = (unsigned)(h->mb_pad / 256);
        const unsigned nsup = ((nbx + 3) / 4) * ((nby + 7) / 8);                 // super-tiles of 4 x 8 tiles, dealt to the XCDs in rounds of eight
        hipLaunchKernelGGL(k_recombine_mfma_big, dim3(((nsup + 7) / 8) * 8 * 32), dim3(512), RCB_LDS, st, h->dR8, 1, h->ldr, h->mb,
                           (int)(h->ldr / 128), h->dZlo, ld, h->dFail, h->dP, B, d_e, m, nbx, nby);
      }
      bottom(p.rsplits > 1 && h->mb > h->w ? h->mb : h->w, p.rsplits > 1 ? 1 : 0);
      hipLaunchKernelGGL(k_recombine_mfma, dim3((unsigned)((B + 127) / 128), (unsigned)((h->mb + 127) / 128), (unsigned)p.rsplits), dim3(256), RC_LDS, st, h->dR,
                         h->ldr, h->mb, (int)(h->ldr / 64), h->dZlo, h->dZhi, ld, h->dFail, h->dP, B, d_e, m, p.rc_big ? 1 : 0, p.kps);
      break;
  }
}

// One samp_p pass over B rows (mp_perturbation.rs:304-336), everything in order on the caller's stream.
static psf_status run_samp_p(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* d_u, int64_t* d_e, hipStream_t st, const SampCall& call) {
  if (!call.keep_fail) hipMemsetAsync(h->dFail, 0, 4 * sizeof(int), st);      // [0] sampler failure, [1] some |z| > 127, [2] some |p| >= 2^15 (third digit plane of the syndrome product in use)
  psf_status gate_rc = PSF_OK;
  auto u_gate = [&]() { if (call.before_u) gate_rc = (*call.before_u)(); };      // (once: each branch below passes it once)
  SampPlan p = plan_samp_p(h, B, call);
  if (!p.one_launch) prepare_samp_p(h, st, p);
  plan_fields(p, h->last_plan);      // as it runs: prepare_samp_p has had its say on the fused tail
  h->has_last_plan = true;
  if (p.one_launch) {
    u_gate();
    if (gate_rc != PSF_OK) return gate_rc;
    ScopedTimer t(h, st, "k_samp_p_small");
    hipLaunchKernelGGL(k_samp_p_small, dim3((unsigned)B), dim3(FS_THREADS), 0, st, seed, first_index, (uint32_t)h->n, (uint32_t)h->k, (uint32_t)h->mb, h->q, h->two64,
                       h->prm.gp.base, h->dLt, h->dA, h->dR, h->ldr, h->szR, GadgetTablesQ{h->dSk, h->dGso, h->dNorm2, h->dSz, h->dRng}, d_u, d_e, h->dFail);
  } else {
    h->normals_ncf = p.ncf;
    normals_stage(h, st, p, seed, first_index, B);
    product_stage(h, st, p, B);
    if (h->structured) {  // x_top -= g R d_2 (exact integer sum on the int8 matrix cores)
      ScopedTimer t(h, st, "k_rd2_mfma");
      hipLaunchKernelGGL(k_rd2_mfma, dim3((unsigned)(h->ld / 64), (unsigned)(round_up(h->mb, 64) / 64)), dim3(256), 3 * (1 + kFixPlanes) * 4096, st, h->dR8, h->ldr, h->dD8,
                         h->ldr * h->ld, h->ld, h->mb, h->g_const, h->dX);
    }
    round_stage(h, st, p, seed, first_index, B);
    u_gate();                                                      // (host path: u reaches the device now)
    syndrome_stage(h, st, p, B, d_u);
    gadget_stage(h, st, p, seed, first_index, B);
    recombine_stage(h, st, p, B, d_e);
  }
  HIP_TRY(hipGetLastError());
  if (gate_rc != PSF_OK) return gate_rc;
  h->last_stream = st;
  if (call.launched && h->multi_launched_ms < 0.0)
    h->multi_launched_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - *call.launched).count();
  return PSF_OK;
}

psf_status psfp_last_status(psfp_handle* h) {
  if (!h) return PSF_ERR_PARAM;
  HIP_TRY(hipStreamSynchronize(h->last_stream));
  int f = 0;
  HIP_TRY(hipMemcpy(&f, h->dFail, sizeof(int), hipMemcpyDeviceToHost));
  return f ? PSF_ERR_SAMPLER : PSF_OK;
}

psf_status psfp_samp_p_dev(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* d_u, int64_t* d_e, void* stream) {
  if (!h || (B && (!d_u || !d_e))) return PSF_ERR_PARAM;
  if (!h->has_key || !h->has_pub) return PSF_ERR_NO_KEY;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  psf_status rc = ensure_batch(h, B);
  if (rc != PSF_OK) return rc;
  if (h->timing) h->slots.clear();       // once per public call: the slices of a host-pointer call add up in psfp_get_timing
  return run_samp_p(h, seed, first_index, B, d_u, d_e, (hipStream_t)stream, SampCall{});
}

// `count` independent psfp_samp_p_dev calls in one submission, in order on the caller's stream (include/psf_mi355x.h).  No second lane: at large batches the FP64
// product holds every SIMD and nothing issues beside it (profiles/r03_probe_coissue.log).  The failure word of every batch is kept (SampCall::keep_fail, as the slices of a
// host-pointer call do); the gates of the later stages ([1..3]) are cleared in front of each batch as a single call clears them.
psf_status psfp_samp_p_dev_many(psfp_handle* h, size_t count, const uint64_t* seeds, const uint64_t* first_indices, size_t B, const uint64_t* d_u, int64_t* d_e, void* stream) {
  if (!h || (count && B && (!seeds || !first_indices || !d_u || !d_e))) return PSF_ERR_PARAM;
  if (!h->has_key || !h->has_pub) return PSF_ERR_NO_KEY;
  if (count == 0 || B == 0) return PSF_OK;
  if (count == 1) return psfp_samp_p_dev(h, seeds[0], first_indices[0], B, d_u, d_e, stream);
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  psf_status rc = ensure_batch(h, B);
  if (rc != PSF_OK) return rc;
  if (h->timing) h->slots.clear();
  hipStream_t st = (hipStream_t)stream;
  SampCall call;
  for (size_t i = 0; i < count && rc == PSF_OK; ++i) {
    if (i > 0) {
      call.keep_fail = true;
      HIP_TRY(hipMemsetAsync(h->dFail + 1, 0, 3 * sizeof(int), st));
    }
    rc = run_samp_p(h, seeds[i], first_indices[i], B, d_u + i * B * h->n, d_e + i * B * h->m, st, call);
  }
  return rc;
}

// ---- host-pointer entry points (the transport: psf_hostpipe.hpp) ----------------------------------------------------------------------------
// what hp_async is told about this handle; B: the rows of the call
static HostCall host_call(psfp_handle* h, size_t B, const int* extra_flags, bool defer_u, bool cut_tail, bool whole_batch) {
  return HostCall{h->prm.device, h->n, h->m, h->dFail, &h->dE, extra_flags, B > h->Bcap, defer_u, cut_tail, whole_batch};
}
// its resize step: the batch buffers for B rows; the timing slots of the call before go (once per public call: the slices of a host-pointer call add up in psfp_get_timing)
static psf_status host_resize(psfp_handle* h, size_t B) {
  const psf_status rc = ensure_batch(h, B);
  if (rc == PSF_OK && h->timing) h->slots.clear();
  return rc;
}

// psfp_samp_p_async behind its checks; cut_tail: see HostCall.  Each slice is a pass of its own that keeps the call's failure words (cleared once, in front of the first).
static psf_status samp_p_host_async(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e, bool cut_tail, const SampCall& call) {
  const psf_status rc = hp_async(h->hp, host_call(h, B, nullptr, true, cut_tail, call.whole_batch), B, u, e, [&]() { return host_resize(h, B); },
                                 [&](size_t off, size_t cnt, const uint64_t* d_u, int64_t* d_e, hipStream_t cs, const HostStage* before_u) -> psf_status {
    SampCall slice = call;
    slice.keep_fail = true;
    slice.before_u = before_u;
    return run_samp_p(h, seed, first_index + off, cnt, d_u, d_e, cs, slice);
  });
  if (rc == PSF_OK) h->last_stream = h->hp.compute;
  return rc;
}

psf_status psfp_samp_p_async(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e) {
  if (!h || (B && (!u || !e))) return PSF_ERR_PARAM;
  if (!h->has_key || !h->has_pub) return PSF_ERR_NO_KEY;
  if (B == 0) return PSF_OK;
  return samp_p_host_async(h, seed, first_index, B, u, e, false, SampCall{});
}

// all asynchronous calls of this handle have completed: their rows are in the callers' buffers; the first non-OK status (oldest call first)
psf_status psfp_wait(psfp_handle* h) {
  if (!h) return PSF_ERR_PARAM;
  HIP_TRY(hipSetDevice(h->prm.device));
  return hp_wait(h->hp);
}

// the ticket the next asynchronous call of this handle will carry, and the status of ONE asynchronous call by its ticket (hp_wait_ticket): psfp_wait returns the
// first failure of everything outstanding and thereby consumes the statuses of calls the caller may not be asking about -- a caller that keeps several batches
// (the shim's PendingBatch) asks per ticket.
uint64_t psfp_async_next_ticket(const psfp_handle* h) { return h ? h->hp.seq : 0; }
psf_status psfp_wait_ticket(psfp_handle* h, uint64_t ticket) {
  if (!h) return PSF_ERR_PARAM;
  HIP_TRY(hipSetDevice(h->prm.device));
  return hp_wait_ticket(h->hp, ticket);
}

// psfp_samp_p, psfp_samp_p_stages and psfp_samp_p_multi behind their own checks
static psf_status samp_p_host(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e, const SampCall& call) {
  if (!h || (B && (!u || !e))) return PSF_ERR_PARAM;
  if (!h->has_key || !h->has_pub) return PSF_ERR_NO_KEY;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  if (B * h->m < ((size_t)1 << 20) || call.whole_batch) {
    // a single call / a handful of preimages (or a stage export): nothing to overlap -- straight through on the default stream
    psf_status rc = psfp_wait(h);
    if (rc != PSF_OK) return rc;
    rc = ensure_batch(h, B);
    if (rc != PSF_OK) return rc;
    if (!call.whole_batch && B * (h->n + h->m) * 8 <= SIO_MAX_BYTES && !psf_exp_env("PSF_HOST_STRAIGHT")) {
      if (h->timing) h->slots.clear();
      int fl[1] = {0};
      rc = sio_call(h->hp, B * h->n, B * h->m, u, e, h->dU, h->dE, h->dFail, nullptr, 0, fl,
                    [&]() { return run_samp_p(h, seed, first_index, B, h->dU, h->dE, nullptr, call); });
      if (rc != PSF_OK) return rc;
      return fl[0] ? PSF_ERR_SAMPLER : PSF_OK;
    }
    HIP_TRY(hipMemcpy(h->dU, u, B * h->n * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (h->timing) h->slots.clear();
    rc = run_samp_p(h, seed, first_index, B, h->dU, h->dE, nullptr, call);
    if (rc != PSF_OK) return rc;
    rc = psfp_last_status(h);
    HIP_TRY(hipMemcpy(e, h->dE, B * h->m * sizeof(int64_t), hipMemcpyDeviceToHost));
    return rc;
  }
  const psf_status rc = samp_p_host_async(h, seed, first_index, B, u, e, true, call);      // a short last slice: single-call latency
  const psf_status rw = psfp_wait(h);
  return rc != PSF_OK ? rc : rw;
}

psf_status psfp_samp_p(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e) {
  return samp_p_host(h, seed, first_index, B, u, e, SampCall{});
}

// One job over several handles (one per GPU of the node, each with the same key): rows are cut into contiguous shares
// (psf_shard_range), share i is computed by handles[i] on its own device and stream; row b draws from the global index first_index + b,
// so the result equals the single-handle one bit for bit.  Host buffers; no collective is involved -- the "gather" of SURVEY.md 8e is
// each device's copy into its slice of e.
// Concurrency: ONE WORKER THREAD PER HANDLE.  The caller's u / e are pageable memory, and HIP's "asynchronous" copies to or from pageable
// memory block the calling host thread until the device has drained -- issued from one thread (round 2) the devices ran one after another.
// Each worker owns its device for the call: upload, the samp_p launch sequence, download (through the handle's own slicing, so the rows of
// the first half cross PCIe while the second half is computed), status.  A failure on one device does not leave work of another in flight:
// every worker runs to completion and synchronises its own stream before the call returns; the first non-OK status in handle order is returned.
// Per handle the call records, relative to its own start (host clock, ms): when the worker had enqueued its first samp_p launch sequence and when its
// last byte had landed in e -- psfp_get_multi_timing; overlap between the handles' [launched, done] windows is what a test can assert even with
// every handle on one GPU.
psf_status psfp_samp_p_multi(psfp_handle* const* handles, int count, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e) {
  if (!handles || count < 1 || (B && (!u || !e))) return PSF_ERR_PARAM;
  for (int i = 0; i < count; ++i) {
    if (!handles[i]) return PSF_ERR_PARAM;
    if (!handles[i]->has_key || !handles[i]->has_pub) return PSF_ERR_NO_KEY;
    if (handles[i]->n != handles[0]->n || handles[i]->m != handles[0]->m || handles[i]->q != handles[0]->q) return PSF_ERR_PARAM;
    for (int j = 0; j < i; ++j) if (handles[j] == handles[i]) return PSF_ERR_PARAM;      // one worker per handle: a handle may appear once
  }
  if (B == 0) return PSF_OK;
  std::vector<size_t> first(count), cnt(count);
  for (int i = 0; i < count; ++i) psf_shard_range(B, count, i, &first[i], &cnt[i]);
  std::vector<psf_status> rc(count, PSF_OK);
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(t - t0).count(); };
  auto work = [&](int i) {
    psfp_handle* h = handles[i];
    h->multi_launched_ms = h->multi_done_ms = -1.0;
    if (!cnt[i]) return;
    SampCall call;
    call.launched = &t0;
    rc[i] = samp_p_host(h, seed, first_index + first[i], cnt[i], u + first[i] * h->n, e + first[i] * h->m, call);
    h->multi_done_ms = ms_since(std::chrono::steady_clock::now());
  };
  std::vector<std::thread> pool;
  int started = 1;
  try {                                                  // nothing may unwind across the extern "C" boundary
    pool.reserve(count > 1 ? count - 1 : 0);
    for (int i = 1; i < count; ++i) { pool.emplace_back(work, i); started = i + 1; }
  } catch (...) {
    for (int i = started; i < count; ++i) rc[i] = PSF_ERR_HIP;      // these shares were never started (no thread available)
  }
  work(0);                                               // the calling thread serves the first handle
  for (auto& t : pool) t.join();
  for (int i = 0; i < count; ++i) if (rc[i] != PSF_OK) return rc[i];
  return PSF_OK;
}

// [launched, done] window of this handle inside the last psfp_samp_p_multi call, in ms since that call began (-1: the handle had no rows)
psf_status psfp_get_multi_timing(const psfp_handle* h, double* launched_ms, double* done_ms) {
  if (!h) return PSF_ERR_PARAM;
  if (launched_ms) *launched_ms = h->multi_launched_ms;
  if (done_ms) *done_ms = h->multi_done_ms;
  return PSF_OK;
}

psf_status psfp_samp_p_stages(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, double* d, double* x,
                              int64_t* p, uint64_t* v, int64_t* z, int64_t* e) {
  if (!h || !u || B == 0) return PSF_ERR_PARAM;
  std::vector<int64_t> etmp(B * h->m);
  SampCall call;
  call.whole_batch = true;
  psf_status rc = samp_p_host(h, seed, first_index, B, u, etmp.data(), call);
  if (rc != PSF_OK && rc != PSF_ERR_SAMPLER) return rc;
  const size_t m = h->m, ld = h->ld;
  if (e) std::memcpy(e, etmp.data(), etmp.size() * sizeof(int64_t));
  DevBuf tbuf;
  HIP_TRY(tbuf.alloc(B * m * sizeof(double)));
  void* tmp = tbuf.as<void>();
  if (d) {
    hipLaunchKernelGGL(k_export_normals, dim3(grid_for(B * m)), dim3(256), 0, 0, h->dDt, m, B, h->nkb, (double*)tmp, h->normals_ncf);
    HIP_TRY(hipMemcpy(d, tmp, B * m * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (x) {
    hipLaunchKernelGGL((k_export_T<double>), dim3(grid_for(B * m)), dim3(256), 0, 0, h->dX, m, B, ld, (double*)tmp);
    HIP_TRY(hipMemcpy(x, tmp, B * m * sizeof(double), hipMemcpyDeviceToHost));
  }
  std::vector<int64_t> ptmp;
  if (p || z) {
    ptmp.resize(B * m);
    hipLaunchKernelGGL(k_export_P, dim3(grid_for(B * m)), dim3(256), 0, 0, h->dP, m, B, ld, (int64_t*)tmp);
    HIP_TRY(hipMemcpy(ptmp.data(), tmp, B * m * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (p) std::memcpy(p, ptmp.data(), ptmp.size() * sizeof(int64_t));
  }
  if (v) {
    hipLaunchKernelGGL((k_export_T<uint64_t>), dim3(grid_for(B * h->n)), dim3(256), 0, 0, h->dV, h->n, B, ld, (uint64_t*)tmp);
    HIP_TRY(hipMemcpy(v, tmp, B * h->n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  if (z)  // e_bottom = p_bottom + z  (mp_perturbation.rs:335 with the identity block of [R; I])
    for (size_t b = 0; b < B; ++b)
      for (size_t c = 0; c < h->w; ++c) z[b * h->w + c] = etmp[b * m + h->mb + c] - ptmp[b * m + h->mb + c];
  return rc;
}

psf_status psfp_samp_d_dev(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, int64_t* d_e, void* stream) {
  if (!h || (B && !d_e)) return PSF_ERR_PARAM;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(h->dFail, 0, sizeof(int), st);
  hipLaunchKernelGGL(k_samp_d, dim3(grid_for(B * h->m, 256, 256 * 32)), dim3(256), 0, st, seed, first_index, h->m, B, h->szSR, d_e, h->dFail);
  HIP_TRY(hipGetLastError());
  h->last_stream = st;
  return PSF_OK;
}

psf_status psfp_samp_d(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, int64_t* e) {
  if (!h || (B && !e)) return PSF_ERR_PARAM;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  DevBuf de;
  HIP_TRY(de.alloc(B * h->m * sizeof(int64_t)));
  psf_status rc = psfp_samp_d_dev(h, seed, first_index, B, de.as<int64_t>(), nullptr);
  if (rc == PSF_OK) rc = psfp_last_status(h);
  HIP_TRY(de.download(e, B * h->m * sizeof(int64_t)));
  return rc;
}

static NormBound domain_bound(const psfp_handle* h) { return h->dom; }   // floor(s^2 * m * r^2), mp_perturbation.rs:401 (r = 1 under PSFGPV / PSFGPVRing)

psf_status psfp_check_domain(psfp_handle* h, size_t B, const int64_t* e, size_t len, uint8_t* ok) {
  if (!h || (B && (!e || !ok))) return PSF_ERR_PARAM;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  if (len == 0) { std::memset(ok, 0, B); return PSF_OK; }
  DevBuf de, dok;
  HIP_TRY(de.alloc(B * len * sizeof(int64_t)));
  HIP_TRY(dok.alloc(B));
  HIP_TRY(de.upload(e, B * len * sizeof(int64_t)));
  hipLaunchKernelGGL(k_check_domain, dim3((unsigned)B), dim3(256), 0, 0, de.as<int64_t>(), len, h->m, domain_bound(h), dok.as<uint8_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(dok.download(ok, B));
  return PSF_OK;
}

psf_status psfp_f_a_dev(psfp_handle* h, size_t B, const int64_t* d_e, uint64_t* d_u, uint8_t* d_ok, void* stream) {
  if (!h || (B && (!d_e || !d_u || !d_ok))) return PSF_ERR_PARAM;
  if (!h->has_pub) return PSF_ERR_NO_KEY;                     // f_a needs the public matrix only (mp_perturbation.rs:366-369)
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  PSFP_QUIESCE(h);
  psf_status rc = ensure_batch(h, B);
  if (rc != PSF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t m = h->m, ld = h->ld;
  hipLaunchKernelGGL(k_check_domain, dim3((unsigned)B), dim3(256), 0, st, d_e, m, m, domain_bound(h), d_ok);   // :367
  hipLaunchKernelGGL(k_narrow_transpose, dim3((unsigned)(ld / 64), (unsigned)((m + 63) / 64)), dim3(256), 0, st, d_e, m, B, ld, h->dPf, d_ok);
  launch_zq(h, st, plan_zq(h, B, false), ZQ_FA, h->dPf, h->dP8f, B, nullptr, d_u, h->n);                                                  // :368
  HIP_TRY(hipGetLastError());
  h->last_stream = st;
  return PSF_OK;
}

psf_status psfp_f_a(psfp_handle* h, size_t B, const int64_t* e, uint64_t* u) {
  if (!h || (B && (!e || !u))) return PSF_ERR_PARAM;
  if (!h->has_pub) return PSF_ERR_NO_KEY;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  { const psf_status rw = psfp_wait(h); if (rw != PSF_OK) return rw; }      // the handle's dU / dE may belong to an asynchronous samp_p in flight
  psf_status rc = ensure_batch(h, B);
  if (rc != PSF_OK) return rc;
  HIP_TRY(hipMemcpy(h->dE, e, B * h->m * sizeof(int64_t), hipMemcpyHostToDevice));
  rc = psfp_f_a_dev(h, B, h->dE, h->dU, h->dOk, nullptr);
  if (rc != PSF_OK) return rc;
  std::vector<uint8_t> ok(B);
  HIP_TRY(hipMemcpy(u, h->dU, B * h->n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ok.data(), h->dOk, B, hipMemcpyDeviceToHost));
  for (uint8_t o : ok) if (!o) return PSF_ERR_DOMAIN;
  return PSF_OK;
}

psf_status psfp_uniform_targets_dev(psfp_handle* h, uint64_t seed, uint64_t first_index, size_t B, uint64_t* d_u, void* stream) {
  if (!h || (B && !d_u)) return PSF_ERR_PARAM;
  if (B == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(h->prm.device));
  hipLaunchKernelGGL(k_uniform_targets, dim3(grid_for(B * h->n)), dim3(256), 0, (hipStream_t)stream, seed, first_index, h->n, B, h->q, d_u);
  HIP_TRY(hipGetLastError());
  h->last_stream = (hipStream_t)stream;
  return PSF_OK;
}

psf_status psf_narrow_rows_dev(const int64_t* d_src, int32_t* d_dst, size_t count, int* d_overflow, int device, void* stream) {
  if (count && (!d_src || !d_dst || !d_overflow)) return PSF_ERR_PARAM;
  if (((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 7)) return PSF_ERR_PARAM;
  if (count == 0) return PSF_OK;
  HIP_TRY(hipSetDevice(device));
  launch_narrow_rows((hipStream_t)stream, d_src, d_dst, count, d_overflow);
  HIP_TRY(hipGetLastError());
  return PSF_OK;
}

// The plan a samp_p pass over B preimages would take on this handle as it stands: plan_samp_p behind what ensure_batch would derive from B.  Nothing is
// launched, allocated or changed; the compact key copies count as present only once a call has found them complete (small_state), as for the call itself.
psf_status psfp_query_plan(const psfp_handle* h, size_t B, int* fields, size_t count) {
  if (!h || !fields || B == 0 || count < PSFP_PLAN_FIELDS) return PSF_ERR_PARAM;
  if (!h->has_key || !h->has_pub) return PSF_ERR_NO_KEY;
  BatchDims bd;
  bd.nbj = round_up(B, TR_BN) / TR_BN;
  bd.zq_split_cap = B <= h->Bcap ? h->zq_split_cap : zq_split_cap_for(h, round_up(B, TR_BN));
  plan_fields(plan_samp_p(h, B, SampCall{}, &bd), fields);
  return PSF_OK;
}

// The plan of the last samp_p pass this handle ran (a host-pointer call above 2^20 coordinates runs in slices: the last slice's)
psf_status psfp_get_last_plan(const psfp_handle* h, int* fields, size_t count) {
  if (!h || !fields || count < PSFP_PLAN_FIELDS) return PSF_ERR_PARAM;
  if (!h->has_last_plan) return PSF_ERR_NO_KEY;
  std::memcpy(fields, h->last_plan, sizeof(h->last_plan));
  return PSF_OK;
}

psf_status psfp_enable_timing(psfp_handle* h, int on) {
  if (!h) return PSF_ERR_PARAM;
  h->timing = on != 0;
  if (!on) h->slots.clear();
  return PSF_OK;
}

psf_status psfp_get_timing(psfp_handle* h, char* names, size_t names_len, double* ms, size_t* count) {
  if (!h || !count) return PSF_ERR_PARAM;
  HIP_TRY(hipStreamSynchronize(h->last_stream));
  std::string joined;
  std::vector<std::string> names_v;
  std::vector<double> sums;
  for (auto& s : h->slots) {          // launches of the same kernel (one per slice) are summed
    float t = 0.f;
    if (hipEventElapsedTime(&t, s.e0, s.e1) != hipSuccess) continue;
    size_t j = 0;
    while (j < names_v.size() && names_v[j] != s.name) ++j;
    if (j == names_v.size()) { names_v.push_back(s.name); sums.push_back(0.0); }
    sums[j] += t;
  }
  size_t nout = 0;
  for (size_t j = 0; j < names_v.size(); ++j) {
    if (ms && nout < *count) ms[nout] = sums[j];
    if (!joined.empty()) joined += ';';
    joined += names_v[j];
    ++nout;
  }
  if (names && names_len) { std::strncpy(names, joined.c_str(), names_len - 1); names[names_len - 1] = 0; }
  *count = nout;
  return PSF_OK;
}

}  // extern "C"

#include "psfgpv_impl.hpp"
