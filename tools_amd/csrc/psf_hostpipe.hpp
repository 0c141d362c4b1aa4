// psf_hostpipe.hpp -- the host-pointer transport of the three PSF types: how targets reach the device and rows reach the caller's int64 buffers.
//   small calls (u + e <= SIO_MAX_BYTES):      one pinned buffer, kernels in stream order, one synchronisation             sio_call
//   nearest-plane batches (PSFGPV / ring):     int32 narrowing, NT piece copies with an event each, threaded widening      sio_batch
//   asynchronous calls, two in flight:         slices, int32 narrowing, chunk copies by the DMA engines, widening workers  hp_async, hp_wait, hp_wait_ticket
// The transport knows no handle: what it needs from one arrives as arguments (HostCall, the compute and resize callbacks).  Its host arithmetic -- slice cuts,
// chunk geometry, the pieces, widen_rows -- is psf_hostpipe_host.hpp, which a CPU program sweeps under the sanitizers.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#include "psf_hip_util.hpp"
#include "psf_host.hpp"
#include "psf_kernels.hpp"
#include "psf_sdma.hpp"
#include "psf_hostpipe_host.hpp"

namespace psf {

// Host-pointer calls: rows are narrowed to int32 on the device, cross PCIe in chunks into pinned buffers and are widened into the caller's int64 rows by worker
// threads, while the compute stream already runs the next slice / the next call.
struct HostPipe {
  static constexpr int NW = 8;                // at most this many worker threads per call (each: its own pinned chunk buffers, copies + widening of chunks c = w mod nw)
  int nw = 4;                                 // workers in use (PSF_HOST_WORKERS)
  DevArr<int32_t> dE32[2];                    // device: narrowed rows of the call in flight, two calls deep (grown to the call's entries)
  bool slot_ready[2] = {false, false};        // the slot's flags, events, pinned chunk buffers and signals exist
  bool common_ready = false;                  // streams, overflow word, transport
  PinArr<int32_t> hbuf[2][NW][2];             // pinned chunk buffers [call slot][worker][double buffer]: two calls in flight never share one
  Event evC[2][NW][2];                        // chunk landed in its pinned buffer
  size_t chunk_entries = 0;
  Event evSlice[2][4];                        // slice j of call slot s has been narrowed (compute stream)
  PinArr<int> hFlags[2];                      // pinned: [0] sampler failure, [1] unused, [2] int32 overflow of a row entry
  DevArr<int> dOvf;                           // device: overflow flag of the narrowing kernel
  PinArr<uint64_t> hU[2];                     // pinned staging of the targets (a copy from pageable memory would block the caller behind the stream)
  DevArr<uint64_t> dU2[2];                    // device copy of the targets per call in flight (filled by k_copy_words at the head of the call); grown with hU
  std::vector<std::thread> workers[2];
  bool busy[2] = {false, false};
  std::atomic<int> status[2] = {{0}, {0}};     // psf_status of the call in each slot (written by its workers)
  size_t next = 0;                            // slot of the next asynchronous call
  uint64_t seq = 0;                           // ticket of the next asynchronous call (0, 1, 2, ... since the handle was created)
  uint64_t slot_seq[2] = {0, 0};              // ticket of the call in each slot
  struct Done { uint64_t seq; int status; bool used; } done[8] = {};      // the last joined calls and their statuses (hp_wait_ticket)
  int copy_mode = 1;                          // how a chunk crosses PCIe: 1 = SDMA engine through the HSA runtime (psf_sdma.hpp), 0 = hipMemcpyAsync (PSF_HOST_COPY)
  SdmaCopy sdma;
  hsa_signal_t sigC[2][NW][2] = {};           // mode 1: chunk landed in its pinned buffer (HSA signals: dropped by the destructor, in front of sdma.close())
  hsa_signal_t sigU = {};                     // mode 1: the call's targets have reached the device
  Stream copy;                                // D2H stream (high priority)
  Stream compute;                             // stream of the asynchronous calls' kernels (normal priority)
  std::thread hp_warm;                        // the prewarm worker (hp_ensure beside a key's factorisation); joined by whoever touches the transport next
  // small host-pointer calls (one preimage is the reference's call): u, e and the flags travel through ONE pinned buffer by kernels in stream order, one
  // synchronisation per call -- the straight form (hipMemcpy in, flags out twice, hipMemcpy out: five blocking runtime calls) cost ~70 us around 47 us of kernels
  PinArr<uint8_t> sio_pin;
  DevArr<uint64_t> sio_du; DevArr<int64_t> sio_de;            // device side for handles without their own (PSFGPV / ring)
  DevArr<int32_t> sio_d32;                                    // narrowed rows of a PSFGPV / ring batch on their way to the host
  Event sio_ev[5];                                            // pieces 0..3 of such a batch have landed; [4]: its flags have
  void quiesce();                             // joins the prewarm worker and the workers of both call slots: in front of every release of what their calls read
  ~HostPipe();
};

constexpr size_t SIO_MAX_BYTES = (size_t)1 << 20;           // calls whose u + e fit this take the one-buffer form (at 4 MB the runtime's copies are faster again: 1.27 vs 1.17 ms at C3, 16 preimages)

// (C linkage: the names these three kernels have always had in the library's code object)
extern "C" {
// flags of a small call into the pinned buffer: [0] = a[0] (the failure word psfp_last_status reads), [1 ..] = c[0 .. nc)
__global__ void k_sio_flags(const int* __restrict__ a, const int* __restrict__ c, int nc, int* __restrict__ out) {
  const int t = threadIdx.x;
  if (t == 0) out[0] = a[0];
  if (t >= 1 && t <= nc) out[t] = c[t - 1];
}
// The flags of an asynchronous call: cleared and sent to pinned host memory by one-wave kernels in stream order.  (hipMemsetAsync / hipMemcpyAsync on the
// compute stream go through the runtime's copy path, where they queue behind the chunk copies of the call before: the next call's kernels then waited for them.)
__global__ void k_host_flags_clear(int* __restrict__ fail, int* __restrict__ ovf) { if (threadIdx.x < 4) fail[threadIdx.x] = 0; if (threadIdx.x < 2) ovf[threadIdx.x] = 0; }
// extra: the eight flag words of a PSFGPV / PSFGPVRing call (psfgpv_impl.hpp: [0] and [4] = a sampler failure of the first / second pass), or nullptr
__global__ void k_host_flags_send(const int* __restrict__ fail, const int* __restrict__ ovf, const int* __restrict__ extra, int* __restrict__ host_flags) {
  if (threadIdx.x == 0) {
    host_flags[0] = fail[0] | (extra ? (extra[0] | extra[4]) : 0);
    host_flags[1] = fail[1]; host_flags[2] = ovf[0]; host_flags[3] = extra ? 1 : 0;        // [3]: a nearest-plane call (an overflow of the narrowing is not a sampler failure there)
    __threadfence_system();
  }
}
}  // extern "C"

// k_narrow_rows over `count` entries on `st`, a pair of entries per lane
static inline void launch_narrow_rows(hipStream_t st, const int64_t* src, int32_t* dst, size_t count, int* ovf) {
  const size_t g = (count / 2 + 1 + 255) / 256;
  hipLaunchKernelGGL(k_narrow_rows, dim3((unsigned)(g > 256 * 16 ? 256 * 16 : g)), dim3(256), 0, st, src, dst, count, ovf);
}

static psf_status sio_ensure(HostPipe& hp, size_t bytes) {
  if (bytes <= hp.sio_pin.cap()) return PSF_OK;
  HIP_TRY(hp.sio_pin.alloc(round_up(bytes, (size_t)64 << 10)));
  return PSF_OK;
}
// device targets and rows for a handle without its own (PSFGPV / ring): hp.sio_du, hp.sio_de
static psf_status sio_dev_rows(HostPipe& hp, size_t nu, size_t ne) {
  HIP_TRY(hp.sio_du.grow(nu));
  HIP_TRY(hp.sio_de.grow(ne));
  return PSF_OK;
}
static inline unsigned sio_grid(size_t words) { const size_t g = (words / 2 + 255) / 256; return (unsigned)(g < 1 ? 1 : g > 64 ? 64 : g); }
// u -> pinned -> d_u (kernel); [the caller's launches]; d_e -> pinned, flags -> pinned (kernels); one synchronisation; pinned -> e.  `flags_out` receives
// 1 + nc ints.  `run` enqueues the call on the null stream and returns its status.
static psf_status sio_call(HostPipe& hp, size_t nu, size_t ne, const uint64_t* u, int64_t* e, uint64_t* d_u, int64_t* d_e, const int* fa, const int* fc, int nc,
                           int* flags_out, const std::function<psf_status()>& run) {
  const size_t ub = round_up(nu * 8, 64), eb = round_up(ne * 8, 64);
  psf_status rc = sio_ensure(hp, ub + eb + 64);
  if (rc != PSF_OK) return rc;
  uint64_t* hu = reinterpret_cast<uint64_t*>(hp.sio_pin.get());
  int64_t* he = reinterpret_cast<int64_t*>(hp.sio_pin + ub);
  int* hf = reinterpret_cast<int*>(hp.sio_pin + ub + eb);
  std::memcpy(hu, u, nu * 8);
  hipLaunchKernelGGL(k_copy_words, dim3(sio_grid(nu)), dim3(256), 0, nullptr, hu, d_u, nu);
  rc = run();
  if (rc != PSF_OK) { hipStreamSynchronize(nullptr); return rc; }
  hipLaunchKernelGGL(k_copy_words, dim3(sio_grid(ne)), dim3(256), 0, nullptr, reinterpret_cast<const uint64_t*>(d_e), reinterpret_cast<uint64_t*>(he), ne);
  hipLaunchKernelGGL(k_sio_flags, dim3(1), dim3(64), 0, nullptr, fa, fc, nc, hf);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  for (int i = 0; i <= nc; ++i) flags_out[i] = hf[i];
  std::memcpy(e, he, ne * 8);
  return PSF_OK;
}

// A batch of a type that keeps no device rows of its own (PSFGPV / ring), as sio_call: cached device buffers (no allocation per call), u through the pinned
// buffer, `run(d_u, d_e)` on the null stream, the rows narrowed to int32 on the device (every entry of a preimage fits by far; k_narrow_rows raises a flag otherwise
// and the int64 rows are copied instead), the flags first, then the rows in NT pieces into pinned memory with an event behind each: thread i widens piece i with
// streaming stores as soon as it has landed, while the later pieces are still crossing PCIe.  The straight form (two pageable copies around two allocations) took
// 9.75 ms around 4.34 ms of kernels at C2.
static psf_status sio_batch(HostPipe& hp, int device, size_t nu, size_t ne, const uint64_t* u, int64_t* e, const int* fa, const int* fc, int nc, int* flags_out,
                            const std::function<psf_status(uint64_t*, int64_t*)>& run) {
  constexpr int NT = 4;
  psf_status rc = sio_dev_rows(hp, nu, ne);
  if (rc != PSF_OK) return rc;
  HIP_TRY(hp.sio_d32.grow(ne, 2 * sizeof(int)));
  const size_t ub = round_up(nu * 8, 64), eb = round_up(ne * 4, 64);
  rc = sio_ensure(hp, ub + eb + 64);
  if (rc != PSF_OK) return rc;
  uint64_t* hu = reinterpret_cast<uint64_t*>(hp.sio_pin.get());
  int32_t* he = reinterpret_cast<int32_t*>(hp.sio_pin + ub);
  int* hf = reinterpret_cast<int*>(hp.sio_pin + ub + eb);
  int* d_ovf = reinterpret_cast<int*>(hp.sio_d32 + ne);                    // overflow word of the narrowing, behind the rows
  std::memcpy(hu, u, nu * 8);
  hipLaunchKernelGGL(k_copy_words, dim3(sio_grid(nu)), dim3(256), 0, nullptr, hu, hp.sio_du, nu);
  HIP_TRY(hipMemsetAsync(d_ovf, 0, 2 * sizeof(int), nullptr));
  rc = run(hp.sio_du, hp.sio_de);
  if (rc != PSF_OK) { hipStreamSynchronize(nullptr); return rc; }
  launch_narrow_rows(nullptr, hp.sio_de, hp.sio_d32, ne, d_ovf);
  hipLaunchKernelGGL(k_sio_flags, dim3(1), dim3(64), 0, nullptr, fa, fc, nc, hf);
  HIP_TRY(hipMemcpyAsync(hf + 12, d_ovf, sizeof(int), hipMemcpyDeviceToHost, nullptr));
  if (!hp.sio_ev[0]) for (auto& ev : hp.sio_ev) HIP_TRY(hipEventCreateWithFlags(ev.put(), hipEventDisableTiming));
  HIP_TRY(hipEventRecord(hp.sio_ev[NT], nullptr));                       // flags and overflow word are in pinned memory
  const size_t per = host_piece_len(ne, NT);
  for (int i = 0; i < NT; ++i) {
    const HostSpan pc = host_piece((size_t)i, ne, per);
    if (pc.cnt) HIP_TRY(hipMemcpyAsync(he + pc.b0, hp.sio_d32 + pc.b0, pc.cnt * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipEventRecord(hp.sio_ev[i], nullptr));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventSynchronize(hp.sio_ev[NT]));
  if (hf[12]) {                                                            // an entry beyond 32 bits: the int64 rows, as before
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(e, hp.sio_de, ne * sizeof(int64_t), hipMemcpyDeviceToHost));
  } else {
    std::thread th[NT];
    std::atomic<int> bad{0};
    auto piece = [&, device](int i, bool set_dev) {
      const HostSpan pc = host_piece((size_t)i, ne, per);
      if (set_dev && hipSetDevice(device) != hipSuccess) { bad = 1; return; }
      if (hipEventSynchronize(hp.sio_ev[i]) != hipSuccess) { bad = 1; return; }
      if (pc.cnt) widen_rows(e + pc.b0, he + pc.b0, pc.cnt);
    };
    int started = 0;
    try {
      for (; started < NT; ++started) th[started] = std::thread(piece, started, true);
    } catch (...) { }
    for (int i = started; i < NT; ++i) piece(i, false);                   // (no thread to be had: this one does the rest)
    for (int i = 0; i < started; ++i) th[i].join();
    if (bad) return PSF_ERR_HIP;
  }
  for (int i = 0; i <= nc; ++i) flags_out[i] = hf[i];
  return PSF_OK;
}

// wait for the asynchronous call in `slot` (its workers have copied and widened every row), release it, return its status
static psf_status hp_join(HostPipe& hp, int slot) {
  if (!hp.busy[slot]) return PSF_OK;
  for (auto& t : hp.workers[slot]) if (t.joinable()) t.join();
  hp.workers[slot].clear();
  hp.busy[slot] = false;
  psf_status rc = (psf_status)hp.status[slot].load();
  if (rc == PSF_OK && hp.hFlags[slot][0]) rc = PSF_ERR_SAMPLER;
  // an entry beyond 32 bits: impossible for PSFPerturbation (every entry is checked on the device: a sampler failure); a PSFGPV / PSFGPVRing row of that size
  // needs the synchronous call, which copies 64-bit rows then
  if (rc == PSF_OK && hp.hFlags[slot][2]) rc = hp.hFlags[slot][3] ? PSF_ERR_UNSUPPORTED : PSF_ERR_SAMPLER;
  hp.done[hp.slot_seq[slot] & 7] = HostPipe::Done{hp.slot_seq[slot], (int)rc, true};      // whoever joins consumes the status: the ticket keeps it
  return rc;
}

// all asynchronous calls have completed: their rows are in the callers' buffers; the first non-OK status (oldest call first)
static psf_status hp_wait(HostPipe& hp) {
  psf_status first = PSF_OK;
  for (int i = 0; i < 2; ++i) {
    const int slot = (int)((hp.next + (size_t)i) & 1);                   // oldest first
    const psf_status rc = hp_join(hp, slot);
    if (first == PSF_OK) first = rc;
  }
  return first;
}

// the status of ONE asynchronous call by its ticket (waits for it and for the older call in flight, nothing newer).  PSF_ERR_PARAM: a ticket never issued or
// older than the last 8 joined calls.
static psf_status hp_wait_ticket(HostPipe& hp, uint64_t ticket) {
  if (ticket >= hp.seq) return PSF_ERR_PARAM;
  for (int i = 0; i < 2; ++i) {                                         // oldest first, up to the ticket's own call
    const int slot = (int)((hp.next + (size_t)i) & 1);
    if (hp.busy[slot] && hp.slot_seq[slot] <= ticket) hp_join(hp, slot);
  }
  const auto& d = hp.done[ticket & 7];
  return (d.used && d.seq == ticket) ? (psf_status)d.status : PSF_ERR_PARAM;
}

// the calls in flight are joined; nothing of the transport is read or written by another thread afterwards
inline void HostPipe::quiesce() {
  if (hp_warm.joinable()) hp_warm.join();
  for (int s = 0; s < 2; ++s) hp_join(*this, s);
}
// (the device of the handle is current)  The signals are dropped and the DMA path is closed here, in front of the members: the streams are destroyed after sdma.close()
inline HostPipe::~HostPipe() {
  quiesce();
  for (auto& slot : sigC) for (auto& wk : slot) for (auto& sg : wk) if (sg.handle) sdma.drop_signal(sg);
  if (sigU.handle) sdma.drop_signal(sigU);
  sdma.close();
}

// streams, transport and the rings of call slot `slot` (which the caller has joined) on `device`.  Everything is allocated on first use and per slot: a caller that
// only ever makes synchronous calls pays for one slot (pinning memory is the expensive part of a handle's first host-pointer call).
static psf_status hp_ensure(HostPipe& hp, int device, int slot, size_t entries, size_t u_words, bool from_prewarm = false) {
  if (!from_prewarm && hp.hp_warm.joinable()) hp.hp_warm.join();      // (the prewarm worker itself never looks at hp.hp_warm: the owner may still be assigning it)
  constexpr int NW = HostPipe::NW;
  if (!hp.common_ready) {
    {  // (matters for the HIP-copy transports only: their copies are shader kernels, which on a queue of lower priority than the compute stream ran only when
       // that stream was idle -- copies on the HIGH-priority queue, the asynchronous calls' kernels on a normal one)
      int lo_prio = 0, hi_prio = 0;
      HIP_TRY(hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
      int pc = hi_prio, pk = (lo_prio + hi_prio) / 2;
      if (const char* env = psf_exp_env("PSF_HOST_PRIO")) { if (std::atoi(env) == 0) pc = pk; else if (std::atoi(env) == 2) { pc = pk; pk = hi_prio; } }      // experiments: 0 = equal, 2 = compute high
      if (!hp.copy) HIP_TRY(hipStreamCreateWithPriority(hp.copy.put(), hipStreamNonBlocking, pc));
      if (!hp.compute) HIP_TRY(hipStreamCreateWithPriority(hp.compute.put(), hipStreamNonBlocking, pk));
    }
    if (!hp.dOvf) HIP_TRY(hp.dOvf.alloc(2));
    hp.chunk_entries = (size_t)2 << 20;                                  // 8 MiB of int32 per chunk
    if (const char* env = std::getenv("PSF_HOST_WORKERS")) { const int v = std::atoi(env); if (v >= 1 && v <= NW) hp.nw = v; }
    if (const char* env = psf_exp_env("PSF_HOST_CHUNK_MB")) { const long v = std::atol(env); if (v >= 1 && v <= 256) hp.chunk_entries = (size_t)v << 18; }
    if (const char* env = psf_exp_env("PSF_HOST_COPY")) if (std::strncmp(env, "runtime", 7) == 0) hp.copy_mode = 0;      // sdma (default) | runtime
    if (hp.copy_mode == 1) {
      int dom = 0, bus = 0, dv = 0;
      HIP_TRY(hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device));
      HIP_TRY(hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device));
      HIP_TRY(hipDeviceGetAttribute(&dv, hipDeviceAttributePciDeviceId, device));
      if (!hp.sdma.open(dom, bus, dv)) hp.copy_mode = 0;                  // no HSA agent for this device: the HIP copies (slower under overlap, same rows)
      else if (!hp.sigU.handle && !hp.sdma.make_signal(&hp.sigU)) return PSF_ERR_HIP;
    }
    hp.common_ready = true;
  }
  if (!hp.slot_ready[slot]) {                                 // (every piece behind its own test: a call that failed half-way is completed, not repeated, by the next)
    if (!hp.hFlags[slot]) HIP_TRY(hp.hFlags[slot].alloc(4));
    for (auto& ev : hp.evSlice[slot]) if (!ev) HIP_TRY(hipEventCreateWithFlags(ev.put(), hipEventDisableTiming));
    for (int w = 0; w < hp.nw; ++w)
      for (int k = 0; k < 2; ++k) {
        if (!hp.hbuf[slot][w][k]) HIP_TRY(hp.hbuf[slot][w][k].alloc(hp.chunk_entries));
        if (!hp.evC[slot][w][k]) HIP_TRY(hipEventCreateWithFlags(hp.evC[slot][w][k].put(), hipEventDisableTiming));
        if (hp.copy_mode == 1 && !hp.sigC[slot][w][k].handle && !hp.sdma.make_signal(&hp.sigC[slot][w][k])) return PSF_ERR_HIP;
      }
    hp.slot_ready[slot] = true;
  }
  HIP_TRY(hp.dE32[slot].grow(entries));
  if (u_words > hp.dU2[slot].cap()) {                         // the pair grows together: both released, then both allocated (dU2 last: its capacity stands for the pair)
    hp.hU[slot].reset(); hp.dU2[slot].reset();
    HIP_TRY(hp.hU[slot].alloc(u_words));
    HIP_TRY(hp.dU2[slot].alloc(u_words));
  }
  return PSF_OK;
}

// What an asynchronous host-pointer call brings from its handle.
struct HostCall {
  int device; size_t n, m;            // the handle's device; words of a target, entries of a row
  int* dFail;                         // the handle's four failure words
  const DevArr<int64_t>* rows;        // where the handle keeps the device rows of its batch (read after `resize`, which may move them)
  const int* extra_flags;             // see k_host_flags_send
  bool regrows;                       // `resize` will reallocate the batch buffers: nothing may be in flight then
  bool defer_u;                       // the targets are uploaded when the pipeline asks for them (PSFPerturbation: behind the product); otherwise at the head of the call
  bool cut_tail;                      // a short last slice (the synchronous form: behind an asynchronous call the next call's compute covers the transfer)
  bool whole_batch;                   // never a cut
};
// stages the call's targets: pageable -> pinned (the calling thread) -> this call's device copy.  Owned by hp_async's frame; a pass that is handed one calls it once.
using HostStage = std::function<psf_status()>;
// `compute(off, cnt, d_u, d_e, cs, before_u)` enqueues the samp_p pipeline of the rows [off, off + cnt) on the stream cs (targets d_u: cnt x n, preimages d_e:
// cnt x m, both on the device).  before_u: nullptr, or (first slice of a call with deferred targets) what it must call in front of the first stage that reads d_u.
using HpCompute = std::function<psf_status(size_t, size_t, const uint64_t*, int64_t*, hipStream_t, const HostStage*)>;

// Asynchronous samp_p on host buffers: returns once the work is enqueued (the targets have been staged); `e` is complete when hp_wait returns.
// At most two calls are in flight: a third waits for the first.  The compute stream runs the slices of the call back to back (row b draws from global
// index first_index + b, so slicing changes no bit); behind each slice its rows are narrowed to int32 (every entry of a preimage is below 2^31: |p| < 2^23
// and |R z| <= w 2^15, both checked on the device), copied in chunks to pinned memory on a second stream and widened into `e` by NW worker threads --
// while the compute stream is already in the next slice or the next call.  A single call therefore ends one short slice after its product
// (slices: all but the last ~1024 rows, then the rest), and back-to-back calls run at the device-resident rate.
// What such a call of any of the three types is made of: `compute` is the type's own; everything around it -- slots, staging of the targets, int32 narrowing,
// chunk transfers by the DMA engines, widening workers, the flags -- is the same.  `resize` fits the handle's batch buffers to B rows, between the joins and the
// first launch.
static psf_status hp_async(HostPipe& hp, const HostCall& hc, size_t B, const uint64_t* u, int64_t* e, const std::function<psf_status()>& resize, const HpCompute& compute) {
  HIP_TRY(hipSetDevice(hc.device));
  const size_t n = hc.n, m = hc.m, total = B * m;
  if (!hp.busy[0] && !hp.busy[1]) hp.next = 0;              // nothing in flight: slot 0 (a caller that only makes synchronous calls never needs -- or allocates -- the second)
  const int slot = (int)(hp.next & 1);
  psf_status rc = hp_join(hp, slot);                        // the call before last used this slot
  if (rc != PSF_OK) return rc;
  if (hc.regrows) { rc = hp_join(hp, slot ^ 1); if (rc != PSF_OK) return rc; }
  rc = resize();
  if (rc != PSF_OK) return rc;
  rc = hp_ensure(hp, hc.device, slot, total, B * n);
  if (rc != PSF_OK) return rc;
  ++hp.next;
  hp.slot_seq[slot] = hp.seq++;
  hipStream_t cs = hp.compute;
  // targets: pageable -> pinned (this thread) -> this call's device copy -- deferred until the syndrome stage of the first slice is about to be enqueued:
  // by then the product is executing, and neither the staging copy nor the upload delays the call
  const HostStage stage_u = [&hp, slot, u, B, n, cs]() -> psf_status {
    std::memcpy(hp.hU[slot], u, B * n * sizeof(uint64_t));
    if (hp.copy_mode == 1) {                                // by the DMA engine (dU2[slot]'s last reader was joined before this call began)
      if (!hp.sdma.start_upload(hp.dU2[slot], hp.hU[slot], B * n * sizeof(uint64_t), hp.sigU) || !hp.sdma.wait(hp.sigU)) return PSF_ERR_HIP;
    } else {
      hipLaunchKernelGGL(k_copy_words, dim3(64), dim3(256), 0, cs, hp.hU[slot], hp.dU2[slot], B * n);  // (see k_copy_words: a HIP copy would queue behind the download before)
    }
    return PSF_OK;
  };
  const bool deferred = hp.copy_mode == 1 && hc.defer_u;    // the copy kernel is ordered by the compute stream only: at the head of the call
  if (!deferred) {
    rc = stage_u();
    if (rc != PSF_OK) return rc;
  }
  const uint64_t* dUcall = hp.dU2[slot];
  int64_t* const dE = *hc.rows;
  size_t tail = 1024;
  if (const char* env = psf_exp_env("PSF_HOST_TAIL")) { const long v = std::atol(env); if (v >= 128) tail = (size_t)v; }
  bool cut = hc.cut_tail;
  if (const char* env = psf_exp_env("PSF_HOST_ASYNC_SLICE")) cut = cut || std::atoi(env) != 0;      // experiments: 1 = asynchronous calls cut the tail slice too
  long forced = 0;
  if (const char* env = psf_exp_env("PSF_HOST_SLICE")) forced = std::atol(env);                     // experiments: equal slices of this many rows (at most four)
  const HostSlices sl = host_slices(B, tail, cut, hc.whole_batch, forced);
  const int nsl = sl.nsl;
  hipLaunchKernelGGL(k_host_flags_clear, dim3(1), dim3(64), 0, cs, hc.dFail, hp.dOvf);
  for (int j = 0; j < nsl; ++j) {
    const size_t off = sl.cuts[j], cnt = sl.cuts[j + 1] - sl.cuts[j];
    rc = compute(off, cnt, dUcall + off * n, dE + off * m, cs, deferred && j == 0 ? &stage_u : nullptr);
    if (rc != PSF_OK) return rc;
    launch_narrow_rows(cs, dE + off * m, hp.dE32[slot] + off * m, cnt * m, hp.dOvf);
    if (j == nsl - 1) {                                     // the call's flags travel with its last slice
      hipLaunchKernelGGL(k_host_flags_send, dim3(1), dim3(64), 0, cs, hc.dFail, hp.dOvf, hc.extra_flags, hp.hFlags[slot]);
    }
    HIP_TRY(hipEventRecord(hp.evSlice[slot][j], cs));
  }
  HIP_TRY(hipGetLastError());
  // workers: chunk c of the call's entries belongs to worker c % NW; a worker copies its chunk into one of its two pinned buffers and widens the
  // previous one meanwhile
  const size_t CE = hp.chunk_entries, nchunks = host_chunks(total, CE);
  hp.status[slot] = (int)PSF_OK;
  hp.busy[slot] = true;
  const int32_t* src = hp.dE32[slot];
  const int device = hc.device;
  size_t slice_end[4]; hipEvent_t slice_ev[4];
  for (int j = 0; j < nsl; ++j) { slice_end[j] = sl.cuts[j + 1] * m; slice_ev[j] = hp.evSlice[slot][j]; }
  const int nw = hp.nw;
  int dbg = 0;
  if (const char* env = psf_exp_env("PSF_HOST_DEBUG")) dbg = std::atoi(env);      // measurement only: 1 = no widening, 2 = no copies either (e is NOT filled)
  const int copy_mode = hp.copy_mode;
  const bool plain_widen = psf_exp_env("PSF_HOST_PLAIN_WIDEN") != nullptr;      // measurement only: the scalar loop with ordinary stores
  auto worker = [&hp, slot, src, e, total, CE, nchunks, nsl, device, slice_end, slice_ev, nw, dbg, copy_mode, plain_widen](int w) {
    if (hipSetDevice(device) != hipSuccess) { hp.status[slot] = (int)PSF_ERR_HIP; return; }
    auto widen = [&](size_t c, int k) {
      if (copy_mode == 1 ? (dbg < 2 && !hp.sdma.wait(hp.sigC[slot][w][k])) : hipEventSynchronize(hp.evC[slot][w][k]) != hipSuccess) { hp.status[slot] = (int)PSF_ERR_HIP; return; }
      const HostSpan ch = host_chunk(c, total, CE);
      const int32_t* hs = hp.hbuf[slot][w][k];
      int64_t* dst = e + ch.b0;
      if (dbg) return;
      if (plain_widen) { for (size_t i = 0; i < ch.cnt; ++i) dst[i] = (int64_t)hs[i]; }
      else widen_rows(dst, hs, ch.cnt);
    };
    long prev = -1; int pk = 0, k = 0;
    for (size_t c = (size_t)w; c < nchunks; c += (size_t)nw) {
      const HostSpan ch = host_chunk(c, total, CE);
      const int j = host_chunk_slice(ch, slice_end, nsl);
      if (copy_mode == 1) {                                              // the slice's rows are complete (host wait), then the DMA engine moves the chunk
        if (hipEventSynchronize(slice_ev[j]) != hipSuccess ||
            (dbg < 2 && !hp.sdma.start(hp.hbuf[slot][w][k], src + ch.b0, ch.cnt * sizeof(int32_t), hp.sigC[slot][w][k]))) { hp.status[slot] = (int)PSF_ERR_HIP; break; }
      } else if (hipStreamWaitEvent(hp.copy, slice_ev[j], 0) != hipSuccess ||
                 (dbg < 2 ? hipMemcpyAsync(hp.hbuf[slot][w][k], src + ch.b0, ch.cnt * sizeof(int32_t), hipMemcpyDeviceToHost, hp.copy) : hipSuccess) != hipSuccess ||
                 hipEventRecord(hp.evC[slot][w][k], hp.copy) != hipSuccess) { hp.status[slot] = (int)PSF_ERR_HIP; break; }
      if (prev >= 0) widen((size_t)prev, pk);
      prev = (long)c; pk = k; k ^= 1;
    }
    if (prev >= 0) widen((size_t)prev, pk);
  };
  try {
    for (int w = 0; w < nw && (size_t)w < nchunks; ++w) hp.workers[slot].emplace_back(worker, w);
  } catch (...) {                                                        // no thread available: the started ones finish, the rest of the rows are missing
    hp.status[slot] = (int)PSF_ERR_HIP;
  }
  // (the call's flags were copied on the compute stream in front of the last slice's event, which the worker of the last chunk waits for: once the
  // workers have been joined the flags have landed)
  return PSF_OK;
}

}  // namespace psf
