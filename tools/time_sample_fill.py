#!/usr/bin/env python3
"""Rates of the sample fills on device buffers (psf_sample_cbd_dev, psf_sample_uniform_dev, psf_sample_discrete_gauss_dev).

  cbd / uniform   each beside a torch `zero_` of the same buffer (the write roof), alternating call by call: bytes written per second and
                  the ratio to the memset; the uniform rows also give Philox blocks per second (one block per coefficient and redraw).
                  CBD at eta = 2, 3, 8 in 16- and 64-bit words; uniform at q = 3329 (16 bits) and q = 2^62 - 57 (64 bits).
  gauss           s = 8 and s = 300, centre 0, on m * B coefficients, three calls alternating:
                    fill     the shared-centre call (k_fill_gauss_tab)
                    general  the same call sent to the general kernel (k_fill_gauss; PSF_SAMPLE_GENERAL=1 in the experiments build)
                    samp_d   psfp_samp_d_dev of a handle whose s r equals the fill's s (k_samp_d: one lock-step sample_z per lane)
                  and the per-element-centre call (centres all 0) at the two widths.  Samples per second and mean Philox blocks per sample
                  (counted on the CPU oracle's rule over 2^14 samples).
HIP events around each call, warm-up excluded, medians of --reps.  Prints one line per row and writes sample_fill_timing.json (or --name).
Needs the experiments build (make exp) for the `general` rows; without it they are left out.

    python tools/time_sample_fill.py --out DIR [--name FILE.json] [--reps 21] [--scale 1.0]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12          # bytes/s, MI355X datasheet
SEED = 20261017


def timed(torch, members, warmup, reps):
    """{name: [ms]} of the members, alternating call by call"""
    for _ in range(warmup):
        for _, f in members:
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in members}
    for _ in range(reps):
        for name, f in members:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return ms


def blocks_per_sample(s, center=0.0, samples=1 << 14):
    """mean Philox blocks a narrow SampleZ draw consumes: one per group of four attempts and one per tie, replayed by the model"""
    from tests.helpers import sample_fill_model as M
    stats = {}
    _, ties, _ = M.gauss_narrow_trace(SEED, 64, 0, 1, samples, center, s, stats=stats)
    return (stats["groups"] + ties) / samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="sample_fill_timing.json")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every coefficient count (rehearsals)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    from tools_amd import _ffi
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    S = T.sample
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    n = 256

    def stat(ms):
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    # ---- write-bound fills beside a memset of the same buffer -------------------------------------------------------------------------------
    cases = [("cbd", io, dict(eta=eta), 1 << (28 if io == 16 else 26)) for eta in (2, 3, 8) for io in (16, 64)]
    cases += [("uniform", 16, dict(q=3329), 1 << 26), ("uniform", 64, dict(q=(1 << 62) - 57), 1 << 25)]
    for kind, io, kw, coeffs in cases:
        count = max(1, int(coeffs * a.scale) // n)
        buf = torch.empty(count * n, dtype=torch.int16 if io == 16 else torch.int64, device="cuda")
        if kind == "cbd":
            def call():
                S.sample_cbd_dev(buf.data_ptr(), count, n, kw["eta"], SEED, io_bits=io, device=a.device, stream=stream)
        else:
            def call():
                S.sample_uniform_dev(buf.data_ptr(), count, n, kw["q"], SEED, io_bits=io, device=a.device, stream=stream)
        ms = timed(torch, [(kind, call), ("memset", lambda: buf.zero_())], a.warmup, a.reps)
        nbytes = count * n * io // 8
        med, mem = statistics.median(ms[kind]), statistics.median(ms["memset"])
        row = {"op": kind, "io_bits": io, **kw, "coefficients": count * n, "bytes_written": nbytes, "reps": a.reps, **stat(ms[kind]),
               "memset_median_ms": round(mem, 4), "bytes_per_s": nbytes / (med * 1e-3), "memset_bytes_per_s": nbytes / (mem * 1e-3),
               "rate_over_memset": round(mem / med, 3), "fraction_of_8tbs": round(nbytes / (med * 1e-3) / HBM_SPEC, 3)}
        if kind == "uniform":
            row["philox_blocks_per_s"] = count * n / (med * 1e-3)
        rows.append(row)
        print(f"{kind:8s} io_bits={io:2d} {kw} n=2^{(count * n).bit_length() - 1} median {med:8.3f} ms  {row['bytes_per_s'] / 1e12:6.3f} TB/s  "
              f"{row['rate_over_memset']:5.3f} of the memset ({mem:.3f} ms)  (min {min(ms[kind]):.3f}, max {max(ms[kind]):.3f})", flush=True)
        del buf
        torch.cuda.empty_cache()

    # ---- Gaussian: the fill, the general kernel on the same input, and the handle-bound lock-step sampler -----------------------------------------
    exp = None
    if os.path.exists(_ffi.EXP_LIB_PATH):
        os.environ["PSF_SAMPLE_GENERAL"] = "1"                             # read by the experiments build only, at each call
        exp = _ffi.open_library(_ffi.EXP_LIB_PATH)
    r = 3.0
    cond1 = cond2 = True
    for s in (8.0, 300.0):
        psf = T.PSFPerturbation(T.GadgetParameters.init_default(8, 64), r, s / r, device=a.device)      # samp_d needs no key: D_{Z^m, s r}
        B = max(1, int((1 << 24) * a.scale) // psf.m)
        total = B * psf.m
        out = torch.empty(total, dtype=torch.int64, device="cuda")
        cen = torch.zeros(total, dtype=torch.float64, device="cuda")
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")

        def fill():
            S.sample_discrete_gauss_dev(out.data_ptr(), B, psf.m, s, SEED, d_fail=fail.data_ptr(), device=a.device, stream=stream)

        def general():
            _ffi.check(exp.psf_sample_discrete_gauss_dev(C.c_int(a.device), C.c_uint64(SEED), C.c_uint32(64), C.c_uint64(0), C.c_size_t(B), C.c_size_t(psf.m),
                                                         C.c_double(0.0), None, C.c_double(s), C.c_void_p(out.data_ptr()), C.c_void_p(fail.data_ptr()),
                                                         C.c_int(64), C.c_void_p(stream)), "general")

        def per_element():
            S.sample_discrete_gauss_dev(out.data_ptr(), B, psf.m, s, SEED, d_centers=cen.data_ptr(), d_fail=fail.data_ptr(), device=a.device, stream=stream)

        def samp_d():
            _ffi.check(_ffi.lib().psfp_samp_d_dev(psf._h, C.c_uint64(SEED), C.c_uint64(0), C.c_size_t(B), C.c_void_p(out.data_ptr()), C.c_void_p(stream)), "samp_d_dev")

        members = [("fill", fill)] + ([("general", general)] if exp is not None else []) + [("per_element", per_element), ("samp_d", samp_d)]
        ms = timed(torch, members, a.warmup, a.reps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        bps = blocks_per_sample(s)
        for name, _ in members:
            row = {"op": "gauss_" + name, "s": s, "center": 0.0, "samples": total, "reps": a.reps, **stat(ms[name]),
                   "samples_per_s": total / (med[name] * 1e-3), "philox_blocks_per_sample": bps, "time_over_samp_d": round(med[name] / med["samp_d"], 3)}
            rows.append(row)
            print(f"gauss {name:12s} s={s:5.1f} samples={total} median {med[name]:8.3f} ms  {row['samples_per_s'] / 1e9:6.2f} Gsamples/s  "
                  f"{row['time_over_samp_d']:.3f} of samp_d  ({bps and round(bps, 2)} blocks/sample; min {min(ms[name]):.3f}, max {max(ms[name]):.3f})", flush=True)
        cond1 = cond1 and med["fill"] < med["samp_d"]
        if exp is not None:
            cond2 = cond2 and med["fill"] < med["general"]
        assert int(fail.item()) == 0
        del out, cen, psf
        torch.cuda.empty_cache()
    print(f"shared-centre fill faster than psfp_samp_d_dev at both widths: {cond1}; table kernel faster than the general kernel: {cond2 if exp is not None else 'n/a'}",
          flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "hbm_spec_bytes_per_s": HBM_SPEC, "fill_faster_than_samp_d": cond1,
                   "table_faster_than_general": cond2 if exp is not None else None, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
