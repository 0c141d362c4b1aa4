#!/usr/bin/env python3
"""samp_p_dev_many against the loop of samp_p_dev calls it replaces, at bench.py's C2 (PSFGPV) and C4 (PSFGPVRing) shapes: same key seed (3), targets of
uniform_targets_dev(seed=7).  For each count: (a) `count` back-to-back samp_p_dev calls on one stream, (b) one samp_p_dev_many; both warmed up, then alternated
(a, b, a, b, ...) inside this process, each leg timed by events on the stream between two device synchronisations.  Prints ms per batch with the spread of the
repetitions, whether (a) and (b) wrote the same rows, and the walk's form with the re-runs counted during each leg; writes one JSON record.

usage: python tools/np_many_sweep.py [--configs c2 c4] [--counts 2 4 16] [--reps 3] [--out profiles/np_many_sweep.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # bench.py CONFIGS: (scheme, n, q, r, s, batch)
    "c2": ("PSFGPV", 256, 3329, None, 1024.0, 1024),
    "c4": ("PSFGPVRing", 256, 3329, None, 0.0, 4096),
}
KEY_SEED = 3


def make(cfg):
    import tools_amd as T
    from tools_amd._ffi import lib, check
    scheme, n, q, _, s, B = SHAPES[cfg]
    if scheme == "PSFGPV":
        psf = T.PSFGPV(T.GadgetParameters.init_default(n, q), s)
        psf.trap_gen(KEY_SEED, export=False)
        return psf, n, psf.m, B
    s = s or ((2 * 2 * 1.005 * math.sqrt(n) + 1) * 2) * 4               # compute_s, gpv_ring.rs:296-298
    psf = T.PSFGPVRing(T.GadgetParametersRing.init_default(n, q), s, 1.005)
    check(lib().psfring_trap_gen(psf._h, C.c_uint64(KEY_SEED)), "trap_gen")
    return psf, n, psf.d, B


def spread(xs):
    return {"min": min(xs), "median": sorted(xs)[len(xs) // 2], "max": max(xs)}


def run(cfg, counts, reps):
    import torch
    psf, n, d, B = make(cfg)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    cmax = max(counts)
    u = torch.empty((cmax * B, n), dtype=torch.int64, device="cuda")
    psf.uniform_targets_dev(u.data_ptr(), cmax * B, seed=7, first_index=0, stream=st)
    ea = torch.empty((cmax * B, d), dtype=torch.int64, device="cuda")
    eb = torch.empty((cmax * B, d), dtype=torch.int64, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rec = {"config": cfg, "batch": B, "d": d, "counts": {}}
    for count in counts:
        seeds = [1000 + i for i in range(count)]
        firsts = [i * B for i in range(count)]

        def seq():
            for i in range(count):
                psf.samp_p_dev(u[i * B].data_ptr(), ea[i * B].data_ptr(), B, seed=seeds[i], first_index=firsts[i], stream=st)

        def many():
            psf.samp_p_dev_many(u.data_ptr(), eb.data_ptr(), B, seeds, firsts, stream=st)

        legs = {"seq": seq, "many": many}
        # enough work per timed leg that launch jitter does not dominate (at least ~32 batches)
        inner = max(1, 32 // count)
        for f in legs.values():                                        # warm-up: both lanes allocated, kernels loaded
            f()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        reruns = {k: 0 for k in legs}
        equal = []
        for _ in range(reps):
            for k, f in legs.items():
                r0 = psf.nearest_plane_form()[3]
                torch.cuda.synchronize()
                ev0.record(stream)
                for _ in range(inner):
                    f()
                ev1.record(stream)
                torch.cuda.synchronize()
                ms[k].append(ev0.elapsed_time(ev1) / (inner * count))
                form = psf.nearest_plane_form()
                reruns[k] += form[3] - r0
                assert psf.last_status() == 0, (cfg, count, k)
            equal.append(bool(torch.equal(ea[:count * B], eb[:count * B])))
        form = psf.nearest_plane_form()
        seq_med, many_med = spread(ms["seq"])["median"], spread(ms["many"])["median"]
        rec["counts"][str(count)] = {
            "ms_per_batch": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "seq": spread(ms["seq"]), "many": spread(ms["many"]),
            "many_vs_seq": round(many_med / seq_med, 4),
            "rows_equal": all(equal), "form": form[0], "preimages_per_wave": form[1], "reruns": reruns,
            "timed_batches_per_leg": inner * count,
        }
        print(f"[{cfg}] count {count:2d}: seq {seq_med:.3f} ms/batch ({min(ms['seq']):.3f}-{max(ms['seq']):.3f}), "
              f"many {many_med:.3f} ({min(ms['many']):.3f}-{max(ms['many']):.3f}), many/seq {many_med / seq_med:.3f}, rows equal {all(equal)}, "
              f"form {form[0]} G {form[1]}, reruns seq {reruns['seq']} many {reruns['many']}", flush=True)
    psf.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c4"], choices=sorted(SHAPES))
    ap.add_argument("--counts", nargs="+", type=int, default=[2, 4, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "np_many_sweep.json"))
    args = ap.parse_args()
    import torch
    t0 = time.time()
    out = {"tool": "tools/np_many_sweep.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "results": [run(c, args.counts, args.reps) for c in args.configs]}
    out["wall_s"] = round(time.time() - t0, 1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
