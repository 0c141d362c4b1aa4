#!/usr/bin/env python3
"""Times the fused R_q multiply-add (psf_matpoly_mul_add_hat_dev, C = E + A B) on device buffers against the two routes it replaces.

Shapes: the module steps A s + e (k x k . k x 1) and A^T r + e (trans_a = 1) for k = 2, 3, 4 at n = 256, q = 3329 over `count` batches, at both word
widths, with one A for every batch given by its images (psf_ntt_forward_dev).  Every timed case alternates, call by call, between three routes on the
same buffers:
  (a) the fused call                    psf_matpoly_mul_add_hat_dev(E, +1)
  (b) the product alone                 psf_matpoly_mul_hat_dev
  (c) the product, then torch           C = remainder(C + E, q)
Warm-up, then HIP events around each call, median of --reps calls per route.  Prints one line per shape and writes one JSON per run,
matpoly_add_timing_run{N}.json, to --out.  The condition a run has to show: median (a) <= median (c) for every shape (`fused_not_slower`); the ratio
(a) / (b) is recorded without a threshold.

    python tools/time_matpoly_add.py --out DIR --run 1 [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_alternating(routes, reps, warmup, torch):
    """{name: (median, min, max) ms}: the routes take turns, call by call, so that drift of the clocks falls on all of them alike"""
    for _ in range(warmup):
        for f in routes.values():
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(reps):
        for name, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def one_shape(T, torch, a, q, n, count, k, trans, io_bits, label):
    dev = torch.device("cuda", a.device)
    dt = torch.int16 if io_bits == 16 else torch.int64
    g = torch.Generator(device=dev)
    g.manual_seed(count * 131 + k * 7 + trans)
    A = torch.randint(0, q, (k, k, n), dtype=dt, device=dev, generator=g)                    # storage order; trans_a reads it transposed
    B = torch.randint(-q + 1, q, (count, k, 1, n), dtype=dt, device=dev, generator=g)
    E = torch.randint(-q + 1, q, (count, k, 1, n), dtype=dt, device=dev, generator=g)
    Cm = torch.empty((count, k, 1, n), dtype=dt, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hat = torch.empty((k * k, n), dtype=torch.int32, device=dev)
    T.gadget.ntt_forward_dev(A.data_ptr(), hat.data_ptr(), q, n, k * k, io_bits=io_bits, device=a.device, stream=st)

    def fused():
        T.rq.matpoly_mul_add_hat_dev(hat.data_ptr(), B.data_ptr(), E.data_ptr(), Cm.data_ptr(), q, n, count, k, k, 1, hat_stride=0, trans_a=trans, sign=1,
                                     io_bits=io_bits, device=a.device, stream=st)

    def product():
        T.rq.matpoly_mul_hat_dev(hat.data_ptr(), B.data_ptr(), Cm.data_ptr(), q, n, count, k, k, 1, hat_stride=0, trans_a=trans, io_bits=io_bits,
                                 device=a.device, stream=st)

    def product_then_torch():
        product()
        torch.remainder(Cm.add_(E), q, out=Cm)

    fused()
    want = Cm.clone()
    product_then_torch()
    torch.cuda.synchronize()
    same = bool(torch.equal(want, Cm))
    t = timed_alternating({"fused": fused, "product": product, "product_then_torch": product_then_torch}, a.reps, a.warmup, torch)
    fm, pm, cm = t["fused"][0], t["product"][0], t["product_then_torch"][0]
    row = {"shape": label, "q": q, "n": n, "count": count, "k": k, "trans_a": trans, "io_bits": io_bits, "reps": a.reps, "results_equal": same,
           "fused_over_product": round(fm / pm, 4), "fused_over_product_then_torch": round(fm / cm, 4), "fused_not_slower": bool(fm <= cm)}
    for name, (med, lo, hi) in t.items():
        row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = round(med, 4), round(lo, 4), round(hi, 4)
    print(f"{label:10s} k={k} count={count:6d} io={io_bits:2d}  (a) fused {fm:7.3f} ms  (b) product {pm:7.3f} ms  (c) product + torch {cm:7.3f} ms  "
          f"a/b {fm / pm:5.3f}  a/c {fm / cm:5.3f}  a <= c: {fm <= cm}  equal={same}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--run", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--counts", default="4096,16384,65536")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 10:
        sys.exit("--reps must be at least 10")
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    q, n = 3329, 256
    rows = []
    for k in (2, 3, 4):
        for count in [int(c) for c in a.counts.split(",")]:
            for trans, label in ((0, "A.s+e"), (1, "A^T.r+e")):
                for io in (16, 64):
                    rows.append(one_shape(T, torch, a, q, n, count, k, trans, io, label))
                    torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"matpoly_add_timing_run{a.run}.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "run": a.run, "variant": "separate kernel (k_matpoly_fma)",
                   "all_fused_not_slower": all(r["fused_not_slower"] for r in rows), "all_results_equal": all(r["results_equal"] for r in rows), "rows": rows},
                  fh, indent=1)


if __name__ == "__main__":
    main()
