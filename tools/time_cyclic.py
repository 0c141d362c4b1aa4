#!/usr/bin/env python3
"""Times the products of the cyclic ring Z_q[X]/(X^n - 1) (psf_*_cyclic*_dev) against their X^n + 1 twins on the same operands, in one process.

Cases: 53 248 pair products at n = 256, q = 3329 (16- and 64-bit words); the image product (one image for every product, both widths); A s for
k = 2, 3, 4 over 65 536 batches with one shared A in the hat form (both widths); and 4096 pair products at q = 2^30, n = 256, which has no NTT (the
schoolbook kernels).  After a warm-up of both rings, every repetition times one call of each ring with HIP events, the order alternating between
repetitions.  Prints one line per case (median, min and max of each ring, and the ratio of the medians) and writes cyclic_timing.json to --out.

    python tools/time_cyclic.py --out DIR [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(f, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def ab(label, cyc, neg, a, torch, extra):
    for _ in range(a.warmup):
        cyc()
        neg()
    torch.cuda.synchronize()
    tc, tn = [], []
    for r in range(a.reps):
        if r % 2 == 0:
            tc.append(event_ms(cyc, torch))
            tn.append(event_ms(neg, torch))
        else:
            tn.append(event_ms(neg, torch))
            tc.append(event_ms(cyc, torch))
    mc, mn = statistics.median(tc), statistics.median(tn)
    row = dict(extra, case=label, reps=a.reps, cyclic_ms=round(mc, 4), cyclic_min_ms=round(min(tc), 4), cyclic_max_ms=round(max(tc), 4),
               negacyclic_ms=round(mn, 4), negacyclic_min_ms=round(min(tn), 4), negacyclic_max_ms=round(max(tn), 4), ratio=round(mc / mn, 4))
    print(f"{label:34s} cyclic {mc:9.4f} ms [{min(tc):9.4f} {max(tc):9.4f}]  negacyclic {mn:9.4f} ms [{min(tn):9.4f} {max(tn):9.4f}]  "
          f"cyclic/negacyclic {mc / mn:6.3f}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 10:
        sys.exit("--reps must be at least 10")
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    dev = torch.device("cuda", a.device)
    st = torch.cuda.current_stream().cuda_stream
    d = a.device
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    rows = []

    q, n = 3329, 256
    for io in (16, 64):
        dt = torch.int16 if io == 16 else torch.int64
        count = 53248
        A = torch.randint(0, q, (count, n), dtype=dt, device=dev, generator=g)
        B = torch.randint(-q + 1, q, (count, n), dtype=dt, device=dev, generator=g)
        O = torch.empty_like(A)
        rows.append(ab(f"pair n=256 q=3329 io={io}",
                       lambda: T.rq.poly_mul_cyclic_dev(A.data_ptr(), B.data_ptr(), O.data_ptr(), q, n, count, io_bits=io, device=d, stream=st),
                       lambda: T.gadget.poly_mul_negacyclic_dev(A.data_ptr(), B.data_ptr(), O.data_ptr(), q, n, count, io_bits=io, device=d, stream=st),
                       a, torch, {"q": q, "n": n, "count": count, "io_bits": io}))
        hc = torch.empty((1, n), dtype=torch.int32, device=dev)
        hn = torch.empty((1, n), dtype=torch.int32, device=dev)
        T.rq.ntt_forward_cyclic_dev(A.data_ptr(), hc.data_ptr(), q, n, 1, io_bits=io, device=d, stream=st)
        T.gadget.ntt_forward_dev(A.data_ptr(), hn.data_ptr(), q, n, 1, io_bits=io, device=d, stream=st)
        rows.append(ab(f"image product n=256 q=3329 io={io}",
                       lambda: T.rq.poly_mul_hat_cyclic_dev(hc.data_ptr(), 0, B.data_ptr(), O.data_ptr(), q, n, count, io_bits=io, device=d, stream=st),
                       lambda: T.gadget.poly_mul_hat_dev(hn.data_ptr(), 0, B.data_ptr(), O.data_ptr(), q, n, count, io_bits=io, device=d, stream=st),
                       a, torch, {"q": q, "n": n, "count": count, "io_bits": io, "hat_stride": 0}))
        del A, B, O
        for k in (2, 3, 4):
            count = 65536
            Am = torch.randint(0, q, (k, k, n), dtype=dt, device=dev, generator=g)
            S = torch.randint(-q + 1, q, (count, k, 1, n), dtype=dt, device=dev, generator=g)
            Cm = torch.empty((count, k, 1, n), dtype=dt, device=dev)
            hc = torch.empty((k * k, n), dtype=torch.int32, device=dev)
            hn = torch.empty((k * k, n), dtype=torch.int32, device=dev)
            T.rq.ntt_forward_cyclic_dev(Am.data_ptr(), hc.data_ptr(), q, n, k * k, io_bits=io, device=d, stream=st)
            T.gadget.ntt_forward_dev(Am.data_ptr(), hn.data_ptr(), q, n, k * k, io_bits=io, device=d, stream=st)
            rows.append(ab(f"A.s hat k={k} n=256 q=3329 io={io}",
                           lambda: T.rq.matpoly_mul_hat_cyclic_dev(hc.data_ptr(), S.data_ptr(), Cm.data_ptr(), q, n, count, k, k, 1, io_bits=io, device=d,
                                                                   stream=st),
                           lambda: T.rq.matpoly_mul_hat_dev(hn.data_ptr(), S.data_ptr(), Cm.data_ptr(), q, n, count, k, k, 1, io_bits=io, device=d, stream=st),
                           a, torch, {"q": q, "n": n, "count": count, "rows": k, "inner": k, "cols": 1, "io_bits": io, "a": "shared/hat"}))
            del Am, S, Cm
            torch.cuda.empty_cache()

    q, count = 1 << 30, 4096                                                # no NTT: the schoolbook kernels
    A = torch.randint(0, q, (count, n), dtype=torch.int64, device=dev, generator=g)
    B = torch.randint(-q + 1, q, (count, n), dtype=torch.int64, device=dev, generator=g)
    O = torch.empty_like(A)
    rows.append(ab("pair schoolbook n=256 q=2^30 io=64",
                   lambda: T.rq.poly_mul_cyclic_dev(A.data_ptr(), B.data_ptr(), O.data_ptr(), q, n, count, device=d, stream=st),
                   lambda: T.gadget.poly_mul_negacyclic_dev(A.data_ptr(), B.data_ptr(), O.data_ptr(), q, n, count, device=d, stream=st),
                   a, torch, {"q": q, "n": n, "count": count, "io_bits": 64}))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "cyclic_timing.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
