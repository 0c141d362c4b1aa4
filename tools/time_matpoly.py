#!/usr/bin/env python3
"""Times the R_q matrix product (psf_matpoly_mul_hat_dev / psf_matpoly_mul_negacyclic_dev) on device buffers against the composed route it replaces:
rows * inner pair products through psf_poly_mul_hat_dev / psf_poly_mul_negacyclic_dev, then a torch sum over k and a mod.

Shapes: the module products A s (k x k . k x 1) and A^T r (trans_a = 1) for k = 2, 3, 4 at n = 256, q = 3329 over `count` batches; both I/O widths;
A shared by every batch through the hat form (images from psf_ntt_forward_dev) and A per batch through the plain form.  And the ring trapdoor check
at the C4 parameters: 1 x (k+2) . (k+2) x n(k+2) (short_basis_ring.rs:183-198), count 1.  The composed route gets its pair operands laid out before
the clock starts (its gather is not timed).  Warm-up, then HIP events around each call, median of --reps calls.  Bytes moved count what the fused
call reads and writes once (A or its images, B, C).  Prints one line per shape and writes matpoly_timing.json to --out.

    python tools/time_matpoly.py --out DIR [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12          # bytes/s, MI355X datasheet


def timed(f, reps, warmup, torch):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def one_shape(T, torch, a, q, n, count, rows, inner, cols, trans, shared, io_bits, label):
    dev = torch.device("cuda", a.device)
    dt = torch.int16 if io_bits == 16 else torch.int64
    wb = io_bits // 8
    g = torch.Generator(device=dev)
    g.manual_seed(count * 131 + rows * 7 + inner)
    na = 1 if shared else count
    A = torch.randint(0, q, (na, rows, inner, n), dtype=dt, device=dev, generator=g)          # logical layout
    Ast = A.transpose(1, 2).contiguous() if trans else A                                     # storage layout
    B = torch.randint(-q + 1, q, (count, inner, cols, n), dtype=dt, device=dev, generator=g)
    Cm = torch.empty((count, rows, cols, n), dtype=dt, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    per = rows * inner
    if shared:                                                                               # the hat form: images of the one A
        hat = torch.empty((per, n), dtype=torch.int32, device=dev)
        T.gadget.ntt_forward_dev(Ast.data_ptr(), hat.data_ptr(), q, n, per, io_bits=io_bits, device=a.device, stream=st)

        def fused():
            T.rq.matpoly_mul_hat_dev(hat.data_ptr(), B.data_ptr(), Cm.data_ptr(), q, n, count, rows, inner, cols, hat_stride=0, trans_a=trans,
                                     io_bits=io_bits, device=a.device, stream=st)
        a_bytes = per * n * 4
        # composed: one psf_poly_mul_hat_dev per (i, k) over the count * cols products A[i][k] * B[c][k][j]; B[:, k] laid out contiguous beforehand
        hat_l = hat.view(inner, rows, n).transpose(0, 1).contiguous() if trans else hat.view(rows, inner, n)
        Bk = [B[:, k].contiguous() for k in range(inner)]
        P = torch.empty((rows, inner, count * cols, n), dtype=dt, device=dev)

        def composed():
            for i in range(rows):
                for k in range(inner):
                    T.gadget.poly_mul_hat_dev(hat_l[i, k].data_ptr(), 0, Bk[k].data_ptr(), P[i, k].data_ptr(), q, n, count * cols, io_bits=io_bits,
                                              device=a.device, stream=st)
            Cm.copy_((P.to(torch.int32).sum(1) % q).view(rows, count, cols, n).transpose(0, 1))
    else:
        def fused():
            T.rq.matpoly_mul_dev(Ast.data_ptr(), B.data_ptr(), Cm.data_ptr(), q, n, count, rows, inner, cols, a_stride=per, trans_a=trans,
                                 io_bits=io_bits, device=a.device, stream=st)
        a_bytes = count * per * n * wb
        # composed: one psf_poly_mul_negacyclic_dev over all count * rows * cols * inner pairs, operands gathered beforehand
        pa = A[:, :, None].expand(count, rows, cols, inner, n).contiguous()
        pb = B.transpose(1, 2)[:, None].expand(count, rows, cols, inner, n).contiguous()
        P = torch.empty_like(pa)
        npairs = count * rows * cols * inner

        def composed():
            T.gadget.poly_mul_negacyclic_dev(pa.data_ptr(), pb.data_ptr(), P.data_ptr(), q, n, npairs, io_bits=io_bits, device=a.device, stream=st)
            Cm.copy_(P.to(torch.int32).sum(3) % q)
    moved = a_bytes + (count * inner * cols + count * rows * cols) * n * wb
    fm, fmin, fmax = timed(fused, a.reps, a.warmup, torch)
    fused_out = Cm.clone()
    cm, cmin, cmax = timed(composed, a.reps, a.warmup, torch)
    torch.cuda.synchronize()
    same = bool(torch.equal(fused_out, Cm))
    outs = count * rows * cols
    row = {"shape": label, "q": q, "n": n, "count": count, "rows": rows, "inner": inner, "cols": cols, "trans_a": trans, "a": "shared/hat" if shared else "per-batch/plain",
           "io_bits": io_bits, "reps": a.reps, "fused_ms": round(fm, 4), "fused_min_ms": round(fmin, 4), "fused_max_ms": round(fmax, 4),
           "composed_ms": round(cm, 4), "composed_min_ms": round(cmin, 4), "composed_max_ms": round(cmax, 4), "speedup": round(cm / fm, 2),
           "fused_outputs_per_s": outs / (fm * 1e-3), "bytes_moved": moved, "fraction_of_8tbs": round(moved / (fm * 1e-3) / HBM_SPEC, 4),
           "results_equal": same}
    print(f"{label:10s} k/rows={rows:2d} inner={inner:2d} cols={cols:5d} count={count:6d} io={io_bits:2d} {row['a']:16s} fused {fm:8.3f} ms "
          f"composed {cm:8.3f} ms  x{cm / fm:5.2f}  {outs / (fm * 1e-3) / 1e6:8.2f} Mpoly/s  {row['fraction_of_8tbs']:.3f} of 8 TB/s  equal={same}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
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
            for trans, label in ((0, "A.s"), (1, "A^T.r")):
                for io in (16, 64):
                    for shared in (True, False):
                        rows.append(one_shape(T, torch, a, q, n, count, k, k, 1, trans, shared, io, label))
                        torch.cuda.empty_cache()
    gp = T.GadgetParametersRing.init_default(n, q)                          # C4: the ring trapdoor check a . S
    K = gp.k + 2
    for io in (16, 64):
        for shared in (True, False):
            rows.append(one_shape(T, torch, a, q, n, 1, 1, K, n * K, 0, shared, io, "a.S(C4)"))
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "matpoly_timing.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "hbm_spec_bytes_per_s": HBM_SPEC, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
