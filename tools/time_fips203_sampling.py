#!/usr/bin/env python3
"""Rates of the FIPS 203 device functions (tools_amd/fips203.py), each beside what it replaces or is bounded by, alternating call by call:

  keccak      psf_keccak_dev, SHAKE256 of 33 bytes into 128 (PRF_2) over 2^20 messages: Keccak-f[1600] permutations per second (one per message)
  sample_ntt  the matrix form at k = 3 over 65 536 seeds (589 824 polynomials) beside psf_sample_uniform_dev of the same output; permutations
              per second at the 3 per polynomial every input needs (a wave runs a fourth for all its lanes when one of them needs it)
  sample_cbd  eta = 2, per_seed = 6 over 65 536 seeds beside psf_sample_cbd_dev of the same output; one permutation per polynomial
  image_from / image_to   beside a device-to-device copy of (bytes read + bytes written) / 2
HIP events around each call, warm-up excluded, medians of --reps.  No time is a pass condition.  Prints one line per row and writes
fips203_timing.json (or --name).

    python tools/time_fips203_sampling.py --out DIR [--name FILE.json] [--reps 15] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261018
Q, N = 3329, 256


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="fips203_timing.json")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size (rehearsals)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    F, S = T.fips203, T.sample
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def stat(ms):
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    def report(op, ms, ref, extra):
        med = {k: statistics.median(v) for k, v in ms.items()}
        for name in ms:
            if name == ref:
                continue
            row = {"op": op, "member": name, "reps": a.reps, **stat(ms[name]), **extra}
            if ref:
                row[ref + "_median_ms"] = round(med[ref], 4)
                row["time_over_" + ref] = round(med[name] / med[ref], 3)
            if "permutations" in extra:
                row["keccak_permutations_per_s"] = extra["permutations"] / (med[name] * 1e-3)
            rows.append(row)
            perm = f"  {row['keccak_permutations_per_s'] / 1e9:7.3f} G permutations/s" if "permutations" in extra else ""
            beside = f"  {row['time_over_' + ref]:7.3f} x {ref} ({med[ref]:.3f} ms)" if ref else ""
            print(f"{op:12s} {name:10s} median {med[name]:9.3f} ms{perm}{beside}  (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})", flush=True)

    # ---- SHAKE256, 33 bytes in, 128 out ------------------------------------------------------------------------------------------------------
    count = max(1, int((1 << 20) * a.scale))
    msg = torch.randint(0, 256, (count, 33), dtype=torch.uint8, device="cuda")
    dig = torch.empty((count, 128), dtype=torch.uint8, device="cuda")
    ms = timed(torch, [("keccak", lambda: F.keccak_dev(F.SHAKE256, count, msg.data_ptr(), 33, dig.data_ptr(), 128, device=a.device, stream=stream))],
               a.warmup, a.reps)
    report("shake256", ms, None, {"messages": count, "in_len": 33, "out_len": 128, "permutations": count})
    del msg, dig

    # ---- the samplers beside the Philox fills of the same output -----------------------------------------------------------------------------
    seeds_n = max(1, int(65536 * a.scale))
    seeds = torch.randint(0, 256, (seeds_n, 32), dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for io in (16, 64):
        k = 3
        polys = seeds_n * k * k
        out = torch.empty(polys * N, dtype=torch.int16 if io == 16 else torch.int64, device="cuda")
        ms = timed(torch, [("sample_ntt", lambda: F.sample_ntt_dev(out.data_ptr(), seeds_n, seeds.data_ptr(), k=k, d_fail=flag.data_ptr(), io_bits=io,
                                                                          device=a.device, stream=stream)),
                          ("philox", lambda: S.sample_uniform_dev(out.data_ptr(), polys, N, Q, SEED, io_bits=io, device=a.device, stream=stream))],
                   a.warmup, a.reps)
        report("sample_ntt", ms, "philox", {"io_bits": io, "k": k, "seeds": seeds_n, "polynomials": polys, "permutations": 3 * polys})
        per = 6
        polys = seeds_n * per
        ms = timed(torch, [("sample_cbd", lambda: F.sample_cbd_dev(out.data_ptr(), seeds_n, seeds.data_ptr(), 2, per_seed=per, io_bits=io, device=a.device,
                                                                          stream=stream)),
                          ("philox", lambda: S.sample_cbd_dev(out.data_ptr(), polys, N, 2, SEED, io_bits=io, device=a.device, stream=stream))],
                   a.warmup, a.reps)
        report("sample_cbd", ms, "philox", {"io_bits": io, "eta": 2, "per_seed": per, "seeds": seeds_n, "polynomials": polys, "permutations": polys})
        del out
        torch.cuda.empty_cache()
    assert int(flag.item()) == 0

    # ---- the image conversions beside a copy of the same bytes -----------------------------------------------------------------------------------
    polys = seeds_n * 9
    for io in (16, 64):
        wb = io // 8
        fhat = torch.randint(0, Q, (polys * N,), dtype=torch.int16 if io == 16 else torch.int64, device="cuda")
        hat = torch.empty(polys * N, dtype=torch.int32, device="cuda")
        half = polys * N * (wb + 4) // 2
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        ms = timed(torch, [("image_from", lambda: F.image_from_fips203_dev(hat.data_ptr(), polys, fhat.data_ptr(), io_bits=io, device=a.device, stream=stream)),
                           ("image_to", lambda: F.image_to_fips203_dev(fhat.data_ptr(), polys, hat.data_ptr(), io_bits=io, device=a.device, stream=stream)),
                           ("copy", lambda: dst.copy_(src))], a.warmup, a.reps)
        report("image", ms, "copy", {"io_bits": io, "polynomials": polys, "bytes_moved": 2 * half})
        del fhat, hat, src, dst
        torch.cuda.empty_cache()

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
