#!/usr/bin/env python3
"""Rates of the four R_q coefficient maps on device buffers (psf_lossy_compress_dev, psf_lossy_decompress_dev, psf_encode_digits_dev,
psf_decode_digits_dev) at 16- and 64-bit words: 1 GiB moved per call (read + written), four times the 256 MiB Infinity Cache, so every call
streams from HBM.  Warm-up, then HIP events around each call, median of --reps calls.  A device-to-device copy of the same buffers
(torch `copy_`) is timed the same way as the read + write yardstick.  Prints one line per (op, io_bits) and writes compression_timing.json
to --out.

    python tools/time_compression.py --out DIR [--reps 25] [--gib 1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12          # bytes/s, MI355X datasheet
# (op, q, d or base) per word size: the ML-KEM setting at 16 bits, a modulus near the library's limit at 64
CASES = {16: [("compress", 3329, 11), ("decompress", 3329, 11), ("encode", 3329, 2), ("decode", 3329, 2)],
         64: [("compress", (1 << 62) - 57, 40), ("decompress", (1 << 62) - 57, 40), ("encode", (1 << 62) - 57, 2), ("decode", (1 << 62) - 57, 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="bytes moved per call, in GiB")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 20:
        sys.exit("--reps must be at least 20")
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    calls = {"compress": T.compression.lossy_compress_dev, "decompress": T.compression.lossy_decompress_dev,
             "encode": T.encodings.encode_digits_dev, "decode": T.encodings.decode_digits_dev}
    rows = []
    for io_bits, cases in CASES.items():
        wb = io_bits // 8
        n = int(a.gib * (1 << 30)) // (2 * wb)                            # coefficients: n words read + n words written
        dtype = torch.int16 if io_bits == 16 else torch.int64
        lo, hi = (-(1 << 15), 1 << 15) if io_bits == 16 else (-(1 << 63), (1 << 63) - 1)
        src = torch.randint(lo, hi, (n,), dtype=dtype, device="cuda")
        dst = torch.empty_like(src)
        stream = torch.cuda.current_stream().cuda_stream

        def copy(*_, **__):                                           # the yardstick: the same bytes read and written, no arithmetic
            dst.copy_(src)

        for op, q, p in cases + [("copy", 0, 0)]:
            f = calls.get(op, copy)
            for _ in range(a.warmup):
                f(src.data_ptr(), dst.data_ptr(), q, p, n, io_bits=io_bits, device=a.device, stream=stream)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f(src.data_ptr(), dst.data_ptr(), q, p, n, io_bits=io_bits, device=a.device, stream=stream)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            moved = 2 * n * wb
            rate = moved / (med * 1e-3)
            row = {"op": op, "io_bits": io_bits, "q": q, "param": p, "coefficients": n, "bytes_moved": moved, "reps": a.reps,
                   "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                   "bytes_per_s": rate, "tb_per_s": round(rate / 1e12, 3), "fraction_of_8tbs": round(rate / HBM_SPEC, 3),
                   "gcoeff_per_s": round(n / (med * 1e-3) / 1e9, 2)}
            rows.append(row)
            print(f"{op:10s} io_bits={io_bits:2d} n={n} median {med:8.3f} ms  {rate / 1e12:6.3f} TB/s  {rate / HBM_SPEC:5.3f} of 8 TB/s  "
                  f"{row['gcoeff_per_s']:7.2f} Gcoeff/s  (min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
        del src, dst
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "compression_timing.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "hbm_spec_bytes_per_s": HBM_SPEC, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
