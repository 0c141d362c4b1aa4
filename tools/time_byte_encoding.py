#!/usr/bin/env python3
"""Rates of the four byte-encoding operations on device buffers (psf_byte_encode_dev, psf_byte_decode_dev, psf_compress_encode_dev,
psf_decode_decompress_dev) against the two-call routes they replace and against a copy of the same traffic.

Cases: 2^28 coefficients in 16-bit words at q = 3329, d in {1, 4, 5, 10, 11, 12}; 2^27 coefficients in 64-bit words at q = 2^62 - 57,
d in {12, 40}.  Every buffer is far larger than the 256 MiB Infinity Cache except the packed bytes at small d.  Per case and direction three
things are timed, alternating call by call in one process, HIP events around each, warm-up excluded, medians of --reps:

  fused     psf_compress_encode_dev                     / psf_decode_decompress_dev
  two-call  psf_lossy_compress_dev + psf_byte_encode_dev / psf_byte_decode_dev + psf_lossy_decompress_dev (one event pair around both)
  copy      a device-to-device copy of (bytes read + bytes written) / 2 bytes of the fused form: the same traffic, no arithmetic

and, the same way, the plain psf_byte_encode_dev / psf_byte_decode_dev (q = 0) with their own matched copy.  Prints one line per row and
writes byte_encoding_timing.json (or --name) to --out.

    python tools/time_byte_encoding.py --out DIR [--name FILE.json] [--reps 21] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12          # bytes/s, MI355X datasheet
CASES = [(16, 3329, d, 1 << 28) for d in (1, 4, 5, 10, 11, 12)] + [(64, (1 << 62) - 57, d, 1 << 27) for d in (12, 40)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="byte_encoding_timing.json")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every coefficient count (rehearsals)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    Cm = T.compression
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for io_bits, q, d, n in CASES:
        n = max(8192, int(n * a.scale) // 8192 * 8192)
        wb = io_bits // 8
        nb = n * d // 8
        dtype = torch.int16 if io_bits == 16 else torch.int64
        lo, hi = (-(1 << 15), 1 << 15) if io_bits == 16 else (-(1 << 63), (1 << 63) - 1)
        vals = torch.randint(lo, hi, (n,), dtype=dtype, device="cuda")
        mid = torch.empty_like(vals)                                     # the d-bit values of the two-call routes, one word each
        back = torch.empty_like(vals)
        packed = torch.empty(nb, dtype=torch.uint8, device="cuda")
        Cm.compress_encode_dev(vals.data_ptr(), packed.data_ptr(), q, d, n, io_bits=io_bits, stream=stream)      # valid bytes for the decodes
        half = (n * wb + nb) // 2                                        # (bytes read + bytes written) / 2 of every one-pass operation here
        csrc = torch.empty(half, dtype=torch.uint8, device="cuda")
        cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
        kw = dict(io_bits=io_bits, device=a.device, stream=stream)
        V, M_, K, P = vals.data_ptr(), mid.data_ptr(), back.data_ptr(), packed.data_ptr()

        def two_call_encode():
            Cm.lossy_compress_dev(V, M_, q, d, n, **kw)
            Cm.byte_encode_dev(M_, P, d, n, **kw)

        def two_call_decode():
            Cm.byte_decode_dev(P, M_, 0, d, n, **kw)
            Cm.lossy_decompress_dev(M_, K, q, d, n, **kw)

        groups = [
            ("encode", [("compress_encode", lambda: Cm.compress_encode_dev(V, P, q, d, n, **kw), n * wb + nb),
                        ("compress+byte_encode", two_call_encode, 2 * n * wb + n * wb + nb),
                        ("copy", lambda: cdst.copy_(csrc), 2 * half)]),
            ("decode", [("decode_decompress", lambda: Cm.decode_decompress_dev(P, K, q, d, n, **kw), n * wb + nb),
                        ("byte_decode+decompress", two_call_decode, nb + n * wb + 2 * n * wb),
                        ("copy", lambda: cdst.copy_(csrc), 2 * half)]),
            ("plain", [("byte_encode", lambda: Cm.byte_encode_dev(V, P, d, n, **kw), n * wb + nb),
                       ("byte_decode", lambda: Cm.byte_decode_dev(P, K, 0, d, n, **kw), n * wb + nb),
                       ("copy", lambda: cdst.copy_(csrc), 2 * half)]),
        ]
        for gname, members in groups:
            for _ in range(a.warmup):
                for _, f, _ in members:
                    f()
            torch.cuda.synchronize()
            ms = {name: [] for name, _, _ in members}
            for _ in range(a.reps):                                      # the members alternate call by call
                for name, f, _ in members:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            med = {name: statistics.median(v) for name, v in ms.items()}
            for name, _, moved in members:
                rate = moved / (med[name] * 1e-3)
                row = {"group": gname, "op": name, "io_bits": io_bits, "q": q, "d": d, "coefficients": n, "bytes_moved": moved, "reps": a.reps,
                       "median_ms": round(med[name], 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                       "bytes_per_s": rate, "tb_per_s": round(rate / 1e12, 3), "fraction_of_8tbs": round(rate / HBM_SPEC, 3),
                       "time_over_copy": round(med[name] / med["copy"], 3), "gcoeff_per_s": round(n / (med[name] * 1e-3) / 1e9, 2)}
                if gname != "plain" and name not in ("copy",) and "+" not in name:
                    two = [m for m, _, _ in members if "+" in m][0]
                    row["time_over_two_call"] = round(med[name] / med[two], 3)
                    row["faster_than_two_call"] = bool(med[name] < med[two])
                rows.append(row)
                extra = f"  {row['time_over_two_call']:.3f} of the two-call route" if "time_over_two_call" in row else ""
                print(f"{name:24s} io_bits={io_bits:2d} d={d:2d} n=2^{n.bit_length() - 1} median {med[name]:8.3f} ms  {rate / 1e12:6.3f} TB/s  "
                      f"{rate / HBM_SPEC:5.3f} of 8 TB/s  {med[name] / med['copy']:6.3f} x copy  (min {min(ms[name]):.3f}, max {max(ms[name]):.3f}){extra}",
                      flush=True)
        del vals, mid, back, packed, csrc, cdst
        torch.cuda.empty_cache()
    fused = [r for r in rows if "time_over_two_call" in r]
    ok = all(r["faster_than_two_call"] for r in fused)
    print(f"fused faster than its two-call route in every case: {ok}  (worst ratio {max(r['time_over_two_call'] for r in fused):.3f})", flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "hbm_spec_bytes_per_s": HBM_SPEC, "fused_faster_in_every_case": ok, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
