#!/usr/bin/env python3
"""Wall time of the host-pointer forms, which stage their buffers on the device for the length of the call (tools_amd/csrc/psf_call.hpp: HostCall):
psf_mlkem_keygen / encaps / decaps (ML-KEM-768), psf_mldsa_keygen / verify (ML-DSA-65) and psf_slhdsa_verify (SLH-DSA-SHAKE-128f), 4 096 instances each,
through raw ctypes on packed numpy arrays.  A call returns when its outputs are on the host, so time.perf_counter around it is the whole of it:
allocation, upload, kernels, download, the wipes of the secret copies and the release.  One warm-up call, then the median of --reps.

The inputs are honest: the keys come from the key generations, the ciphertexts from encaps, the signatures from psf_mldsa_sign and psf_slhdsa_sign, and
before timing every verification must accept and decaps must return the shared secrets of encaps.  PSF_LIB selects another build of the same ABI, which
is how two commits are compared in one session.  No time is a pass condition.  Prints one line per entry point and writes host_forms_timing.json (or
--name).

    python tools/time_host_forms.py --out DIR [--name FILE.json] [--reps 7] [--count 4096]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEM, DSA, SLH = "ML-KEM-768", "ML-DSA-65", "SLH-DSA-SHAKE-128f"
MSG_LEN = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="host_forms_timing.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    n, dev = a.count, a.device
    rng = np.random.default_rng(20261020)

    def rand(length):
        return rng.integers(0, 256, (n, length), dtype=np.uint8)

    def out(length):
        return np.zeros((n, length), np.uint8)

    def p(x):
        return x.ctypes.data

    def ok(status, where):
        if status != 0:
            sys.exit(f"{where}: status {status}")

    K, kem, ksz = T.mlkem._lib(), T.mlkem._param(KEM), T.mlkem.sizes(KEM)
    D, dsa, dsz = T.mldsa._lib(), T.mldsa._param(DSA), T.mldsa.sizes(DSA)
    S, slh, ssz = T.slhdsa._lib(), T.slhdsa._param(SLH), T.slhdsa.sizes(SLH)
    sn = ssz["pk"] // 2

    d, z, m, ek, dk, ss, ss2, ct = rand(32), rand(32), rand(32), out(ksz["ek"]), out(ksz["dk"]), out(32), out(32), out(ksz["ct"])
    xi, msg, dpk, dsk, dsig, dok = rand(32), rand(MSG_LEN), out(dsz["pk"]), out(dsz["sk"]), out(dsz["sig"]), out(1)
    seeds, spk, ssk, ssig, sok = [rand(sn) for _ in range(3)], out(ssz["pk"]), out(ssz["sk"]), out(ssz["sig"]), out(1)

    calls = [
        ("psf_mlkem_keygen", KEM, lambda: K.psf_mlkem_keygen(dev, kem, n, p(d), p(z), p(ek), p(dk))),
        ("psf_mlkem_encaps", KEM, lambda: K.psf_mlkem_encaps(dev, kem, n, p(ek), p(m), p(ss), p(ct))),
        ("psf_mlkem_decaps", KEM, lambda: K.psf_mlkem_decaps(dev, kem, n, p(dk), p(ct), p(ss2))),
        ("psf_mldsa_keygen", DSA, lambda: D.psf_mldsa_keygen(dev, dsa, n, p(xi), p(dpk), p(dsk))),
        ("psf_mldsa_verify", DSA, lambda: D.psf_mldsa_verify(dev, dsa, n, p(dpk), dsz["pk"], p(msg), MSG_LEN, MSG_LEN, 0, p(dsig), p(dok), None)),
        ("psf_slhdsa_verify", SLH, lambda: S.psf_slhdsa_verify(dev, slh, n, p(spk), ssz["pk"], p(msg), MSG_LEN, MSG_LEN, p(ssig), p(sok))),
    ]
    # what the timed calls read that they do not make themselves
    setup = {
        "psf_mldsa_verify": lambda: D.psf_mldsa_sign(dev, dsa, n, p(dsk), dsz["sk"], p(msg), MSG_LEN, MSG_LEN, 0, None, p(dsig), 64, None),
        "psf_slhdsa_verify": lambda: (S.psf_slhdsa_keygen(dev, slh, n, p(seeds[0]), p(seeds[1]), p(seeds[2]), p(spk), p(ssk))
                                      or S.psf_slhdsa_sign(dev, slh, n, p(ssk), ssz["sk"], p(msg), MSG_LEN, MSG_LEN, None, p(ssig))),
    }
    rows = []
    for entry, name, call in calls:
        if entry in setup:
            ok(setup[entry](), entry + ": inputs")
        ok(call(), entry)                                                  # the warm-up call, and the one whose results are checked
        if entry == "psf_mlkem_decaps":
            assert (ss2 == ss).all() and ss.any(), "decaps does not return the shared secrets of encaps"
        if entry.endswith("_verify"):
            assert (dok if entry == "psf_mldsa_verify" else sok).all(), entry + " rejects an honest signature"
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            status = call()
            ms.append((time.perf_counter() - t0) * 1e3)
            ok(status, entry)
        row = {"entry": entry, "set": name, "count": n, "reps": a.reps, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
               "max_ms": round(max(ms), 4)}
        rows.append(row)
        print(f"{entry:18s} {name:19s} {n:6d}  median {row['median_ms']:10.3f} ms  min {row['min_ms']:10.3f}  max {row['max_ms']:10.3f}", flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(dev), "library": os.path.basename(T._ffi.LIB_PATH), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
