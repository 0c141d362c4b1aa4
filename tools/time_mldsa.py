#!/usr/bin/env python3
"""Rates of the batched ML-DSA entry points (tools_amd/mldsa.py: keygen_dev, verify_dev) for the three parameter sets at 4 096 and 65 536 instances:
KeyGen, Verify with one key per instance and Verify with one key for all (pk_stride = 0), both with mu given (PSF_MLDSA_MSG_MU).  HIP events around
each call, warm-up excluded, medians of --reps.  Beside each time stands the Keccak-only floor: the permutations of the operation as DESIGN.md
"ML-DSA" derives them from the byte counts, at the 5.2 G permutations/s that profiles/fips203_timing_run*.json record for SHAKE256 alone, and the
fraction floor / time.

The keys are the device's own (keygen_dev).  The signatures are well formed and do not verify: random c~ and z bytes and an empty hint, so every
stage runs as it does for an honest signature up to the last comparison, which fails (the check before timing: ok = 0 and no PSF_MLDSA_WHY_HINT for
every instance).  No time is a pass condition.  Prints one line per row and writes mldsa_timing.json (or --name).

    python tools/time_mldsa.py --out DIR [--name FILE.json] [--reps 9] [--counts 4096,65536]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KECCAK_PER_S = 5.2e9
# name: (k, l, lambda / 4, w1 bits, omega)
PARAMS = {"ML-DSA-44": (4, 4, 32, 6, 80), "ML-DSA-65": (6, 5, 48, 4, 55), "ML-DSA-87": (8, 7, 64, 4, 75)}


def permutations(name, op, pk_len):
    """Keccak-f[1600] calls per instance (DESIGN.md "ML-DSA"): an absorb of n bytes at rate r takes floor(n / r) + 1; RejNTTPoly reads 5 blocks of
    SHAKE128, RejBoundedPoly 2 of SHAKE256 (a wave runs until its last lane is done), SampleInBall 1"""
    k, l, cb, bits, omega = PARAMS[name]
    expand_a = 5 * k * l
    if op == "keygen":
        return 1 + expand_a + 2 * (k + l) + pk_len // 136 + 1
    tail = (64 + 32 * bits * k) // 136 + 1
    return (expand_a if op == "verify" else 0) + 1 + tail


def timed(torch, f, warmup, reps):
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
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="mldsa_timing.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--counts", default="4096,65536")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    D = T.mldsa
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, (k, l, cb, bits, omega) in PARAMS.items():
        sz = D.sizes(name)
        for count in (int(c) for c in a.counts.split(",")):
            gen = torch.Generator(device="cuda").manual_seed(20261019 + count)
            xi = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda", generator=gen)
            mu = torch.randint(0, 256, (count, 64), dtype=torch.uint8, device="cuda", generator=gen)
            sig = torch.randint(0, 256, (count, sz["sig"]), dtype=torch.uint8, device="cuda", generator=gen)
            sig[:, sz["sig"] - omega - k:] = 0                             # HintBitPack of an all-zero hint
            pk, sk = torch.empty((count, sz["pk"]), dtype=torch.uint8, device="cuda"), torch.empty((count, sz["sk"]), dtype=torch.uint8, device="cuda")
            ok, why = torch.empty(count, dtype=torch.uint8, device="cuda"), torch.empty(count, dtype=torch.uint8, device="cuda")
            wsb = {op: D.workspace_bytes(name, count, op) for op in ("keygen", "verify")}
            ws = torch.empty(max(wsb.values()) + 256, dtype=torch.uint8, device="cuda")
            pws = (ws.data_ptr() + 255) // 256 * 256
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")

            def verify(stride):
                D.verify_dev(name, count, pk.data_ptr(), mu.data_ptr(), 64, sig.data_ptr(), ok.data_ptr(), pws, wsb["verify"], d_why=why.data_ptr(),
                             pk_stride=stride, msg_kind=D.MSG_MU, d_fail=flag.data_ptr(), device=a.device, stream=stream)
            calls = {
                "keygen": lambda: D.keygen_dev(name, count, xi.data_ptr(), pk.data_ptr(), sk.data_ptr(), pws, wsb["keygen"], flag.data_ptr(), a.device, stream),
                "verify": lambda: verify(sz["pk"]),
                "verify_one_key": lambda: verify(0),
            }
            calls["keygen"]()
            for op in ("verify", "verify_one_key"):
                calls[op]()
                torch.cuda.synchronize()
                assert not bool(ok.any().item()) and not bool((why & D.WHY_HINT).any().item()) and bool((why & D.WHY_HASH).all().item()), (name, count, op)
            assert int(flag.item()) == 0, (name, count)
            for op, f in calls.items():
                ms = timed(torch, f, a.warmup, a.reps)
                med = statistics.median(ms)
                perms = permutations(name, op, sz["pk"])
                floor_ms = perms * count / KECCAK_PER_S * 1e3
                row = {"set": name, "op": op, "count": count, "reps": a.reps, "workspace_bytes": wsb["keygen" if op == "keygen" else "verify"],
                       "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "ops_per_s": round(count / (med * 1e-3)),
                       "permutations_per_op": perms, "keccak_floor_ms": round(floor_ms, 4), "floor_over_time": round(floor_ms / med, 3)}
                rows.append(row)
                print(f"{name:10s} {op:15s} {count:6d}  {med:9.3f} ms ({row['ops_per_s'] / 1e6:7.3f} M/s)  workspace {row['workspace_bytes'] / 2**20:8.1f} MiB"
                      f"  {perms:4d} permutations, floor {floor_ms:8.3f} ms = {row['floor_over_time']:5.3f} of the time", flush=True)
            del xi, mu, sig, pk, sk, ok, why, ws
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "keccak_permutations_per_s": KECCAK_PER_S, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
