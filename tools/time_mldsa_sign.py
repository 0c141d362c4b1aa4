#!/usr/bin/env python3
"""Rates of batched ML-DSA signing (tools_amd/mldsa.py: sign_begin_dev / sign_round_dev / sign_end_dev) for the three parameter sets at 4 096 and
65 536 instances, one key for all (sk_stride = 0) and one key per instance, mu given (PSF_MLDSA_MSG_MU), rnd given.  A call is begin, then rounds with
`active` = the 4 bytes of d_live read back after each round until it is 0, then end, timed on the host clock from before begin to after end (the
read-backs are part of a call); medians of --reps after --warmup.  Per row:
  signatures per second; the mean and maximum attempts (d_rounds) and the number of rounds;
  the time of the first round alone (HIP events around it: every instance is live);
  `full_active`: the same call with active = count in every round (the products run over dead slots too), to show what the shrinking prefix buys;
  `verify_one_key`: psf_mldsa_verify_dev with pk_stride = 0 over the same batch, a yardstick for the work of one round;
  the Keccak permutations per attempt (5 l for ExpandMask, 7 / 7 / 9 for c~, 1 for SampleInBall: 28 / 33 / 45) times the attempts made, at the 5.2 G
  permutations/s that profiles/fips203_timing_run*.json record for SHAKE256 alone, as a fraction of the time.
The share of a call spent in compaction (k_sign_match, k_sign_move, k_sign_commit) is not visible from outside the call: it is read from a kernel
trace of this same script (rocprofv3 --kernel-trace --stats -- python tools/time_mldsa_sign.py ... --shrinking-only --reps 1 --warmup 0), see
profiles/README.md.
The keys are the device's own (keygen_dev); every signature is checked with verify_dev before timing.  No time is a pass condition.

    python tools/time_mldsa_sign.py --out DIR [--name FILE.json] [--reps 3] [--counts 4096,65536] [--sets ML-DSA-44,ML-DSA-65,ML-DSA-87]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KECCAK_PER_S = 5.2e9
# name: (k, l, permutations of the c~ hash: floor((64 + 32 bits k) / 136) + 1)
PARAMS = {"ML-DSA-44": (4, 4, 7), "ML-DSA-65": (6, 5, 7), "ML-DSA-87": (8, 7, 9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="mldsa_sign_timing.json")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--counts", default="4096,65536")
    ap.add_argument("--sets", default=",".join(PARAMS))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shrinking-only", action="store_true", help="for a kernel trace: no check by verify_dev, no full_active calls, no verify yardstick")
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    D = T.mldsa
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for name in a.sets.split(","):
        k, l, ct_perms = PARAMS[name]
        perms = 5 * l + ct_perms + 1
        sz = D.sizes(name)
        for count in (int(c) for c in a.counts.split(",")):
            gen = torch.Generator(device="cuda").manual_seed(20261019 + count)
            xi = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda", generator=gen)
            mu = torch.randint(0, 256, (count, 64), dtype=torch.uint8, device="cuda", generator=gen)
            rnd = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda", generator=gen)
            pk, sk = torch.empty((count, sz["pk"]), dtype=torch.uint8, device="cuda"), torch.empty((count, sz["sk"]), dtype=torch.uint8, device="cuda")
            sig = torch.zeros((count, sz["sig"]), dtype=torch.uint8, device="cuda")
            rounds = torch.zeros(count, dtype=torch.int32, device="cuda")
            ok = torch.empty(count, dtype=torch.uint8, device="cuda")
            live = torch.zeros(1, dtype=torch.int32, device="cuda")
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            host_live = torch.zeros(1, dtype=torch.int32).pin_memory()
            wsb = {"keygen": D.workspace_bytes(name, count, "keygen"), "verify": D.workspace_bytes(name, count, "verify"),
                   0: D.sign_workspace_bytes(name, count, 0), sz["sk"]: D.sign_workspace_bytes(name, count, sz["sk"])}
            ws = torch.empty(max(wsb.values()) + 256, dtype=torch.uint8, device="cuda")
            pws = (ws.data_ptr() + 255) // 256 * 256
            D.keygen_dev(name, count, xi.data_ptr(), pk.data_ptr(), sk.data_ptr(), pws, wsb["keygen"], flag.data_ptr(), a.device, stream)

            def sign(stride, full, first=None):
                """one call; returns the number of rounds; first: a pair of events recorded around the first round"""
                rounds.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                D.sign_begin_dev(name, count, sk.data_ptr(), mu.data_ptr(), 64, pws, wsb[stride], live.data_ptr(), d_rnd=rnd.data_ptr(), sk_stride=stride,
                                 msg_kind=D.MSG_MU, d_fail=flag.data_ptr(), device=a.device, stream=stream)
                now, n = count, 0
                while now:
                    if first and n == 0:
                        first[0].record()
                    D.sign_round_dev(name, count, count if full else now, sig.data_ptr(), pws, wsb[stride], live.data_ptr(), d_rounds=rounds.data_ptr(), sk_stride=stride,
                                     d_fail=flag.data_ptr(), device=a.device, stream=stream)
                    if first and n == 0:
                        first[1].record()
                    host_live.copy_(live, non_blocking=True)
                    torch.cuda.current_stream().synchronize()
                    now, n = int(host_live.item()), n + 1
                D.sign_end_dev(name, count, pws, wsb[stride], sk_stride=stride, device=a.device, stream=stream)
                torch.cuda.synchronize()
                return n, (time.perf_counter() - t0) * 1e3

            def verify():
                D.verify_dev(name, count, pk.data_ptr(), mu.data_ptr(), 64, sig.data_ptr(), ok.data_ptr(), pws, wsb["verify"], pk_stride=0, msg_kind=D.MSG_MU,
                             d_fail=flag.data_ptr(), device=a.device, stream=stream)

            for mode, stride in (("one_key", 0), ("key_per_instance", sz["sk"])):
                sign(stride, False)
                if not a.shrinking_only:
                    D.verify_dev(name, count, pk.data_ptr(), mu.data_ptr(), 64, sig.data_ptr(), ok.data_ptr(), pws, wsb["verify"], pk_stride=stride and sz["pk"],
                                 msg_kind=D.MSG_MU, d_fail=flag.data_ptr(), device=a.device, stream=stream)
                    torch.cuda.synchronize()
                    assert bool(ok.all().item()), (name, count, mode)
                assert int(flag.item()) == 0 and bool((rounds > 0).all().item()), (name, count, mode)
                attempts = rounds.to(torch.float64)
                row = {"set": name, "mode": mode, "count": count, "reps": a.reps, "workspace_bytes": wsb[stride], "mean_attempts": round(float(attempts.mean().item()), 3),
                       "max_attempts": int(rounds.max().item()), "permutations_per_attempt": perms}
                for key, full in (("shrinking", False), ("full_active", True))[:1 if a.shrinking_only else 2]:
                    for _ in range(a.warmup):
                        sign(stride, full)
                    ms, first_ms, n = [], [], 0
                    for _ in range(a.reps):
                        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                        n, t = sign(stride, full, ev)
                        ms.append(t)
                        first_ms.append(ev[0].elapsed_time(ev[1]))
                    med = statistics.median(ms)
                    row[key] = {"rounds": n, "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                                "signatures_per_s": round(count / (med * 1e-3)), "first_round_ms": round(statistics.median(first_ms), 3)}
                vms = [0.0] * (a.warmup + 1)
                for _ in range(0 if a.shrinking_only else a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    verify()
                    e1.record()
                    e1.synchronize()
                    vms.append(e0.elapsed_time(e1))
                row["verify_one_key_ms"] = round(statistics.median(vms[a.warmup:]), 3)
                floor_ms = perms * float(attempts.sum().item()) / KECCAK_PER_S * 1e3
                row["keccak_floor_ms"] = round(floor_ms, 3)
                row["floor_over_time"] = round(floor_ms / row["shrinking"]["median_ms"], 3)
                rows.append(row)
                s, f = row["shrinking"], row.get("full_active", {"median_ms": 0.0})
                print(f"{name:10s} {mode:17s} {count:6d}  {s['median_ms']:9.2f} ms ({s['signatures_per_s'] / 1e3:8.1f} k/s)  attempts mean {row['mean_attempts']:.2f} max "
                      f"{row['max_attempts']:2d}  first round {s['first_round_ms']:7.2f} ms  verify {row['verify_one_key_ms']:7.2f} ms  active = count {f['median_ms']:9.2f} ms"
                      f"  keccak floor {row['floor_over_time']:5.3f} of the time", flush=True)
            del xi, mu, rnd, pk, sk, sig, rounds, ok, ws
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "keccak_permutations_per_s": KECCAK_PER_S, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
