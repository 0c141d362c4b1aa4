#!/usr/bin/env python3
"""Rates of the batched SLH-DSA entry points (tools_amd/slhdsa.py: keygen_dev, verify_dev) for the six SHAKE parameter sets: KeyGen at 64 and 1 024
instances (s sets) or 4 096 and 65 536 (f sets), Verify at 4 096 and 65 536 instances with one key per instance and with one key for all
(pk_stride = 0).  HIP events around each call, warm-up excluded, medians of --reps, operations per second and the workspace size.  Beside each time
stand two yardsticks, neither of them the code under test:
  (a) the permutations of the operation divided by the SHAKE256 rate of psf_keccak_dev on 64-byte inputs and 32-byte outputs (one permutation per
      message), timed in this process alternating call by call with the operation, over as many messages as the operation has permutations -- capped
      at 2^24 messages (1.5 GiB of buffers), beyond which the rate no longer changes;
  (b) the same permutations at the 5.2 G permutations/s that profiles/fips203_timing_run*.json record.
Permutations per operation (DESIGN.md "SLH-DSA"): KeyGen 2^h' (16 len + B(len)) + 2^h' - 1; Verify B_msg + k (1 + a) + B(k) + d (7.5 len + B(len) + h'),
with B(l) = floor((n + 32 + l n) / 136) + 1, B_msg = floor((3 n + msg_len) / 136) + 1 and 7.5 the mean of 15 - digit over a uniform digit (a wave runs
until its longest chain is done, so the device spends more than this count: that is part of what the fraction shows).

KeyGen runs on random seeds.  The public keys and signatures of Verify are random bytes: verification has no early exit and every digit and index
comes out of a hash, so every stage runs as it does for an honest signature up to the last comparison, which fails (the check before timing: ok = 0
for every instance).  That the device verifies honest signatures is tests/test_gpu_slhdsa.py.  No time is a pass condition.  Prints one line per row
and writes slhdsa_timing.json (or --name).

    python tools/time_slhdsa.py --out DIR [--name FILE.json] [--reps 7] [--sets 128s,128f,...] [--ops keygen,verify,verify_one_key] [--counts N,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KECCAK_PER_S = 5.2e9
MSG_LEN = 32
YARDSTICK_CAP = 1 << 24
# name: (n, h, d, h', a, k)
PARAMS = {"SLH-DSA-SHAKE-128s": (16, 63, 7, 9, 12, 14), "SLH-DSA-SHAKE-128f": (16, 66, 22, 3, 6, 33), "SLH-DSA-SHAKE-192s": (24, 63, 7, 9, 14, 17),
          "SLH-DSA-SHAKE-192f": (24, 66, 22, 3, 8, 33), "SLH-DSA-SHAKE-256s": (32, 64, 8, 8, 14, 22), "SLH-DSA-SHAKE-256f": (32, 68, 17, 4, 9, 35)}
KEYGEN_COUNTS = {"s": (64, 1024), "f": (4096, 65536)}
VERIFY_COUNTS = (4096, 65536)


def blocks(n, items):
    """permutations of T_l over `items` n-byte strings: PK.seed || ADRS || items at rate 136"""
    return (n + 32 + items * n) // 136 + 1


def permutations(name, op, msg_len=MSG_LEN):
    n, h, d, hp, a, k = PARAMS[name]
    ln = 2 * n + 3
    if op == "keygen":
        return (1 << hp) * (16 * ln + blocks(n, ln)) + (1 << hp) - 1
    return (3 * n + msg_len) // 136 + 1 + k * (1 + a) + blocks(n, k) + d * (7.5 * ln + blocks(n, ln) + hp)


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
    ap.add_argument("--name", default="slhdsa_timing.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="128s,128f,192s,192f,256s,256f")
    ap.add_argument("--ops", default="keygen,verify,verify_one_key")
    ap.add_argument("--counts", default="", help="instances for every case, instead of the table above (for a kernel trace of one shape)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    D, F = T.slhdsa, T.fips203
    stream = torch.cuda.current_stream().cuda_stream
    ops = a.ops.split(",")
    rows = []

    def u8(*shape, gen=None):
        if gen is None:
            return torch.empty(shape, dtype=torch.uint8, device="cuda")
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)

    for short in a.sets.split(","):
        name = "SLH-DSA-SHAKE-" + short
        n = PARAMS[name][0]
        sz = D.sizes(name)
        given = [int(c) for c in a.counts.split(",") if c]
        cases = [("keygen", c) for c in given or KEYGEN_COUNTS[short[-1]] if "keygen" in ops]
        cases += [(op, c) for c in given or VERIFY_COUNTS for op in ("verify", "verify_one_key") if op in ops]
        for op, count in cases:
            kind = "keygen" if op == "keygen" else "verify"
            gen = torch.Generator(device="cuda").manual_seed(20261019 + count)
            seeds = [u8(count, n, gen=gen) for _ in range(3)]
            pk, sk = u8(count, sz["pk"]), u8(count, sz["sk"])
            wsb = D.workspace_bytes(name, count, kind)
            ws = u8(wsb + 256)
            pws = (ws.data_ptr() + 255) // 256 * 256
            perms = permutations(name, kind)
            messages = int(min(perms * count, YARDSTICK_CAP))
            y_in, y_out = u8(messages, 64, gen=gen), u8(messages, 32)

            def yardstick():
                F.keccak_dev(F.SHAKE256, messages, y_in.data_ptr(), 64, y_out.data_ptr(), 32, device=a.device, stream=stream)

            def keygen():
                D.keygen_dev(name, count, seeds[0].data_ptr(), seeds[1].data_ptr(), seeds[2].data_ptr(), pk.data_ptr(), sk.data_ptr(), pws, wsb, a.device, stream)
            if kind == "keygen":
                call = keygen
            else:
                pk[:] = u8(count, sz["pk"], gen=gen)
                msg, sig, ok = u8(count, MSG_LEN, gen=gen), u8(count, sz["sig"], gen=gen), u8(count)
                stride = sz["pk"] if op == "verify" else 0

                def call():
                    D.verify_dev(name, count, pk.data_ptr(), msg.data_ptr(), MSG_LEN, sig.data_ptr(), ok.data_ptr(), pws, wsb, pk_stride=stride, device=a.device, stream=stream)
                ok.fill_(7)
                call()
                torch.cuda.synchronize()
                assert not bool(ok.any().item()), (name, count, op)
            ms = timed(torch, [(op, call), ("shake256", yardstick)], a.warmup, a.reps)
            med, ymed = statistics.median(ms[op]), statistics.median(ms["shake256"])
            rate = messages / (ymed * 1e-3)
            a_ms, b_ms = perms * count / rate * 1e3, perms * count / KECCAK_PER_S * 1e3
            row = {"set": name, "op": op, "count": count, "reps": a.reps, "workspace_bytes": wsb, "median_ms": round(med, 4),
                   "min_ms": round(min(ms[op]), 4), "max_ms": round(max(ms[op]), 4), "ops_per_s": round(count / (med * 1e-3), 1), "permutations_per_op": perms,
                   "shake256_messages": messages, "shake256_median_ms": round(ymed, 4), "shake256_permutations_per_s": round(rate),
                   "yardstick_a_ms": round(a_ms, 4), "a_over_time": round(a_ms / med, 3), "yardstick_b_ms": round(b_ms, 4), "b_over_time": round(b_ms / med, 3)}
            rows.append(row)
            print(f"{name:19s} {op:15s} {count:6d}  {med:10.3f} ms ({row['ops_per_s']:12.1f} /s)  workspace {row['workspace_bytes'] / 2**20:8.1f} MiB  "
                  f"{perms:9.1f} permutations  (a) {a_ms:9.3f} ms at {rate / 1e9:5.2f} G/s = {row['a_over_time']:5.3f} of the time  (b) {b_ms:9.3f} ms = {row['b_over_time']:5.3f}",
                  flush=True)
            del seeds, pk, sk, ws, y_in, y_out
            if kind == "verify":
                del msg, sig, ok
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "keccak_permutations_per_s": KECCAK_PER_S, "message_bytes": MSG_LEN, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
