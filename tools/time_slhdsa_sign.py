#!/usr/bin/env python3
"""Rates of batched SLH-DSA signing (tools_amd/slhdsa.py: sign_dev) for the six SHAKE parameter sets: 64 and 1 024 instances for the s sets, 1 024 and
16 384 for the f sets (at 16 384 the workspace of 256f is 9 GiB), with one key per instance and with one key for all (sk_stride = 0), hedged.  HIP
events around each call, warm-up excluded, medians of --reps, signatures per second and the workspace size.  Beside each time stand the two yardsticks
of tools/time_slhdsa.py, whose code this tool reuses, neither of them the code under test:
  (a) the permutations of a signature at the SHAKE256 rate of psf_keccak_dev, timed in this process alternating call by call with the signing call;
  (b) the same permutations at 5.2 G permutations/s.
Permutations per signature (DESIGN.md "SLH-DSA: signing"): B_prf + B_msg + k (3 2^a - 1) + B(k) + d KeyGen + 8.5 d len, with
B_prf = floor((2 n + msg_len) / 136) + 1, KeyGen and the rest as in tools/time_slhdsa.py, and 8.5 = 1 + the mean digit.

The keys are made by keygen_dev from random seeds.  Before timing, the signatures of one batch per set are verified with verify_dev: every ok is 1.
That the bytes are the model's is tests/test_gpu_slhdsa_sign.py.  No time is a pass condition.  Prints one line per row and writes
slhdsa_sign_timing.json (or --name).

    python tools/time_slhdsa_sign.py --out DIR [--name FILE.json] [--reps 7] [--sets 128s,128f,...] [--ops sign,sign_one_key] [--counts N,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_slhdsa as Y  # noqa: E402  (the yardstick code: PARAMS, blocks, permutations, timed)

MSG_LEN = Y.MSG_LEN
SIGN_COUNTS = {"s": (64, 1024), "f": (1024, 16384)}


def stages(name, msg_len=MSG_LEN):
    """permutations of one signature by stage: {"digest", "fors", "trees", "wots"}"""
    n, h, d, hp, a, k = Y.PARAMS[name]
    ln = 2 * n + 3
    return {"digest": (2 * n + msg_len) // 136 + 1 + (3 * n + msg_len) // 136 + 1, "fors": k * (3 * (1 << a) - 1) + Y.blocks(n, k),
            "trees": d * Y.permutations(name, "keygen"), "wots": 8.5 * d * ln}


def permutations(name, msg_len=MSG_LEN):
    return sum(stages(name, msg_len).values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="slhdsa_sign_timing.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="128s,128f,192s,192f,256s,256f")
    ap.add_argument("--ops", default="sign,sign_one_key")
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
        n = Y.PARAMS[name][0]
        sz = D.sizes(name)
        given = [int(c) for c in a.counts.split(",") if c]
        checked = False
        for count in given or SIGN_COUNTS[short[-1]]:
            gen = torch.Generator(device="cuda").manual_seed(20261020 + count)
            seeds = [u8(count, n, gen=gen) for _ in range(3)]
            pk, sk = u8(count, sz["pk"]), u8(count, sz["sk"])
            kws = u8(D.workspace_bytes(name, count, "keygen") + 256)
            D.keygen_dev(name, count, seeds[0].data_ptr(), seeds[1].data_ptr(), seeds[2].data_ptr(), pk.data_ptr(), sk.data_ptr(),
                         (kws.data_ptr() + 255) // 256 * 256, kws.numel() - 256, a.device, stream)
            torch.cuda.synchronize()
            del kws, seeds
            torch.cuda.empty_cache()
            msg, rnd, sig = u8(count, MSG_LEN, gen=gen), u8(count, n, gen=gen), u8(count, sz["sig"])
            wsb = D.sign_workspace_bytes(name, count)
            ws = u8(wsb + 256)
            pws = (ws.data_ptr() + 255) // 256 * 256
            perms = permutations(name)
            messages = int(min(perms * count, Y.YARDSTICK_CAP))
            y_in, y_out = u8(messages, 64, gen=gen), u8(messages, 32)

            def yardstick():
                F.keccak_dev(F.SHAKE256, messages, y_in.data_ptr(), 64, y_out.data_ptr(), 32, device=a.device, stream=stream)

            for op in [o for o in ("sign", "sign_one_key") if o in ops]:
                stride = sz["sk"] if op == "sign" else 0

                def call():
                    D.sign_dev(name, count, sk.data_ptr(), msg.data_ptr(), MSG_LEN, rnd.data_ptr(), sig.data_ptr(), pws, wsb, sk_stride=stride, device=a.device, stream=stream)
                if not checked:                                            # one batch per set: the device accepts what it signed, under either stride
                    vws = u8(D.workspace_bytes(name, count, "verify") + 256)
                    ok = u8(count)
                    ok.fill_(7)
                    call()
                    D.verify_dev(name, count, pk.data_ptr(), msg.data_ptr(), MSG_LEN, sig.data_ptr(), ok.data_ptr(), (vws.data_ptr() + 255) // 256 * 256, vws.numel() - 256,
                                 pk_stride=sz["pk"] if stride else 0, device=a.device, stream=stream)
                    torch.cuda.synchronize()
                    assert bool((ok == 1).all().item()), (name, count, op)
                    assert not bool(ws[pws - ws.data_ptr():pws - ws.data_ptr() + wsb].any().item()), (name, count, op, "workspace not cleared")
                    del vws, ok
                ms = Y.timed(torch, [(op, call), ("shake256", yardstick)], a.warmup, a.reps)
                med, ymed = statistics.median(ms[op]), statistics.median(ms["shake256"])
                rate = messages / (ymed * 1e-3)
                a_ms, b_ms = perms * count / rate * 1e3, perms * count / Y.KECCAK_PER_S * 1e3
                row = {"set": name, "op": op, "count": count, "reps": a.reps, "workspace_bytes": wsb, "median_ms": round(med, 4), "min_ms": round(min(ms[op]), 4),
                       "max_ms": round(max(ms[op]), 4), "ops_per_s": round(count / (med * 1e-3), 1), "permutations_per_op": perms,
                       "permutations_per_s": round(perms * count / (med * 1e-3)), "stages": stages(name), "shake256_messages": messages,
                       "shake256_median_ms": round(ymed, 4), "shake256_permutations_per_s": round(rate), "yardstick_a_ms": round(a_ms, 4),
                       "a_over_time": round(a_ms / med, 3), "yardstick_b_ms": round(b_ms, 4), "b_over_time": round(b_ms / med, 3)}
                rows.append(row)
                print(f"{name:19s} {op:13s} {count:6d}  {med:10.3f} ms ({row['ops_per_s']:10.1f} /s, {row['permutations_per_s'] / 1e9:5.2f} G perm/s)  workspace "
                      f"{wsb / 2**20:8.1f} MiB  {perms:9.1f} permutations  (a) {a_ms:9.3f} ms at {rate / 1e9:5.2f} G/s = {row['a_over_time']:5.3f} of the time  "
                      f"(b) {b_ms:9.3f} ms = {row['b_over_time']:5.3f}", flush=True)
            checked = True
            del pk, sk, msg, rnd, sig, ws, y_in, y_out
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "keccak_permutations_per_s": Y.KECCAK_PER_S, "message_bytes": MSG_LEN, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
