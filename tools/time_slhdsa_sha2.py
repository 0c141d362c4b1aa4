#!/usr/bin/env python3
"""Rates of the batched SLH-DSA entry points for the six SHA-2 parameter sets (tools_amd/slhdsa_sha2.py: keygen_dev, verify_dev) at the counts of
tools/time_slhdsa.py: KeyGen at 64 and 1 024 instances (s sets) or 4 096 and 65 536 (f sets), Verify at 4 096 and 65 536 instances with one key per
instance.  In ONE process, alternating call by call, stand beside each operation:
  the SHAKE twin    psf_slhdsa_keygen_dev / psf_slhdsa_verify_dev of the SHAKE set with the same (n, h, d, h', a, k), same count, same inputs
  the yardsticks    psf_sha2_dev on one-block messages (32 bytes in, 32 out for SHA-256; 64 in, 64 out for SHA-512: one compression per message), over
                    2^22 messages each, SHA-256 and SHA-512 separately; the operation's compressions at those two rates is the yardstick time
HIP events around each call, warm-up excluded, medians of --reps.  Compressions per operation are the closed formulas of DESIGN.md "SLH-DSA: the SHA-2
sets" (tests/test_slhdsa_sha2_cpu.py checks them against the core), with 7.5 = the mean of 15 - digit for the chain steps of Verify.

Before anything is timed, KeyGen of three seed triples and Verify of an honest and a tampered signature of the pure-Python model
(tests/helpers/slhdsa_sha2_model.py) are compared with the model on SLH-DSA-SHA2-128f.  KeyGen then runs on random seeds, Verify on random keys and
signatures (no early exit: every stage runs as for an honest signature, and the check before timing is ok = 0 for every instance).  No time is a pass
condition.  Prints one line per row and writes slhdsa_sha2_timing.json (or --name).

    python tools/time_slhdsa_sha2.py --out DIR [--name FILE.json] [--reps 7] [--sets 128s,128f,...] [--ops keygen,verify] [--counts N,...] [--no-twin]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MSG_LEN = 32
YARDSTICK_MESSAGES = 1 << 22
# short name: (n, h, d, h', a, k)
PARAMS = {"128s": (16, 63, 7, 9, 12, 14), "128f": (16, 66, 22, 3, 6, 33), "192s": (24, 63, 7, 9, 14, 17), "192f": (24, 66, 22, 3, 8, 33),
          "256s": (32, 64, 8, 8, 14, 22), "256f": (32, 68, 17, 4, 9, 35)}
KEYGEN_COUNTS = {"s": (64, 1024), "f": (4096, 65536)}
VERIFY_COUNTS = (4096, 65536)


def t_blocks(n, items):
    """compressions of T_l past the midstate over `items` n-byte strings"""
    block, pad = (64, 9) if n == 16 else (128, 17)
    return -(-(22 + items * n + pad) // block)


def compressions(short, op, msg_len=MSG_LEN):
    """(SHA-256, SHA-512) per operation, the midstates of every stage counted once per key"""
    n, h, d, hp, a, k = PARAMS[short]
    ln, leaves = 2 * n + 3, 1 << hp
    if op == "keygen":
        chains, rest = 1 + leaves * ln * 16, (1 + leaves * t_blocks(n, ln)) + (1 + leaves - 1)
        return (chains + rest, 0) if n == 16 else (chains, rest)
    steps = 7.5 * ln * d
    if n == 16:
        return -(-(3 * n + msg_len + 9) // 64) + 3 + (1 + k + k * a) + (1 + t_blocks(n, k)) + d * (2 + t_blocks(n, ln) + hp) + steps, 0
    digest = -(-(3 * n + msg_len + 17) // 128) + -(-(2 * n + 68 + 17) // 128)
    return (1 + k) + d + steps, digest + (1 + k * a) + (1 + t_blocks(n, k)) + d * (1 + t_blocks(n, ln) + hp)


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


def check_against_the_model(torch, D):
    """KeyGen and Verify of one small batch on SLH-DSA-SHA2-128f equal the model"""
    import random
    from tests.helpers import slhdsa_sha2_model as M
    name, n = "SLH-DSA-SHA2-128f", 16
    rng = random.Random(20261020)
    seeds = [[rng.randbytes(n) for _ in range(3)] for _ in range(3)]
    got = D.keygen_internal(name, *seeds)
    want = [M.keygen_internal(name, a, b, c) for a, b, c in zip(*seeds)]
    assert got == [(pk, sk) for sk, pk in want], "KeyGen differs from the model"
    pk, sk = got[0]
    msg = rng.randbytes(MSG_LEN)
    sig = M.sign_internal(name, msg, sk, rng.randbytes(n))
    bad = bytes([sig[100] ^ 1 if i == 100 else b for i, b in enumerate(sig)])
    assert D.verify_internal(name, pk, [msg, msg], [sig, bad]) == [True, False] == [M.verify_internal(name, msg, s, pk) for s in (sig, bad)], "Verify differs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="slhdsa_sha2_timing.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="128s,128f,192s,192f,256s,256f")
    ap.add_argument("--ops", default="keygen,verify")
    ap.add_argument("--counts", default="", help="instances for every case, instead of the table above (for a kernel trace of one shape)")
    ap.add_argument("--no-twin", action="store_true", help="the SHA-2 operation alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    D2, D1, H = T.slhdsa_sha2, T.slhdsa, T.sha2
    check_against_the_model(torch, D2)
    stream = torch.cuda.current_stream().cuda_stream
    ops = a.ops.split(",")
    rows = []

    def u8(*shape, gen=None):
        if gen is None:
            return torch.empty(shape, dtype=torch.uint8, device="cuda")
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)

    ygen = torch.Generator(device="cuda").manual_seed(7)
    y256_in, y256_out = u8(YARDSTICK_MESSAGES, 32, gen=ygen), u8(YARDSTICK_MESSAGES, 32)
    y512_in, y512_out = u8(YARDSTICK_MESSAGES, 64, gen=ygen), u8(YARDSTICK_MESSAGES, 64)

    def yard256():
        H.sha2_dev(H.SHA2_256, YARDSTICK_MESSAGES, y256_in.data_ptr(), 32, y256_out.data_ptr(), 32, device=a.device, stream=stream)

    def yard512():
        H.sha2_dev(H.SHA2_512, YARDSTICK_MESSAGES, y512_in.data_ptr(), 64, y512_out.data_ptr(), 64, device=a.device, stream=stream)

    for short in a.sets.split(","):
        name2, name1 = "SLH-DSA-SHA2-" + short, "SLH-DSA-SHAKE-" + short
        n = PARAMS[short][0]
        sz = D2.sizes(name2)
        assert sz == D1.sizes(name1)
        given = [int(c) for c in a.counts.split(",") if c]
        cases = [("keygen", c) for c in given or KEYGEN_COUNTS[short[-1]] if "keygen" in ops]
        cases += [("verify", c) for c in given or VERIFY_COUNTS if "verify" in ops]
        for op, count in cases:
            gen = torch.Generator(device="cuda").manual_seed(20261020 + count)
            seeds = [u8(count, n, gen=gen) for _ in range(3)]
            pk, sk = u8(count, sz["pk"]), u8(count, sz["sk"])
            wsb = max(D2.workspace_bytes(name2, count, op), D1.workspace_bytes(name1, count, op))
            ws = u8(wsb + 256)
            pws = (ws.data_ptr() + 255) // 256 * 256
            if op == "keygen":
                def call(D, name):
                    D.keygen_dev(name, count, seeds[0].data_ptr(), seeds[1].data_ptr(), seeds[2].data_ptr(), pk.data_ptr(), sk.data_ptr(), pws, wsb, a.device, stream)
            else:
                pk[:] = u8(count, sz["pk"], gen=gen)
                msg, sig, ok = u8(count, MSG_LEN, gen=gen), u8(count, sz["sig"], gen=gen), u8(count)

                def call(D, name):
                    D.verify_dev(name, count, pk.data_ptr(), msg.data_ptr(), MSG_LEN, sig.data_ptr(), ok.data_ptr(), pws, wsb, device=a.device, stream=stream)
                ok.fill_(7)
                call(D2, name2)
                torch.cuda.synchronize()
                assert not bool(ok.any().item()), (name2, count, op)
            members = [("sha2", lambda: call(D2, name2))]
            if not a.no_twin:
                members += [("shake", lambda: call(D1, name1)), ("sha256", yard256), ("sha512", yard512)]
            ms = timed(torch, members, a.warmup, a.reps)
            med = statistics.median(ms["sha2"])
            c256, c512 = compressions(short, op)
            row = {"set": name2, "op": op, "count": count, "reps": a.reps, "workspace_bytes": D2.workspace_bytes(name2, count, op), "median_ms": round(med, 4),
                   "min_ms": round(min(ms["sha2"]), 4), "max_ms": round(max(ms["sha2"]), 4), "ops_per_s": round(count / (med * 1e-3), 1),
                   "sha256_per_op": c256, "sha512_per_op": c512, "sha256_per_s": round(c256 * count / (med * 1e-3)), "sha512_per_s": round(c512 * count / (med * 1e-3))}
            line = f"{name2:18s} {op:7s} {count:6d}  {med:10.3f} ms ({row['ops_per_s']:12.1f} /s)  {c256:10.1f} SHA-256 + {c512:8.1f} SHA-512 per op"
            if not a.no_twin:
                twin, y256, y512 = (statistics.median(ms[k]) for k in ("shake", "sha256", "sha512"))
                r256, r512 = YARDSTICK_MESSAGES / (y256 * 1e-3), YARDSTICK_MESSAGES / (y512 * 1e-3)
                yard = (c256 * count / r256 + c512 * count / r512) * 1e3
                row.update({"shake_median_ms": round(twin, 4), "shake_min_ms": round(min(ms["shake"]), 4), "shake_max_ms": round(max(ms["shake"]), 4),
                            "sha2_over_shake": round(med / twin, 3), "yardstick_sha256_per_s": round(r256), "yardstick_sha512_per_s": round(r512),
                            "yardstick_ms": round(yard, 4), "yardstick_over_time": round(yard / med, 3)})
                line += (f"  SHAKE twin {twin:10.3f} ms: SHA-2 / SHAKE = {row['sha2_over_shake']:5.3f}  yardstick {yard:9.3f} ms at {r256 / 1e9:5.2f} / {r512 / 1e9:5.2f} G/s"
                         f" = {row['yardstick_over_time']:5.3f} of the time")
            rows.append(row)
            print(line, flush=True)
            del seeds, pk, sk, ws
            if op == "verify":
                del msg, sig, ok
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "message_bytes": MSG_LEN, "yardstick_messages": YARDSTICK_MESSAGES, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
