#!/usr/bin/env python3
"""Rates of batched SLH-DSA signing for the six SHA-2 parameter sets (tools_amd/slhdsa_sha2.py: sign_dev) beside their SHAKE twins (tools_amd/slhdsa.py:
sign_dev): 64 and 1 024 instances for the s sets, 1 024 and 16 384 for the f sets (at 16 384 the workspace of 256f is 9 GiB), with one key per instance
and with one key for all (sk_stride = 0), hedged.  The SHA-2 call and the twin's call alternate call by call in one process, each between HIP events,
warm-up excluded; medians of --reps, signatures per second, the ratio of the two medians, and the SHA-256 / SHA-512 compressions of a signature
(DESIGN.md "SLH-DSA: signing for the SHA-2 sets", every lane's midstate included, the mean digit 7.5).

The keys of either family are made by its keygen_dev from the same random seeds.  Before timing, the SHA-2 signatures of one batch per set are verified
with slhdsa_sha2.verify_dev: every ok is 1, and the workspace is all zero.  That the bytes are the model's is tests/test_gpu_slhdsa_sha2_sign.py.  No
time is a pass condition.  Prints one line per row and writes slhdsa_sha2_sign_timing.json (or --name).

    python tools/time_slhdsa_sha2_sign.py --out DIR [--name FILE.json] [--reps 7] [--sets 128s,128f,...] [--ops sign,sign_one_key] [--counts N,...]
                                          [--no-twin]     (the SHA-2 calls alone: for a kernel trace of one shape)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_slhdsa as Y  # noqa: E402  (PARAMS, MSG_LEN, timed)

MSG_LEN = Y.MSG_LEN
SIGN_COUNTS = {"s": (64, 1024), "f": (1024, 16384)}


def _ceil(a, b):
    return -(-a // b)


def compressions(short, msg_len=MSG_LEN):
    """{"sha256", "sha512"} compressions of one signature on the device, by stage: every lane makes its midstate(s), and a signed digit is 7.5 on average"""
    n, h, d, hp, a, k = Y.PARAMS["SLH-DSA-SHAKE-" + short]
    ln, leaves = 2 * n + 3, 1 << hp
    wide = n > 16
    blk, pad = (128, 17) if wide else (64, 9)
    fors_wgs = k << (a - 9) if a >= 9 else _ceil(k, 1 << (9 - a))
    f = {"fors": 2 * (k << a) + 256 * fors_wgs, "chains": 17 * d * leaves * ln, "wots": (2 + 7.5) * d * ln}
    hh = {"prf_msg": 3 + _ceil(n + msg_len + pad, blk), "digest": _ceil(3 * n + msg_len + pad, blk) + (2 if wide else 3),
          "fors": k * ((1 << a) - 1) + (256 * fors_wgs if wide else 0), "fors_top": k * (1 + (1 << (a - 9)) - 1) if a > 9 else 0,
          "fors_pk": 1 + _ceil(22 + k * n + pad, blk), "leaf": d * leaves * (1 + _ceil(22 + ln * n + pad, blk)), "tree": d * (leaves - 1) + d * leaves / 2}
    if a > 9:
        hh["fors"] = k * ((1 << a) - (1 << (a - 9))) + (256 * fors_wgs if wide else 0)
    both = {"sha256": dict(f), "sha512": {}}
    both["sha512" if wide else "sha256"].update({("h_" + s if s in f else s): v for s, v in hh.items()})
    return {fam: {"stages": st, "total": sum(st.values())} for fam, st in both.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="slhdsa_sha2_sign_timing.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="128s,128f,192s,192f,256s,256f")
    ap.add_argument("--ops", default="sign,sign_one_key")
    ap.add_argument("--counts", default="", help="instances for every case, instead of the table above (for a kernel trace of one shape)")
    ap.add_argument("--no-twin", action="store_true", help="time the SHA-2 calls alone")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import tools_amd as T
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    torch.cuda.set_device(a.device)
    stream = torch.cuda.current_stream().cuda_stream
    ops = a.ops.split(",")
    rows = []

    def u8(*shape, gen=None):
        if gen is None:
            return torch.empty(shape, dtype=torch.uint8, device="cuda")
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)

    for short in a.sets.split(","):
        fams = [("sha2", T.slhdsa_sha2, "SLH-DSA-SHA2-" + short)] + ([] if a.no_twin else [("shake", T.slhdsa, "SLH-DSA-SHAKE-" + short)])
        n = Y.PARAMS["SLH-DSA-SHAKE-" + short][0]
        sz = T.slhdsa_sha2.sizes(fams[0][2])
        given = [int(c) for c in a.counts.split(",") if c]
        checked = False
        for count in given or SIGN_COUNTS[short[-1]]:
            gen = torch.Generator(device="cuda").manual_seed(20261020 + count)
            seeds = [u8(count, n, gen=gen) for _ in range(3)]
            keys = {}
            for tag, D, name in fams:
                pk, sk = u8(count, sz["pk"]), u8(count, sz["sk"])
                kws = u8(D.workspace_bytes(name, count, "keygen") + 256)
                D.keygen_dev(name, count, seeds[0].data_ptr(), seeds[1].data_ptr(), seeds[2].data_ptr(), pk.data_ptr(), sk.data_ptr(),
                             (kws.data_ptr() + 255) // 256 * 256, kws.numel() - 256, a.device, stream)
                torch.cuda.synchronize()
                keys[tag] = (pk, sk)
                del kws
            del seeds
            torch.cuda.empty_cache()
            msg, rnd, sig = u8(count, MSG_LEN, gen=gen), u8(count, n, gen=gen), u8(count, sz["sig"])
            wsb = T.slhdsa_sha2.sign_workspace_bytes(fams[0][2], count)
            assert all(D.sign_workspace_bytes(name, count) == wsb for _, D, name in fams)
            ws = u8(wsb + 256)                                             # one workspace and one signature buffer serve both: the calls are ordered on one stream
            pws = (ws.data_ptr() + 255) // 256 * 256
            for op in [o for o in ("sign", "sign_one_key") if o in ops]:
                stride = sz["sk"] if op == "sign" else 0

                def caller(D, name, sk):
                    return lambda: D.sign_dev(name, count, sk.data_ptr(), msg.data_ptr(), MSG_LEN, rnd.data_ptr(), sig.data_ptr(), pws, wsb, sk_stride=stride,
                                              device=a.device, stream=stream)
                members = [(tag, caller(D, name, keys[tag][1])) for tag, D, name in fams]
                if not checked:                                            # one batch per set: the device accepts what it signed, under either stride
                    D, name = fams[0][1], fams[0][2]
                    vws = u8(D.workspace_bytes(name, count, "verify") + 256)
                    ok = u8(count)
                    ok.fill_(7)
                    members[0][1]()
                    D.verify_dev(name, count, keys["sha2"][0].data_ptr(), msg.data_ptr(), MSG_LEN, sig.data_ptr(), ok.data_ptr(), (vws.data_ptr() + 255) // 256 * 256,
                                 vws.numel() - 256, pk_stride=sz["pk"] if stride else 0, device=a.device, stream=stream)
                    torch.cuda.synchronize()
                    assert bool((ok == 1).all().item()), (name, count, op)
                    assert not bool(ws[pws - ws.data_ptr():pws - ws.data_ptr() + wsb].any().item()), (name, count, op, "workspace not cleared")
                    del vws, ok
                ms = Y.timed(torch, members, a.warmup, a.reps)
                med = statistics.median(ms["sha2"])
                row = {"set": fams[0][2], "op": op, "count": count, "reps": a.reps, "workspace_bytes": wsb, "median_ms": round(med, 4), "min_ms": round(min(ms["sha2"]), 4),
                       "max_ms": round(max(ms["sha2"]), 4), "ops_per_s": round(count / (med * 1e-3), 1), "compressions_per_op": compressions(short)}
                text = ""
                if not a.no_twin:
                    tmed = statistics.median(ms["shake"])
                    row.update({"shake_median_ms": round(tmed, 4), "shake_min_ms": round(min(ms["shake"]), 4), "shake_max_ms": round(max(ms["shake"]), 4),
                                "sha2_over_shake": round(med / tmed, 3), "not_slower_than_the_twin": bool(med <= tmed)})
                    text = f"  twin {tmed:10.3f} ms  sha2 / shake {med / tmed:5.3f}"
                rows.append(row)
                print(f"{fams[0][2]:18s} {op:13s} {count:6d}  {med:10.3f} ms ({row['ops_per_s']:10.1f} /s)  workspace {wsb / 2**20:8.1f} MiB{text}", flush=True)
            checked = True
            del keys, msg, rnd, sig, ws
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "message_bytes": MSG_LEN, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
