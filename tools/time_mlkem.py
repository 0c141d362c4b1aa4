#!/usr/bin/env python3
"""Rates of the batched ML-KEM entry points (tools_amd/mlkem.py: keygen_dev, encaps_dev, decaps_dev) for the three parameter sets at 4 096 and
65 536 instances, each beside the COMPOSED route: the same algorithm as a caller of the library without these entry points would write it --
the device calls of tests/test_gpu_fips203.py::test_kpke_in_device_calls_equals_the_model_bytes (16-bit words), with psf_keccak_dev for
G, H and J and torch for the glue (cat, where, slices made contiguous, the comparison and selection of decapsulation).  Both run in this process,
alternating call by call; HIP events around each call, warm-up excluded, medians of --reps.  Before timing, the outputs of the two routes are
compared once and must be equal.  No time is a pass condition.  Prints one line per row and writes mlkem_timing.json (or --name).

    python tools/time_mlkem.py --out DIR [--name FILE.json] [--reps 9] [--counts 4096,65536]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, N = 3329, 256
PARAMS = {"ML-KEM-512": (2, 3, 2, 10, 4), "ML-KEM-768": (3, 2, 2, 10, 4), "ML-KEM-1024": (4, 2, 2, 11, 5)}


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


class Composed:
    """ML-KEM from the library's lower entry points and torch, 16-bit words; every tensor is (count, ...) uint8 / int16 / int32 on the device"""

    def __init__(self, torch, T, name, device, stream):
        self.t, self.T, self.F, self.C = torch, T, T.fips203, T.compression
        self.k, self.eta1, self.eta2, self.du, self.dv = PARAMS[name]
        self.dev, self.st = device, stream

    def u8(self, *shape):
        return self.t.empty(shape, dtype=self.t.uint8, device="cuda")

    def words(self, *shape):
        return self.t.empty(shape, dtype=self.t.int16, device="cuda")

    def images(self, *shape):
        return self.t.empty(shape, dtype=self.t.int32, device="cuda")

    def hash(self, func, x, out_len):
        x = x.contiguous()
        out = self.u8(x.shape[0], out_len)
        self.F.keccak_dev(func, x.shape[0], x.data_ptr(), x.shape[1], out.data_ptr(), out_len, device=self.dev, stream=self.st)
        return out

    def fma(self, hat, b, e, c, B, rows, inner, hat_stride, trans=0, sign=1):
        self.T.rq.matpoly_mul_add_hat_dev(hat.data_ptr(), b.data_ptr(), e.data_ptr(), c.data_ptr(), Q, N, B, rows, inner, 1, hat_stride=hat_stride, trans_a=trans,
                                          sign=sign, io_bits=16, device=self.dev, stream=self.st)

    def matrix(self, rho, B):
        k, F = self.k, self.F
        rho = rho.contiguous()
        a_fips, a_hat = self.words(B, k, k, N), self.images(B, k, k, N)
        F.sample_ntt_dev(a_fips.data_ptr(), B, rho.data_ptr(), k=k, io_bits=16, device=self.dev, stream=self.st)
        F.image_from_fips203_dev(a_hat.data_ptr(), B * k * k, a_fips.data_ptr(), io_bits=16, device=self.dev, stream=self.st)
        return a_hat

    def keygen(self, d, z):
        t, k, F, B = self.t, self.k, self.F, d.shape[0]
        g = self.hash(F.SHA3_512, t.cat([d, t.full((B, 1), k, dtype=t.uint8, device="cuda")], dim=1), 64)
        a_hat = self.matrix(g[:, :32], B)
        s, e, tt = self.words(B, k, N), self.words(B, k, N), self.words(B, k, N)
        F.sample_cbd_dev(s.data_ptr(), B, g.data_ptr() + 32, self.eta1, first_nonce=0, per_seed=k, sigma_stride=64, io_bits=16, device=self.dev, stream=self.st)
        F.sample_cbd_dev(e.data_ptr(), B, g.data_ptr() + 32, self.eta1, first_nonce=k, per_seed=k, sigma_stride=64, io_bits=16, device=self.dev, stream=self.st)
        self.fma(a_hat, s, e, tt, B, k, k, k * k * N)
        s_mod = t.where(s < 0, s + Q, s).contiguous()
        st_hat, st_fips = self.images(2, B, k, N), self.words(2, B, k, N)
        self.T.gadget.ntt_forward_dev(tt.data_ptr(), st_hat[0].data_ptr(), Q, N, B * k, io_bits=16, device=self.dev, stream=self.st)
        self.T.gadget.ntt_forward_dev(s_mod.data_ptr(), st_hat[1].data_ptr(), Q, N, B * k, io_bits=16, device=self.dev, stream=self.st)
        F.image_to_fips203_dev(st_fips.data_ptr(), 2 * B * k, st_hat.data_ptr(), io_bits=16, device=self.dev, stream=self.st)
        key = self.u8(2, B, 384 * k)
        self.C.byte_encode_dev(st_fips.data_ptr(), key.data_ptr(), 12, 2 * B * k * N, io_bits=16, device=self.dev, stream=self.st)
        ek = t.cat([key[0], g[:, :32]], dim=1).contiguous()
        dk = t.cat([key[1], ek, self.hash(F.SHA3_256, ek, 32), z], dim=1).contiguous()
        return ek, dk

    def encrypt(self, ek, m, r, B):
        """c = K-PKE.Encrypt(ek, m, r); r may be a view with a row stride"""
        t, k, F, C = self.t, self.k, self.F, self.C
        a_hat = self.matrix(ek[:, 384 * k:], B)
        t_fips, t_hat = self.words(B, k, N), self.images(B, k, N)
        ek_t = ek[:, :384 * k].contiguous()
        C.byte_decode_dev(ek_t.data_ptr(), t_fips.data_ptr(), Q, 12, B * k * N, io_bits=16, device=self.dev, stream=self.st)
        F.image_from_fips203_dev(t_hat.data_ptr(), B * k, t_fips.data_ptr(), io_bits=16, device=self.dev, stream=self.st)
        r, m = r.contiguous(), m.contiguous()
        y, e1, e2, mu, u, v = self.words(B, k, N), self.words(B, k, N), self.words(B, 1, N), self.words(B, 1, N), self.words(B, k, N), self.words(B, 1, N)
        F.sample_cbd_dev(y.data_ptr(), B, r.data_ptr(), self.eta1, first_nonce=0, per_seed=k, io_bits=16, device=self.dev, stream=self.st)
        F.sample_cbd_dev(e1.data_ptr(), B, r.data_ptr(), self.eta2, first_nonce=k, per_seed=k, io_bits=16, device=self.dev, stream=self.st)
        F.sample_cbd_dev(e2.data_ptr(), B, r.data_ptr(), self.eta2, first_nonce=2 * k, per_seed=1, io_bits=16, device=self.dev, stream=self.st)
        C.decode_decompress_dev(m.data_ptr(), mu.data_ptr(), Q, 1, B * N, io_bits=16, device=self.dev, stream=self.st)
        self.fma(a_hat, y, e1, u, B, k, k, k * k * N, trans=1)
        e2mu = (e2 + mu).contiguous()
        self.fma(t_hat, y, e2mu, v, B, 1, k, k * N, trans=1)
        c1, c2 = self.u8(B, 32 * self.du * k), self.u8(B, 32 * self.dv)
        C.compress_encode_dev(u.data_ptr(), c1.data_ptr(), Q, self.du, B * k * N, io_bits=16, device=self.dev, stream=self.st)
        C.compress_encode_dev(v.data_ptr(), c2.data_ptr(), Q, self.dv, B * N, io_bits=16, device=self.dev, stream=self.st)
        return t.cat([c1, c2], dim=1).contiguous()

    def encaps(self, ek, m):
        t, F, B = self.t, self.F, ek.shape[0]
        g = self.hash(F.SHA3_512, t.cat([m, self.hash(F.SHA3_256, ek, 32)], dim=1), 64)
        return g[:, :32].contiguous(), self.encrypt(ek, m, g[:, 32:], B)

    def decaps(self, dk, ct):
        t, k, F, C, B = self.t, self.k, self.F, self.C, dk.shape[0]
        s_fips, s_hat, u, v, w = self.words(B, k, N), self.images(B, k, N), self.words(B, k, N), self.words(B, 1, N), self.words(B, 1, N)
        dk_pke = dk[:, :384 * k].contiguous()
        c1, c2 = ct[:, :32 * self.du * k].contiguous(), ct[:, 32 * self.du * k:].contiguous()
        C.byte_decode_dev(dk_pke.data_ptr(), s_fips.data_ptr(), Q, 12, B * k * N, io_bits=16, device=self.dev, stream=self.st)
        F.image_from_fips203_dev(s_hat.data_ptr(), B * k, s_fips.data_ptr(), io_bits=16, device=self.dev, stream=self.st)
        C.decode_decompress_dev(c1.data_ptr(), u.data_ptr(), Q, self.du, B * k * N, io_bits=16, device=self.dev, stream=self.st)
        C.decode_decompress_dev(c2.data_ptr(), v.data_ptr(), Q, self.dv, B * N, io_bits=16, device=self.dev, stream=self.st)
        self.fma(s_hat, u, v, w, B, 1, k, k * N, trans=1, sign=-1)
        m2 = self.u8(B, 32)
        C.compress_encode_dev(w.data_ptr(), m2.data_ptr(), Q, 1, B * N, io_bits=16, device=self.dev, stream=self.st)
        g = self.hash(F.SHA3_512, t.cat([m2, dk[:, 768 * k + 32:768 * k + 64]], dim=1), 64)
        k_bar = self.hash(F.SHAKE256, t.cat([dk[:, 768 * k + 64:], ct], dim=1), 32)
        c_again = self.encrypt(dk[:, 384 * k:768 * k + 32], m2, g[:, 32:], B)
        same = (c_again == ct).all(dim=1, keepdim=True)
        return t.where(same, g[:, :32], k_bar).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="mlkem_timing.json")
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
    K = T.mlkem
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for name in PARAMS:
        sz = K.sizes(name)
        for count in (int(c) for c in a.counts.split(",")):
            gen = torch.Generator(device="cuda").manual_seed(20261019 + count)
            d, z, m = (torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3))
            ek, dk = torch.empty((count, sz["ek"]), dtype=torch.uint8, device="cuda"), torch.empty((count, sz["dk"]), dtype=torch.uint8, device="cuda")
            ss, ct = torch.empty((count, 32), dtype=torch.uint8, device="cuda"), torch.empty((count, sz["ct"]), dtype=torch.uint8, device="cuda")
            ss2 = torch.empty_like(ss)
            wsb = {op: K.workspace_bytes(name, count, op) for op in ("keygen", "encaps", "decaps")}
            ws = torch.empty(max(wsb.values()) + 256, dtype=torch.uint8, device="cuda")
            pws = (ws.data_ptr() + 255) // 256 * 256
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            comp = Composed(torch, T, name, a.device, stream)
            entry = {
                "keygen": lambda: K.keygen_dev(name, count, d.data_ptr(), z.data_ptr(), ek.data_ptr(), dk.data_ptr(), pws, wsb["keygen"], flag.data_ptr(), a.device, stream),
                "encaps": lambda: K.encaps_dev(name, count, ek.data_ptr(), m.data_ptr(), ss.data_ptr(), ct.data_ptr(), pws, wsb["encaps"], flag.data_ptr(), a.device, stream),
                "decaps": lambda: K.decaps_dev(name, count, dk.data_ptr(), ct.data_ptr(), ss2.data_ptr(), pws, wsb["decaps"], flag.data_ptr(), a.device, stream),
            }
            composed = {"keygen": lambda: comp.keygen(d, z), "encaps": lambda: comp.encaps(ek, m), "decaps": lambda: comp.decaps(dk, ct)}
            # the two routes agree before anything is timed
            entry["keygen"]()
            entry["encaps"]()
            entry["decaps"]()
            cek, cdk = composed["keygen"]()
            css, cct = composed["encaps"]()
            cs2 = composed["decaps"]()
            torch.cuda.synchronize()
            assert torch.equal(cek, ek) and torch.equal(cdk, dk) and torch.equal(css, ss) and torch.equal(cct, ct), (name, count)
            assert torch.equal(cs2, ss2) and torch.equal(ss, ss2) and int(flag.item()) == 0, (name, count)
            del cek, cdk, css, cct, cs2
            for op in ("keygen", "encaps", "decaps"):
                ms = timed(torch, [("entry", entry[op]), ("composed", composed[op])], a.warmup, a.reps)
                med = {k: statistics.median(v) for k, v in ms.items()}
                row = {"set": name, "op": op, "count": count, "reps": a.reps, "workspace_bytes": wsb[op],
                       "entry_median_ms": round(med["entry"], 4), "entry_min_ms": round(min(ms["entry"]), 4), "entry_max_ms": round(max(ms["entry"]), 4),
                       "composed_median_ms": round(med["composed"], 4), "composed_min_ms": round(min(ms["composed"]), 4),
                       "composed_max_ms": round(max(ms["composed"]), 4), "entry_ops_per_s": round(count / (med["entry"] * 1e-3)),
                       "composed_ops_per_s": round(count / (med["composed"] * 1e-3)), "composed_over_entry": round(med["composed"] / med["entry"], 3)}
                rows.append(row)
                print(f"{name:12s} {op:7s} {count:6d}  entry {med['entry']:9.3f} ms ({row['entry_ops_per_s'] / 1e6:7.3f} M/s)  composed {med['composed']:9.3f} ms"
                      f"  composed / entry {row['composed_over_entry']:6.3f}", flush=True)
            del d, z, m, ek, dk, ss, ct, ss2, ws
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(a.device), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
