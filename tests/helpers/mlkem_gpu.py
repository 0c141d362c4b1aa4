"""The harness of the ML-KEM device tests (tests/test_gpu_mlkem*.py): buffers at chosen byte offsets from a 16-byte boundary with guard bytes around
every output, the workspace and sampler flag of a call with their checks, one function per device entry point that runs it and applies all of
them, and the cached run of the pure-Python model that the tests compare with.  Nothing here imports the library or torch: both are arguments.

Offsets.  Every `dev_*` function and `_run_check` takes `offs`: None (every buffer one byte past a 16-byte boundary, the default of the suite), an
int (that offset for every buffer) or a dict from `offsets()` with one entry per buffer: the inputs "in_d", "in_z", "in_ek", "in_m", "in_dk",
"in_ct" and the outputs "out_ek", "out_dk", "out_ss", "out_ct", "out_ok"."""
import functools
import random

import numpy as np

from tests.helpers import fips203_kpke_model as M
from tests.helpers import mlkem_model as R

GUARD, FILL = 64, 0xA5
NAMES = sorted(M.PARAMS)
INPUTS = ("d", "z", "ek", "m", "dk", "ct")
OUTPUTS = ("ek", "dk", "ss", "ct", "ok")


@functools.lru_cache(maxsize=None)
def model(name, count):
    """the model's run of `count` instances from a fixed seed: inputs, keys, ciphertexts and shared secrets (never modified by a test)"""
    rng = random.Random(1009 * NAMES.index(name) + count)
    d, z, m = ([rng.randbytes(32) for _ in range(count)] for _ in range(3))
    keys = [R.keygen_internal(a, b, name) for a, b in zip(d, z)]
    enc = [R.encaps_internal(ek, mm, name) for (ek, _), mm in zip(keys, m)]
    for (_, dk), (key, c) in zip(keys[:2], enc[:2]):
        assert R.decaps_internal(dk, c, name) == key
    return {"d": d, "z": z, "m": m, "ek": [k[0] for k in keys], "dk": [k[1] for k in keys], "K": [e[0] for e in enc], "c": [e[1] for e in enc]}


def offsets(inputs=1, outputs=1, **named):
    """the `offs` dict with every input at `inputs`, every output at `outputs`, and the buffers in `named` (in_ek=0, out_ct=4, ...) at their own"""
    offs = {"in_" + k: inputs for k in INPUTS}
    offs.update({"out_" + k: outputs for k in OUTPUTS})
    for key, value in named.items():
        assert key in offs, key
        offs[key] = value
    return offs


def _off(offs, key):
    if offs is None:
        return 1
    if isinstance(offs, int):
        return offs
    return offs[key]


def _out(torch, nbytes, off=1):
    buf = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + GUARD + off


def _take(torch, buf, nbytes, size, what, off=1):
    """the items of `size` bytes a call wrote, after checking that the guard bytes on both sides are untouched"""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo = GUARD + off
    assert (host[:lo] == FILL).all(), (what, "wrote before the output")
    assert (host[lo + nbytes:] == FILL).all(), (what, "wrote beyond the output")
    return [bytes(host[lo + i:lo + i + size]) for i in range(0, nbytes, size)]


def _take_dev(torch, buf, nbytes, size, what, off=1):
    """_take without the host copy: the guard checks as device reductions, and the written bytes as a (count, size) view of the buffer"""
    torch.cuda.synchronize()
    lo = GUARD + off
    assert bool((buf[:lo] == FILL).all().item()), (what, "wrote before the output")
    assert bool((buf[lo + nbytes:] == FILL).all().item()), (what, "wrote beyond the output")
    return buf[lo:lo + nbytes].view(nbytes // size, size)


def _put(torch, items, off=1):
    """the concatenation of `items` on the device, the first byte `off` bytes past a 16-byte boundary; returns (tensor, pointer)"""
    data = np.frombuffer(b"".join(items), dtype=np.uint8)
    buf = torch.zeros((16 + data.size + off,), dtype=torch.uint8, device="cuda")
    buf[off:off + data.size] = torch.from_numpy(data.copy())
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + off


def _put_dev(torch, rows, off=1):
    """_put for a (count, size) uint8 tensor that is already on the device"""
    n = rows.numel()
    buf = torch.zeros((16 + n + off,), dtype=torch.uint8, device="cuda")
    buf[off:off + n] = rows.reshape(-1)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + off


class Scratch:
    """the workspace of one call, filled with a non-zero byte, and a sampler flag that starts at `flag`"""

    def __init__(self, torch, K, name, count, op, flag=0):
        self.torch, self.bytes = torch, K.workspace_bytes(name, count, op)
        assert self.bytes % 256 == 0 and self.bytes > 0
        self.ws = torch.full((self.bytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        self.ptr = (self.ws.data_ptr() + 255) // 256 * 256
        self.start = flag
        self.flag = torch.full((1,), flag, dtype=torch.int32, device="cuda")

    def check(self, what):
        self.torch.cuda.synchronize()
        lo = self.ptr - self.ws.data_ptr()
        host = self.ws.cpu().numpy()
        assert not host[lo:lo + self.bytes].any(), (what, "the workspace is not all zero after the call")
        assert (host[:lo] == 0x5A).all() and (host[lo + self.bytes:] == 0x5A).all(), (what, "wrote outside the workspace")
        assert int(self.flag.item()) == self.start, (what, "the sampler flag changed")

    def check_dev(self, what):
        """check() with reductions on the device: no copy of the workspace to the host, no temporary of its size"""
        self.torch.cuda.synchronize()
        lo = self.ptr - self.ws.data_ptr()
        assert not bool(self.ws[lo:lo + self.bytes].any().item()), (what, "the workspace is not all zero after the call")
        assert bool((self.ws[:lo] == 0x5A).all().item()) and bool((self.ws[lo + self.bytes:] == 0x5A).all().item()), (what, "wrote outside the workspace")
        assert int(self.flag.item()) == self.start, (what, "the sampler flag changed")


def dev_keygen(torch, K, name, d, z, flag=0, offs=None):
    count, sz = len(d), R.sizes(name)
    o_ek, o_dk = _off(offs, "out_ek"), _off(offs, "out_dk")
    (bd, pd), (bz, pz) = _put(torch, d, _off(offs, "in_d")), _put(torch, z, _off(offs, "in_z"))      # the tensors live until the call has run
    bek, pek = _out(torch, count * sz["ek"], o_ek)
    bdk, pdk = _out(torch, count * sz["dk"], o_dk)
    sc = Scratch(torch, K, name, count, "keygen", flag)
    torch.cuda.synchronize()
    K.keygen_dev(name, count, pd, pz, pek, pdk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
    ek = _take(torch, bek, count * sz["ek"], sz["ek"], (name, count, "ek"), o_ek)
    dk = _take(torch, bdk, count * sz["dk"], sz["dk"], (name, count, "dk"), o_dk)
    sc.check((name, count, "keygen"))
    del bd, bz
    return ek, dk, (bek, pek)


def dev_encaps(torch, K, name, ek, m, flag=0, ek_ptr=None, offs=None):
    count, sz = len(m), R.sizes(name)
    o_ss, o_ct = _off(offs, "out_ss"), _off(offs, "out_ct")
    keep = None
    if ek_ptr is None:
        keep, ek_ptr = _put(torch, ek, _off(offs, "in_ek"))
    bm, pm = _put(torch, m, _off(offs, "in_m"))
    bss, pss = _out(torch, count * 32, o_ss)
    bct, pct = _out(torch, count * sz["ct"], o_ct)
    sc = Scratch(torch, K, name, count, "encaps", flag)
    torch.cuda.synchronize()
    K.encaps_dev(name, count, ek_ptr, pm, pss, pct, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
    ss = _take(torch, bss, count * 32, 32, (name, count, "ss"), o_ss)
    ct = _take(torch, bct, count * sz["ct"], sz["ct"], (name, count, "ct"), o_ct)
    sc.check((name, count, "encaps"))
    del keep, bm
    return ss, ct


def dev_decaps(torch, K, name, dk, ct, flag=0, offs=None):
    count = len(dk)
    o_ss = _off(offs, "out_ss")
    bdk, pdk = _put(torch, dk, _off(offs, "in_dk"))
    bct, pct = _put(torch, ct, _off(offs, "in_ct"))
    bss, pss = _out(torch, count * 32, o_ss)
    sc = Scratch(torch, K, name, count, "decaps", flag)
    torch.cuda.synchronize()
    K.decaps_dev(name, count, pdk, pct, pss, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
    ss = _take(torch, bss, count * 32, 32, (name, count, "decaps"), o_ss)
    sc.check((name, count, "decaps"))
    del bdk, bct
    return ss


def flip(c, pos, bit=0):
    b = bytearray(c)
    b[pos] ^= 1 << bit
    return bytes(b)


def _run_check(torch, fn, name, items, offs=None):
    """check_ek_dev / check_dk_dev (`fn`) over `items`: the input at offset "in_ek" / "in_dk" by the function's name, the result bytes at "out_ok" """
    count = len(items)
    o_ok = _off(offs, "out_ok")
    bin_, pin = _put(torch, items, _off(offs, "in_dk" if fn.__name__ == "check_dk_dev" else "in_ek"))
    bok, pok = _out(torch, count, o_ok)
    torch.cuda.synchronize()
    fn(name, count, pin, pok)
    ok = _take(torch, bok, count, 1, (name, fn.__name__), o_ok)          # the guard: bytes of d_ok beyond count are untouched
    del bin_
    return [b[0] for b in ok]
