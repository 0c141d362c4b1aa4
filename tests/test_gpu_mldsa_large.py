"""ML-DSA-87 on the MI355X at the smallest batch in which one array that a single kernel addresses passes 2^32 bytes: the images `a_hat` of ExpandA
(57 344 bytes per instance) in KeyGen, in Verify and in the slots of signing with one key per instance, at 74 902 instances; and w and c t0 of signing
with one key for all (16 384 bytes per instance), at 262 147.  An index computed in 32 bits anywhere below the entry points would wrap there; the
largest batch that checks bytes elsewhere in the suite is 321 instances (signing) and 259 (verification).

Instance i is instance i mod 7 of the model (KeyGen, Verify) or i mod 29 (signing: 29 (key, M', rnd) over 7 keys, whose attempt counts differ, so that
slots leave the live prefix in an irregular pattern and k_sign_match / k_sign_move compact tens of thousands of slots per round).  Neither period
divides the batch, 64 or 256, and 2^32 bytes is not a whole number of periods of `a_hat`, so an instance read or written at a wrapped index does not
meet bytes equal to its own.  Inputs and expected outputs are built on the device from the period; every byte of every instance is compared there,
and the guard bytes, the workspace and the flag are checked there too: nothing of the batch's size is copied to the host.  Each test frees what it
allocated."""
import functools
import random

import numpy as np
import pytest

from tests.helpers import mldsa_model as M
from tests.helpers.mldsa_gpu import Scratch, flip, keys, layout, with_hint
from tests.helpers.mldsa_sign_gpu import reference
from tests.helpers.mlkem_gpu import _out, _put_dev, _take_dev

pytestmark = pytest.mark.gpu

NAME, K_RANK, L_RANK = "ML-DSA-87", 8, 7
COUNT = 74902                                                            # 2^32 / 57 344 rounded up, plus 3 (a ragged last workgroup)
PERIOD, SIGN_PERIOD, MSG_LEN = 7, 29, 72
IMAGE, POLY = 1024, 2048                                                 # bytes of a product image and of a polynomial of 64-bit words


@pytest.fixture(scope="module")
def D():
    import tools_amd
    return tools_amd.mldsa


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def sections(op, count):
    """the workspace sections of psf_mldsa.hip (keygen_ws, verify_ws) and psf_mldsa_sign.hip (sign_ws with one key per instance: "sign", with one key
    for all: "sign_one") in order, as (name, bytes)"""
    k, l, c = K_RANK, L_RANK, count
    if op == "sign_one":
        return [(n, b // c if n in ("a_hat", "s1", "s2", "t0") else b) for n, b in sections("sign", count)]
    if op == "keygen":
        return [("rho_p", 64 * c), ("a_hat", c * k * l * IMAGE), ("s1", c * l * POLY), ("s2", c * k * POLY), ("t", c * k * POLY)]
    if op == "verify":
        return [("tr", 64 * c), ("mu", 64 * c), ("flags", 4 * c), ("h", 32 * k * c), ("a_hat", c * k * l * IMAGE), ("z", c * l * POLY), ("t1", c * k * POLY),
                ("c", c * POLY), ("w", c * k * POLY)]
    return [("a_hat", c * k * l * IMAGE), ("s1", c * l * IMAGE), ("s2", c * k * IMAGE), ("t0", c * k * IMAGE), ("mu", 64 * c), ("rho", 64 * c), ("kappa", 4 * c),
            ("index", 4 * c), ("ctl", 16), ("y", c * l * POLY), ("w", c * k * POLY), ("c", c * POLY), ("z", c * l * POLY), ("ct0", c * k * POLY), ("ct", 64 * c),
            ("flags", 4 * c), ("holes", 4 * c), ("srcs", 4 * c)]


def crossing(D, op, period, count=COUNT, section="a_hat", per_instance=K_RANK * L_RANK * IMAGE):
    """`count` is the smallest batch at which `section`, the largest of the operation, reaches 2^32 bytes, plus 3; returns the workspace size"""
    secs = dict(sections(op, count))
    assert secs[section] == per_instance * count == max(secs.values())
    assert per_instance * (count - 3) >= 2 ** 32 > per_instance * (count - 4)
    assert count % 64 != 0 and count % 256 != 0 and count % period != 0
    assert (2 ** 32) % (per_instance * period) != 0
    if op in ("sign", "sign_one"):
        need = D.sign_workspace_bytes(NAME, count, 0 if op == "sign_one" else None)
    else:
        need = D.workspace_bytes(NAME, count, op)
    assert need == sum((b + 255) // 256 * 256 for _, b in sections(op, count))       # the section formulas are the library's
    return need


def room(torch, need, rest):
    free, _ = torch.cuda.mem_get_info()
    if free < need + rest + 2 ** 30:
        pytest.skip(f"{free} bytes of device memory are free; the test needs its workspace of {need} bytes, {rest} bytes of inputs and outputs, and {2 ** 30}")


def rows(torch, items):
    """the period's items as a (period, size) uint8 tensor on the device"""
    return torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), len(items[0])).copy()).cuda()


def tile(torch, period_rows, count):
    p = period_rows.shape[0]
    return period_rows.repeat((count + p - 1) // p, 1)[:count].contiguous()


def same_rows(torch, got, period_rows, what):
    """got[i] == period_rows[i mod period] for every i, compared on the device a slab of periods at a time; names the first instances that differ"""
    count, step = got.shape[0], period_rows.shape[0] * 2048
    want = tile(torch, period_rows, min(step, count))
    bad = []
    for lo in range(0, count, step):
        part = got[lo:lo + step]
        ne = (part != want[:part.shape[0]]).any(dim=1)
        if bool(ne.any().item()):
            bad += [lo + int(i) for i in ne.nonzero().flatten()[:8].tolist()]
            if len(bad) >= 8:
                break
    assert not bad, (what, "first differing instances:", bad[:8], "of", count)


def release(torch):
    import gc
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def sign_period(one_key=False):
    """29 instances (pk, sk, M', rnd, sigma, attempts): instance j under key j mod 7, or all under key 0"""
    ks = keys(NAME, PERIOD)
    rng = random.Random(8713)
    out = []
    for j in range(SIGN_PERIOD):
        msg, rnd, key = rng.randbytes(MSG_LEN), rng.randbytes(32), 0 if one_key else j % PERIOD
        out.append((ks["pk"][key], ks["sk"][key], msg, rnd) + reference(NAME, ks["sk"][key], msg, rnd, False))
    assert len({o[5] for o in out}) >= 4                                  # attempt counts differ: slots leave in an irregular pattern
    return out


def test_keygen_with_the_images_of_the_matrix_at_4_gib(D, torch):
    need = crossing(D, "keygen", PERIOD)
    sz = M.sizes(NAME)
    room(torch, need, COUNT * (sz["pk"] + sz["sk"] + 32))
    ref = keys(NAME, PERIOD)
    try:
        bxi, pxi = _put_dev(torch, tile(torch, rows(torch, ref["xi"]), COUNT), 0)
        bpk, ppk = _out(torch, COUNT * sz["pk"], 0)
        bsk, psk = _out(torch, COUNT * sz["sk"], 0)
        sc = Scratch(torch, D, NAME, COUNT, "keygen", flag=0)
        torch.cuda.synchronize()
        D.keygen_dev(NAME, COUNT, pxi, ppk, psk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
        pk = _take_dev(torch, bpk, COUNT * sz["pk"], sz["pk"], "pk", 0)
        sk = _take_dev(torch, bsk, COUNT * sz["sk"], sz["sk"], "sk", 0)
        same_rows(torch, pk, rows(torch, ref["pk"]), "pk")
        same_rows(torch, sk, rows(torch, ref["sk"]), "sk")
        sc.check("keygen", cleared=True)
    finally:
        bxi = bpk = bsk = sc = pk = sk = None
        release(torch)


def test_verify_with_a_key_per_instance_and_the_images_at_4_gib(D, torch):
    need = crossing(D, "verify", PERIOD)
    sz, lay = M.sizes(NAME), layout(NAME)
    room(torch, need, COUNT * (sz["pk"] + sz["sig"] + MSG_LEN + 2))
    per = sign_period()[:PERIOD]
    pks, msgs, sigs = [p[0] for p in per], [p[2] for p in per], [p[4] for p in per]
    sigs[2] = flip(sigs[2], lay["z"] + 1234, 5)
    sigs[5] = with_hint(NAME, sigs[5], bytes([9, 9]) + bytes(sz["sig"] - lay["hint"] - 2))
    why = [M.verify_why(p, m, s, NAME) for p, m, s in zip(pks, msgs, sigs)]
    assert why == [0, 0, M.HASH, 0, 0, M.HINT | M.HASH, 0]
    try:
        bp, pp = _put_dev(torch, tile(torch, rows(torch, pks), COUNT), 0)
        bm, pm = _put_dev(torch, tile(torch, rows(torch, msgs), COUNT), 0)
        bs, ps = _put_dev(torch, tile(torch, rows(torch, sigs), COUNT), 0)
        bok, pok = _out(torch, COUNT, 0)
        bwhy, pwhy = _out(torch, COUNT, 0)
        sc = Scratch(torch, D, NAME, COUNT, "verify", flag=0)
        torch.cuda.synchronize()
        D.verify_dev(NAME, COUNT, pp, pm, MSG_LEN, ps, pok, sc.ptr, sc.bytes, d_why=pwhy, d_fail=sc.flag.data_ptr())
        ok = _take_dev(torch, bok, COUNT, 1, "ok", 0)
        got = _take_dev(torch, bwhy, COUNT, 1, "why", 0)
        same_rows(torch, got, rows(torch, [bytes([w]) for w in why]), "why")
        same_rows(torch, ok, rows(torch, [bytes([w == 0]) for w in why]), "ok")
        sc.check("verify", cleared=False)
    finally:
        bp = bm = bs = bok = bwhy = sc = ok = got = None
        release(torch)


def sign_all(D, torch, count, need, one_key):
    """begin / round / end over `count` instances tiled from sign_period(one_key), `active` read back after every round, with every check on the device"""
    sz = M.sizes(NAME)
    room(torch, need, count * (sz["sig"] + MSG_LEN + 32 + 4 + (0 if one_key else sz["sk"])))
    per = sign_period(one_key)
    stride = 0 if one_key else sz["sk"]
    try:
        bsk, psk = _put_dev(torch, rows(torch, [per[0][1]]) if one_key else tile(torch, rows(torch, [p[1] for p in per]), count), 0)
        bm, pm = _put_dev(torch, tile(torch, rows(torch, [p[2] for p in per]), count), 0)
        br, pr = _put_dev(torch, tile(torch, rows(torch, [p[3] for p in per]), count), 0)
        bsig, psig = _out(torch, count * sz["sig"], 0)
        rounds = torch.zeros(count, dtype=torch.int32, device="cuda")
        live = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        pws = (ws.data_ptr() + 255) // 256 * 256
        lo = pws - ws.data_ptr()
        torch.cuda.synchronize()
        D.sign_begin_dev(NAME, count, psk, pm, MSG_LEN, pws, need, live.data_ptr(), d_rnd=pr, sk_stride=stride, d_fail=fail.data_ptr())
        torch.cuda.synchronize()
        now = int(live.item())
        assert now == count
        trail = []
        while now and len(trail) < 400:
            D.sign_round_dev(NAME, count, now, psig, pws, need, live.data_ptr(), d_rounds=rounds.data_ptr(), sk_stride=stride, d_fail=fail.data_ptr())
            torch.cuda.synchronize()
            now = int(live.item())
            trail.append(now)
            assert now == int((rounds == 0).sum().item()), ("d_live against the zero entries of d_rounds", len(trail), now)
        D.sign_end_dev(NAME, count, pws, need, sk_stride=stride)
        torch.cuda.synchronize()
        attempts = [p[5] for p in per]
        assert now == 0 and len(trail) == max(attempts)
        want_rounds = torch.tensor(attempts, dtype=torch.int32, device="cuda").repeat((count + SIGN_PERIOD - 1) // SIGN_PERIOD)[:count]
        ne = (rounds != want_rounds).nonzero().flatten()
        assert ne.numel() == 0, ("attempt counts, first differing instances:", ne[:8].tolist())
        sig = _take_dev(torch, bsig, count * sz["sig"], sz["sig"], "sig", 0)
        same_rows(torch, sig, rows(torch, [p[4] for p in per]), "sig")
        assert not bool(ws[lo:lo + need].any().item()), "the workspace is not all zero after end"
        assert bool((ws[:lo] == 0x5A).all().item()) and bool((ws[lo + need:] == 0x5A).all().item()), "wrote outside the workspace"
        assert int(fail.item()) == 0
    finally:
        bsk = bm = br = bsig = rounds = ws = sig = want_rounds = ne = None
        release(torch)


def test_sign_with_a_key_per_instance_and_the_images_at_4_gib(D, torch):
    sign_all(D, torch, COUNT, crossing(D, "sign", SIGN_PERIOD), one_key=False)


def test_sign_with_one_key_for_all_and_w_and_c_t0_at_4_gib(D, torch):
    """with one key the images are one instance's, and the largest arrays are w and c t0 (16 384 bytes per instance): they reach 2^32 bytes at 262 144"""
    count = 262147
    sign_all(D, torch, count, crossing(D, "sign_one", SIGN_PERIOD, count, "w", K_RANK * POLY), one_key=True)
