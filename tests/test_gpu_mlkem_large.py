"""ML-KEM-1024 on the MI355X at the smallest batches in which one array that a single kernel addresses passes 2^32 bytes: the images `hat` of Decaps
(24 576 bytes per instance) and of Encaps (20 480), and the images `a_hat` of KeyGen (16 384).  An index computed in 32 bits anywhere below the
entry points would wrap there, and at 65 536 instances, the largest batch any other test or tool runs, no array reaches that size.

Instance i is instance i mod 7 of the model's run of seven (tests/helpers/mlkem_cases.py `tiled`).  Seven is coprime to the 64 instances of a
workgroup and the 256 lanes of a block, and in none of the three arrays is 2^32 bytes a whole number of periods (in `a_hat` it is 262 144
instances, 1 mod 7), so an instance read or written at a wrapped index does not meet bytes equal to its own.  Inputs and expected outputs are built on the device from the period;
every byte of every instance is compared there, and the guard bytes, the cleared workspace and the sampler flag are checked there too: nothing of
the batch's size is copied to the host.  Each test frees what it allocated."""
import pytest

from tests.helpers import mlkem_cases as C
from tests.helpers import mlkem_model as R
from tests.helpers.mlkem_gpu import Scratch, _out, _put_dev, _take_dev

pytestmark = pytest.mark.gpu

NAME, PERIOD, K_RANK = "ML-KEM-1024", 7, 4
POLY = 512                                                               # bytes of a polynomial of 16-bit words; its image takes twice that


@pytest.fixture(scope="module")
def K():
    import tools_amd
    return tools_amd.mlkem


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def sections(op, count):
    """the workspace sections of psf_mlkem.hip (keygen_ws, encaps_ws, decaps_ws) for ML-KEM-1024 in order, as (name, bytes)"""
    k, c, ct = K_RANK, count, R.sizes(NAME)["ct"]
    if op == "keygen":
        return [("sigma", 32 * c), ("a_fips", c * k * k * POLY), ("a_hat", c * k * k * POLY * 2), ("e", c * k * POLY), ("ts", c * 2 * k * POLY),
                ("st_hat", c * 2 * k * POLY * 2), ("st_fips", c * 2 * k * POLY)]
    if op == "encaps":
        return [("h", 32 * c), ("r", 32 * c), ("fips", c * (k * k + k) * POLY), ("hat", c * (k * k + k) * POLY * 2), ("y", c * k * POLY), ("e1", c * k * POLY),
                ("e2", c * POLY), ("u", c * k * POLY), ("v", c * POLY)]
    return [("fips", c * (k * k + 2 * k) * POLY), ("hat", c * (k * k + 2 * k) * POLY * 2), ("u2", c * k * POLY), ("v2", c * POLY), ("w", c * POLY), ("mp", 32 * c),
            ("kp", 32 * c), ("rp", 32 * c), ("y", c * k * POLY), ("e1", c * k * POLY), ("e2", c * POLY), ("u", c * k * POLY), ("v", c * POLY), ("cp", c * ct)]


def crossing(K, op, count, section, per_instance):
    """`count` is the smallest batch at which `section` reaches 2^32 bytes, plus 3 (a ragged last workgroup); returns the workspace size"""
    secs = dict(sections(op, count))
    assert secs[section] == per_instance * count == max(secs.values())
    assert per_instance * (count - 3) >= 2 ** 32 > per_instance * (count - 4)
    assert count % 64 != 0 and count % 256 != 0 and count % PERIOD != 0
    assert (2 ** 32) % (per_instance * PERIOD) != 0
    need = K.workspace_bytes(NAME, count, op)
    assert need == sum((b + 255) // 256 * 256 for _, b in sections(op, count))       # the section formulas are the library's
    return need


def room(torch, need):
    free, _ = torch.cuda.mem_get_info()
    if free < need + 2 * 2 ** 30:
        pytest.skip(f"{free} bytes of device memory are free; the test needs its workspace of {need} bytes plus {2 * 2 ** 30}")


def rows(torch, items):
    """the period's items as a (period, size) uint8 tensor on the device"""
    import numpy as np
    return torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), len(items[0])).copy()).cuda()


def tile(torch, period_rows, count):
    return period_rows.repeat((count + PERIOD - 1) // PERIOD, 1)[:count].contiguous()


def same_rows(torch, got, period_rows, what):
    """got[i] == period_rows[i mod 7] for every i, compared on the device a slab of periods at a time; names the first instances that differ"""
    count, step = got.shape[0], PERIOD * 4096
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


def test_decaps_with_the_images_past_4_gib(K, torch):
    count = 174766
    need = crossing(K, "decaps", count, "hat", 24576)
    room(torch, need)
    ref, _ = C.tiled(NAME, PERIOD, count)
    try:
        bdk, pdk = _put_dev(torch, tile(torch, rows(torch, ref.fields["dk"]), count), 0)
        bct, pct = _put_dev(torch, tile(torch, rows(torch, ref.fields["c"]), count), 0)
        bss, pss = _out(torch, count * 32, 0)
        sc = Scratch(torch, K, NAME, count, "decaps", flag=4)
        torch.cuda.synchronize()
        K.decaps_dev(NAME, count, pdk, pct, pss, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
        ss = _take_dev(torch, bss, count * 32, 32, "decaps", 0)
        same_rows(torch, ss, rows(torch, ref.fields["K"]), "K")
        sc.check_dev("decaps")
    finally:
        bdk = bct = bss = sc = ss = None
        release(torch)


def test_encaps_with_the_images_past_4_gib(K, torch):
    count = 209719
    need = crossing(K, "encaps", count, "hat", 20480)
    room(torch, need)
    ref, _ = C.tiled(NAME, PERIOD, count)
    sz = R.sizes(NAME)
    try:
        bek, pek = _put_dev(torch, tile(torch, rows(torch, ref.fields["ek"]), count), 0)
        bm, pm = _put_dev(torch, tile(torch, rows(torch, ref.fields["m"]), count), 0)
        bss, pss = _out(torch, count * 32, 0)
        bct, pct = _out(torch, count * sz["ct"], 0)
        sc = Scratch(torch, K, NAME, count, "encaps", flag=0)
        torch.cuda.synchronize()
        K.encaps_dev(NAME, count, pek, pm, pss, pct, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
        ss = _take_dev(torch, bss, count * 32, 32, "ss", 0)
        ct = _take_dev(torch, bct, count * sz["ct"], sz["ct"], "ct", 0)
        same_rows(torch, ct, rows(torch, ref.fields["c"]), "c")
        same_rows(torch, ss, rows(torch, ref.fields["K"]), "K")
        sc.check_dev("encaps")
    finally:
        bek = bm = bss = bct = sc = ss = ct = None
        release(torch)


def test_keygen_with_the_images_of_the_matrix_at_4_gib(K, torch):
    count = 262147
    need = crossing(K, "keygen", count, "a_hat", 16384)
    room(torch, need)
    ref, _ = C.tiled(NAME, PERIOD, count)
    sz = R.sizes(NAME)
    try:
        bd, pd = _put_dev(torch, tile(torch, rows(torch, ref.fields["d"]), count), 0)
        bz, pz = _put_dev(torch, tile(torch, rows(torch, ref.fields["z"]), count), 0)
        bek, pek = _out(torch, count * sz["ek"], 0)
        bdk, pdk = _out(torch, count * sz["dk"], 0)
        sc = Scratch(torch, K, NAME, count, "keygen", flag=0)
        torch.cuda.synchronize()
        K.keygen_dev(NAME, count, pd, pz, pek, pdk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr())
        ek = _take_dev(torch, bek, count * sz["ek"], sz["ek"], "ek", 0)
        dk = _take_dev(torch, bdk, count * sz["dk"], sz["dk"], "dk", 0)
        same_rows(torch, ek, rows(torch, ref.fields["ek"]), "ek")
        same_rows(torch, dk, rows(torch, ref.fields["dk"]), "dk")
        sc.check_dev("keygen")
    finally:
        bd = bz = bek = bdk = sc = ek = dk = None
        release(torch)
