"""SHAKE256, SHA-256 and SHA-512 at a pitch of 4096 bytes, the FIPS 203 samplers and the NTT-image interop (psf_keccak.hip, psf_sha2.hip) on the
MI355X at the smallest batches in which the messages, the digests, the sampled polynomials or the images pass 2^32 bytes.  The largest batch of
any other test is 257 messages, so c * in_stride, c * out_stride, (p0 + p) * 256 + j and c * 256 + src have never reached 2^32; a truncated
offset stays inside the buffer and faults nothing.

About a million short hashes 4096 bytes apart give the crossing: nothing hashes 4 GiB.  Instance i is instance i mod 7 of a period whose
expectation comes from hashlib and tests/helpers/fips203_kpke_model.py (period 13 where the count, 2^20 + 3, is a multiple of 7); 2^32 bytes
are no whole number of periods.  Every output is prefilled with the guard byte between guard bytes, one byte (one word for the polynomials)
past a 16-byte boundary; every byte of every output is compared on the device, and the gap bytes between pitched digests keep the guard value.
The sampler flag stays 0.  Each test frees what it allocated."""
import hashlib
import time

import numpy as np
import pytest

from tests.helpers import fips203_kpke_model as K
from tests.helpers import large_cases as L
from tests.helpers.slhdsa_gpu import release, rows, same_rows, tile

pytestmark = pytest.mark.gpu

PITCH = 4096


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def report(request, torch):
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    print(f"\n{request.node.name}: {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB of device memory")


def hashers(T):
    return {
        "keccak": (lambda *a, **k: T.fips203.keccak_dev(T.fips203.SHAKE256, *a, **k), lambda m: hashlib.shake_256(m).digest(32)),
        "sha256": (lambda *a, **k: T.sha2.sha2_dev(T.sha2.SHA2_256, *a, **k), lambda m: hashlib.sha256(m).digest()),
        "sha512": (lambda *a, **k: T.sha2.sha2_dev(T.sha2.SHA2_512, *a, **k), lambda m: hashlib.sha512(m).digest()),
    }


def case_of(name):
    h = L.HASHES[name]
    assert L.crossing(h["count"], h["per_item"], h["period"]) and L.period_ok(h["period"], h["per_item"])
    return h


def pitched_rows(torch, buf, off, count, size):
    """the leading `size` bytes of the `count` items PITCH bytes apart from byte `off` of a buffer, and the gap bytes behind them, as strided views"""
    grid = buf[off:off + count * PITCH].view(count, PITCH)
    return grid[:, :size], grid[:, size:]


@pytest.mark.parametrize("name", ["keccak", "sha256", "sha512"])
def test_hash_with_the_messages_past_2_32_bytes(T, torch, name):
    h = case_of(name)
    count, in_len, out_len = h["count"], h["in_len"], h["out_len"]
    run, ref = hashers(T)[name]
    msgs = L.byte_period(in_len, seed=21, period=h["period"])
    assert (count - 1) * PITCH + in_len > L.TWO32
    L.room(torch, count * PITCH)
    ib = ob = got = None
    try:
        ib = torch.full((16 + 1 + count * PITCH,), 0x3C, dtype=torch.uint8, device="cuda")      # the bytes between two messages are never read
        head, _ = pitched_rows(torch, ib, 1, count, in_len)
        head.copy_(tile(torch, rows(torch, msgs), count))
        ob, op = L.out_buffer(torch, count * out_len, 1)
        run(count, ib.data_ptr() + 1, in_len, op, out_len, in_stride=PITCH)
        got = L.written(torch, ob, count * out_len, 1, (name, "in_stride")).view(count, out_len)
        same_rows(torch, got, rows(torch, [ref(m) for m in msgs]), (name, "in_stride"))
    finally:
        ib = ob = got = head = None
        release(torch)


@pytest.mark.parametrize("name", ["keccak", "sha256", "sha512"])
def test_hash_with_the_digests_past_2_32_bytes(T, torch, name):
    h = case_of(name)
    count, in_len, out_len = h["count"], h["in_len"], h["out_len"]
    run, ref = hashers(T)[name]
    msgs = L.byte_period(in_len, seed=22, period=h["period"])
    span = (count - 1) * PITCH + out_len
    assert span > L.TWO32
    L.room(torch, count * PITCH)
    ib = ob = got = gaps = None
    try:
        ib, view, ip = L.in_buffer(torch, count * in_len, 1)
        view.view(count, in_len).copy_(tile(torch, rows(torch, msgs), count))
        ob, op = L.out_buffer(torch, count * PITCH, 1)                        # the last pitch is all guard behind its digest
        run(count, ip, in_len, op, out_len, out_stride=PITCH)
        L.written(torch, ob, span, 1, (name, "out_stride"))
        got, gaps = pitched_rows(torch, ob, L.GUARD + 1, count, out_len)
        same_rows(torch, got, rows(torch, [ref(m) for m in msgs]), (name, "out_stride"))
        step = 1 << 16
        for lo in range(0, count, step):                                      # the gap bytes keep the guard value
            assert bool((gaps[lo:lo + step] == L.FILL).all().item()), (name, "wrote between two digests, instances from", lo)
    finally:
        ib = ob = got = gaps = view = None
        release(torch)


def poly_rows(torch, polys, signed):
    """polynomials (lists of 256 integers) as rows of 2048 bytes: 64-bit little-endian words"""
    return rows(torch, [np.asarray(p, dtype=np.int64 if signed else np.uint64).astype("<i8" if signed else "<u8").tobytes() for p in polys])


def test_sample_ntt_with_the_polynomials_past_2_32_bytes(T, torch):
    h = case_of("sample_ntt")
    count = h["count"]
    seeds = L.byte_period(34, seed=23)
    want = [K.sample_ntt(s) for s in seeds]
    L.room(torch, count * 2048 + count * 34)
    sb = ob = got = None
    try:
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        sb, view, sp = L.in_buffer(torch, count * 34, 1)
        view.view(count, 34).copy_(tile(torch, rows(torch, seeds), count))
        ob, op = L.out_buffer(torch, count * 2048, 8)
        T.fips203.sample_ntt_dev(op, count, sp, k=0, d_fail=flag.data_ptr(), io_bits=64)
        got = L.written(torch, ob, count * 2048, 8, "sample_ntt").view(count, 2048)
        same_rows(torch, got, poly_rows(torch, want, False), "sample_ntt")
        assert int(flag.item()) == 0
    finally:
        sb = ob = got = view = None
        release(torch)


def test_sample_cbd_with_the_polynomials_past_2_32_bytes(T, torch):
    h = case_of("sample_cbd")
    count, eta = h["count"], 2
    sigmas = L.byte_period(32, seed=24)
    want = [K.sample_poly_cbd(eta, K.PRF(eta, s, 0)) for s in sigmas]
    L.room(torch, count * 2048 + count * 32)
    sb = ob = got = None
    try:
        sb, view, sp = L.in_buffer(torch, count * 32, 1)
        view.view(count, 32).copy_(tile(torch, rows(torch, sigmas), count))
        ob, op = L.out_buffer(torch, count * 2048, 8)
        T.fips203.sample_cbd_dev(op, count, sp, eta, first_nonce=0, per_seed=1, io_bits=64)
        got = L.written(torch, ob, count * 2048, 8, "sample_cbd").view(count, 2048)
        same_rows(torch, got, poly_rows(torch, want, True), "sample_cbd")
    finally:
        sb = ob = got = view = None
        release(torch)


def test_image_from_and_to_fips203_with_the_images_past_2_32_bytes(T, torch):
    """16-bit residues: the images (1024 bytes per polynomial) equal the tiled images of a call on the seven polynomials of the period, and the way
    back returns the residues"""
    h = case_of("image")
    count = h["count"]
    rng = np.random.default_rng(25)
    per = rng.integers(0, K.Q, size=(L.INSTANCES, 256), dtype=np.uint16)
    per[0, :3], per[1, 255] = (0, 1, K.Q - 1), K.Q - 1
    per_rows = rows(torch, [r.astype("<u2").tobytes() for r in per])
    L.room(torch, count * (512 + 1024 + 512))
    fb = hb = rb = small = got = back = None
    try:
        small_in = per_rows.clone()
        small, smp = L.out_buffer(torch, L.INSTANCES * 1024, 4)
        T.fips203.image_from_fips203_dev(smp, L.INSTANCES, small_in.data_ptr(), io_bits=16)
        want = L.written(torch, small, L.INSTANCES * 1024, 4, "the images of the period").view(L.INSTANCES, 1024).clone()
        assert len({bytes(r) for r in want.cpu().numpy()}) == L.INSTANCES
        fb, view, fp = L.in_buffer(torch, count * 512, 2)
        view.view(count, 512).copy_(tile(torch, per_rows, count))
        hb, hp = L.out_buffer(torch, count * 1024, 4)
        T.fips203.image_from_fips203_dev(hp, count, fp, io_bits=16)
        got = L.written(torch, hb, count * 1024, 4, "image_from").view(count, 1024)
        same_rows(torch, got, want, "image_from")
        rb, rp = L.out_buffer(torch, count * 512, 2)
        T.fips203.image_to_fips203_dev(rp, count, hp, io_bits=16)
        back = L.written(torch, rb, count * 512, 2, "image_to").view(count, 512)
        same_rows(torch, back, per_rows, "image_to")
    finally:
        fb = hb = rb = small = got = back = view = want = None
        release(torch)
