"""The uniform, centred-binomial and discrete-Gaussian fills on the MI355X where one output passes 2^32 bytes (F1: 2^21 + 3 polynomials of 256
64-bit words), 2^32 words (F2: 2^24 + 3 polynomials of 256 16-bit words) and where a single polynomial has 2^32 - 1 coefficients (F3, the
largest n the header allows).  No other test fills more than 2^22 + 77 words, so the reciprocal divisions (div_u64, locate, div_u32), the
32-bit coefficient counters and the grid-stride and tile offsets of psf_sample.hip have never met an offset at or past 2^32; a truncated one
stays inside the buffer and faults nothing.

A fill is a pure function of (seed, tag, polynomial index, coefficient), so the references need no input of the buffer's size.  F1 and F2: the
large fill equals, over the whole buffer and on the device, the concatenation of fills of at most 2^18 polynomials at advancing first_index
(every flat offset of those is small), and it equals the model (tests/helpers/sample_fill_model.py, windowed forms) in windows of 512
coefficients: the first, the two around byte 2^32 - 1, the last and eight seeded ones.  F3: model windows at the start, around coefficient
2^31, across the boundary of the two polynomials, at the end and eight seeded ones; polynomial 1 equals a count = 1 fill at first_index + 1;
and the whole fill equals the same fill written one word further from the 16-byte boundary (another head / vector / tile split), compared
slab by slab.  Every output is prefilled with the guard byte and sits one word past a 16-byte boundary between guard bytes; the failure flag
of every Gaussian case stays 0.  Nothing of a buffer's size is copied to the host, and each test frees what it allocated."""
import time

import numpy as np
import pytest

from tests.helpers import large_cases as L
from tests.helpers import sample_fill_model as M
from tests.helpers.slhdsa_gpu import release

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED12345678
FIRST = 5


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


def word(torch, io_bits):
    return torch.int16 if io_bits == 16 else torch.int64


def device_fill(T, torch, kind, kw, ptr, count, n, io_bits, first, tag, flag=None, d_centers=None):
    """one device fill; returns the milliseconds it took on the device"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if kind == "uniform":
        T.sample.sample_uniform_dev(ptr, count, n, kw["q"], SEED, tag=tag, first_index=first, io_bits=io_bits)
    elif kind == "cbd":
        T.sample.sample_cbd_dev(ptr, count, n, kw["eta"], SEED, tag=tag, first_index=first, io_bits=io_bits)
    else:
        T.sample.sample_discrete_gauss_dev(ptr, count, n, kw["s"], SEED, center=kw.get("center", 0.0), d_centers=d_centers, d_fail=flag.data_ptr(),
                                           tag=tag, first_index=first, io_bits=io_bits)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def model_window(kind, kw, tag, first, n, e0, e1, centres=None):
    """flat offsets [e0, e1) of the fill by the model, as int64"""
    out, at = [], 0
    for c, i0, i1 in L.pieces(e0, e1, n):
        if kind == "uniform":
            part = M.uniform_window(SEED, tag, first + c, i0, i1, kw["q"]).astype(np.int64)
        elif kind == "cbd":
            part = M.cbd_window(SEED, tag, first + c, i0, i1, kw["eta"])
        else:
            cen = None if centres is None else centres[at:at + i1 - i0]
            part, failed = M.gauss_window(SEED, tag, first + c, i0, i1, kw["s"], center=kw.get("center", 0.0), centers=cen)
            assert not failed
        out.append(part)
        at += i1 - i0
    return np.concatenate(out)


def check_windows(torch, big, starts, kind, kw, tag, first, n, centres=None):
    for e0 in starts:
        got = big[e0:e0 + L.WINDOW].cpu().numpy().astype(np.int64)
        cen = None if centres is None else centres[e0:e0 + L.WINDOW].cpu().numpy()
        want = model_window(kind, kw, tag, first, n, e0, e0 + L.WINDOW, cen)
        assert np.array_equal(got, want), (kind, kw, "window at", e0, "first differing offset", e0 + int(np.nonzero(got != want)[0][0]))


def concatenation_case(T, torch, shape, kind, kw, tag, per_element=False):
    n, io_bits, count = shape["n"], shape["io_bits"], shape["count"]
    wb = io_bits // 8
    total, nbytes = count * n, count * n * wb
    assert L.crossing(count, shape["per_item"])
    assert (total * wb > L.TWO32) if shape["unit"] == "bytes" else (total > L.TWO32)
    if per_element:
        assert L.period_ok(L.CENTRES, 8) and total * 8 > L.TWO32 and total % L.CENTRES != 0
    L.room(torch, nbytes * (3 if per_element else 1) + L.CHUNK * n * wb)
    buf = cbuf = cen_buf = big = cen = None
    try:
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        cptr0 = None
        if per_element:
            cen_buf, view, cptr0 = L.in_buffer(torch, total * 8, 8)
            cen = view.view(torch.float64)
            L.tile_into(torch, cen, torch.from_numpy(L.centre_period()).cuda())
        buf, ptr = L.out_buffer(torch, nbytes, wb)
        ms = device_fill(T, torch, kind, kw, ptr, count, n, io_bits, FIRST, tag, flag, cptr0)
        print(f"\n{kind} {kw} {count} x {n} x {io_bits} bits: {ms:.1f} ms on the device, {total / ms / 1e6:.1f} G values/s")
        big = L.written(torch, buf, nbytes, wb, (kind, kw), word(torch, io_bits))
        also = (L.TWO32 - L.WINDOW // 2,) if total >= L.TWO32 + L.WINDOW // 2 else ()         # F2: around word 2^32
        check_windows(torch, big, L.window_starts(total, wb, seed=tag, also=also), kind, kw, tag, FIRST, n, cen)
        for c0 in range(0, count, L.CHUNK):
            k = min(L.CHUNK, count - c0)
            if cbuf is None or k != L.CHUNK:
                cbuf = None
                cbuf, cptr = L.out_buffer(torch, k * n * wb, 0)
            else:
                cbuf.fill_(L.FILL)
            device_fill(T, torch, kind, kw, cptr, k, n, io_bits, FIRST + c0, tag, flag, None if cptr0 is None else cptr0 + c0 * n * 8)
            part = L.written(torch, cbuf, k * n * wb, 0, (kind, kw, "chunk at", c0), word(torch, io_bits))
            assert torch.equal(big[c0 * n:(c0 + k) * n], part), (kind, kw, "the large fill differs from the fill of polynomials", c0, "to", c0 + k)
        assert int(flag.item()) == 0
    finally:
        buf = cbuf = cen_buf = big = cen = part = view = None
        release(torch)


@pytest.mark.parametrize("kind,kw", L.F1_KINDS, ids=["uniform", "cbd", "gauss_table", "gauss_general"])
def test_f1_fill_past_2_32_bytes(T, torch, kind, kw):
    concatenation_case(T, torch, L.FILLS["F1"], kind, kw, tag=70 + L.F1_KINDS.index((kind, kw)))


def test_f1_gauss_with_per_element_centres_past_2_32_bytes(T, torch):
    concatenation_case(T, torch, L.FILLS["F1"], "gauss", dict(s=8.0, center=float("nan")), tag=75, per_element=True)


@pytest.mark.parametrize("kind,kw", L.F2_KINDS, ids=["uniform", "cbd", "gauss_table"])
def test_f2_fill_past_2_32_words(T, torch, kind, kw):
    concatenation_case(T, torch, L.FILLS["F2"], kind, kw, tag=80 + L.F2_KINDS.index((kind, kw)))


def whole_polynomial_case(T, torch, kind, kw, tag, count):
    """F3: `count` polynomials of 2^32 - 1 coefficients at 16-bit words, the first of index 2^32 - 1 (the second has another tag word)"""
    n, io_bits, wb = L.FILLS["F3"]["n"], 16, 2
    first = (1 << 32) - 1
    total, nbytes = count * n, count * n * wb
    assert n == L.TWO32 - 1                                                  # the boundary of the two polynomials at flat offset 2^32 - 1
    L.room(torch, 2 * nbytes)
    a_buf = b_buf = a = b = None
    try:
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        a_buf, a_ptr = L.out_buffer(torch, nbytes, wb)
        ms = device_fill(T, torch, kind, kw, a_ptr, count, n, io_bits, first, tag, flag)
        print(f"\n{kind} {kw} {count} x (2^32 - 1) x 16 bits: {ms:.1f} ms on the device, {total / ms / 1e6:.1f} G values/s")
        a = L.written(torch, a_buf, nbytes, wb, (kind, kw), torch.int16)
        starts = L.f3_windows(n, seed=tag) if count == 2 else L.window_starts(n, wb, seed=tag, also=((1 << 31) - L.WINDOW // 2,))
        check_windows(torch, a, starts, kind, kw, tag, first, n)
        b_buf, b_ptr = L.out_buffer(torch, nbytes, 2 * wb)                      # one word further from the boundary
        device_fill(T, torch, kind, kw, b_ptr, count, n, io_bits, first, tag, flag)
        b = L.written(torch, b_buf, nbytes, 2 * wb, (kind, kw, "second offset"), torch.int16)
        L.same_flat(torch, a, b, (kind, kw, "the fill at one word and at two words past a 16-byte boundary"))
        b = b_buf = None
        release(torch)
        if count == 2:
            b_buf, b_ptr = L.out_buffer(torch, n * wb, 0)
            device_fill(T, torch, kind, kw, b_ptr, 1, n, io_bits, first + 1, tag, flag)
            b = L.written(torch, b_buf, n * wb, 0, (kind, kw, "polynomial 1 alone"), torch.int16)
            L.same_flat(torch, a[n:], b, (kind, kw, "polynomial 1 of the fill and a fill of it alone"))
        assert int(flag.item()) == 0
    finally:
        a_buf = b_buf = a = b = None
        release(torch)


@pytest.mark.parametrize("kind,kw", L.F3_KINDS, ids=["uniform", "cbd"])
def test_f3_two_polynomials_of_2_32_minus_1_coefficients(T, torch, kind, kw):
    whole_polynomial_case(T, torch, kind, kw, tag=90 + L.F3_KINDS.index((kind, kw)), count=2)


def test_f3_gauss_table_over_one_polynomial_of_2_32_minus_1_coefficients(T, torch):
    """the table kernel at the largest n: 2^21 waves of 2048 samples, the last one ragged"""
    whole_polynomial_case(T, torch, "gauss", dict(s=8.0, center=0.5), tag=95, count=1)
