"""The R_q products (psf_rq.hip, psf_rq_kernels.hpp, psf_ntt.hip, psf_ntt_kernels.hpp, psf_ntt_matpoly_body.hpp, psf_ntt_fma.hip) on the MI355X at
the smallest batches in which an operand, the images or the result pass 2^32 bytes: pair products by the wave kernel (64- and 16-bit words), the
generic LDS kernel (n = 2048) and the schoolbook kernels (q = 2^30, one workgroup per pair for the negacyclic ring), the image forms, and the
matrix products with their fused and schoolbook forms.  The largest call of any other test is 65 536 batches (2 GiB), so row * N + r * 64 + lane,
pr * hat_stride, c * a_stride, o * n + cc and pair * a_stride have never addressed a byte at or past 2^32.  Element indices stay below 2^32 at
these sizes (at most 2^31 + 767): what the suite pins is every offset in bytes, and every 32-bit quantity that counts bytes or halves of words.

Instance i is instance i mod 7 of a period of operands in range for the word size (13 where 7 divides the count: 2^20 + 3 and 2^23 + 3); the
expectation is the big-integer model (tests/helpers/rq_model.py, rq_cyclic_model.py, rq_fma_model.py) on the period, and 2^32 bytes are no whole
number of periods of any array.  Operands and expectations are tiled on the device, every word of every result is compared there, every output
is prefilled with the guard byte between guard bytes one word past a 16-byte boundary.  Each test frees what it allocated."""
import time

import numpy as np
import pytest

from tests.helpers import large_cases as L
from tests.helpers import rq_cyclic_model, rq_fma_model, rq_model
from tests.helpers.slhdsa_gpu import release, same_rows

pytestmark = pytest.mark.gpu


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


def case_of(name):
    r = L.RQ[name]
    assert L.crossing(r["count"], r["per_item"], r["period"]) and L.period_ok(r["period"], r["per_item"], r["per_item"] // 2, r["n"])
    return r


def word(torch, io_bits):
    return torch.int16 if io_bits == 16 else torch.int64


def dev(torch, a, io_bits):
    """integers (non-negative residues or signed) as a device tensor of the call's words"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int16 if io_bits == 16 else np.int64))).cuda()


def tiled(torch, period, count, io_bits, off=None):
    """(buffer, pointer): `count` items that repeat the rows of `period` (period, words per item), the first one word past a 16-byte boundary"""
    wb = io_bits // 8
    per = dev(torch, period, io_bits)
    buf, view, ptr = L.in_buffer(torch, count * per.shape[1] * wb, wb if off is None else off)
    L.tile_into(torch, view.view(word(torch, io_bits)), per.reshape(-1))
    return buf, ptr


def result(torch, buf, count, words_per, io_bits, what, want):
    wb = io_bits // 8
    got = L.written(torch, buf, count * words_per * wb, wb, what, word(torch, io_bits)).view(count, words_per)
    same_rows(torch, got, dev(torch, want, io_bits), what)


def negacyclic_model(a, b, q):
    return np.array([[int(v) % q for v in rq_model.negacyclic(x, y)] for x, y in zip(a, b)], dtype=np.int64)


def pair_case(T, torch, name, ring):
    r = case_of(name)
    q, n, io, count, period = r["q"], r["n"], r["io_bits"], r["count"], r["period"]
    wb = io // 8
    a, b = L.poly_period(q, n, 31, False, period), L.poly_period(q, n, 32, True, period)
    want = negacyclic_model(a, b, q) if ring == "negacyclic" else rq_cyclic_model.poly_mul(a, b, q).astype(np.int64)
    run = T.gadget.poly_mul_negacyclic_dev if ring == "negacyclic" else T.rq.poly_mul_cyclic_dev
    L.room(torch, 3 * count * n * wb)
    ab = bb = ob = None
    try:
        ab, ap = tiled(torch, a, count, io)
        bb, bp = tiled(torch, b, count, io)
        ob, op = L.out_buffer(torch, count * n * wb, wb)
        run(ap, bp, op, q, n, count, io_bits=io)
        result(torch, ob, count, n, io, (name, ring), want)
    finally:
        ab = bb = ob = None
        release(torch)


@pytest.mark.parametrize("name", ["wave64", "wave16", "lds", "school"])
def test_negacyclic_pair_products_past_2_32_bytes(T, torch, name):
    pair_case(T, torch, name, "negacyclic")


@pytest.mark.parametrize("name", ["wave64", "school"])
def test_cyclic_pair_products_past_2_32_bytes(T, torch, name):
    pair_case(T, torch, name, "cyclic")


@pytest.mark.parametrize("ring", ["negacyclic", "cyclic"])
def test_image_forms_with_the_images_past_2_32_bytes(T, torch, ring):
    """ntt_forward_dev then poly_mul_hat_dev at hat_stride = n: the images equal the tiled images of the seven polynomials alone, and the products the model"""
    r = case_of("hat16")
    q, n, io, count, period = r["q"], r["n"], r["io_bits"], r["count"], r["period"]
    a, b = L.poly_period(q, n, 33, False, period), L.poly_period(q, n, 34, True, period)
    want = negacyclic_model(a, b, q) if ring == "negacyclic" else rq_cyclic_model.poly_mul(a, b, q).astype(np.int64)
    fwd, mul = (T.gadget.ntt_forward_dev, T.gadget.poly_mul_hat_dev) if ring == "negacyclic" else (T.rq.ntt_forward_cyclic_dev, T.rq.poly_mul_hat_cyclic_dev)
    L.room(torch, count * n * (2 + 4 + 2 + 2))
    ab = bb = hb = ob = sb = hat = small = None
    try:
        sb, sp = tiled(torch, a, period, io, off=0)
        small, smp = L.out_buffer(torch, period * n * 4, 4)
        fwd(sp, smp, q, n, period, io_bits=io)
        small = L.written(torch, small, period * n * 4, 4, (ring, "the images of the period"), torch.int32).view(period, n).clone()
        ab, ap = tiled(torch, a, count, io)
        hb, hp = L.out_buffer(torch, count * n * 4, 4)
        fwd(ap, hp, q, n, count, io_bits=io)
        hat = L.written(torch, hb, count * n * 4, 4, (ring, "forward"), torch.int32).view(count, n)
        same_rows(torch, hat, small, (ring, "forward"))
        ab = None
        release(torch)
        bb, bp = tiled(torch, b, count, io)
        ob, op = L.out_buffer(torch, count * n * 2, 2)
        mul(hp, n, bp, op, q, n, count, io_bits=io)
        result(torch, ob, count, n, io, (ring, "mul_hat"), want)
    finally:
        ab = bb = hb = ob = sb = hat = small = None
        release(torch)


def matrix_period(r, trans_a, seed):
    """(A as stored (period, 4 n), B (period, 2 n), E (period, 2 n), the model's C and E - C as (period, 2 n)) for rows, inner, cols = 2, 2, 1"""
    q, n, period = r["q"], r["n"], r["period"]
    assert (r["rows"], r["inner"], r["cols"]) == (2, 2, 1)
    A = L.poly_period(q, 4 * n, seed, False, period).reshape(period, 2, 2, n)
    Bm = L.poly_period(q, 2 * n, seed + 1, True, period).reshape(period, 2, 1, n)
    E = L.poly_period(q, 2 * n, seed + 2, True, period).reshape(period, 2, 1, n)
    math_a = A.transpose(0, 2, 1, 3) if trans_a else A                       # stored inner x rows
    prod = np.stack([rq_model.matpoly_mul(x, y, q) for x, y in zip(math_a, Bm)]).astype(np.int64)
    fused = np.stack([rq_fma_model.matpoly_mul_add(x, y, e, q, sign=-1) for x, y, e in zip(math_a, Bm, E)]).astype(np.int64)
    flat = lambda x: x.reshape(period, -1)
    return flat(A), flat(Bm), flat(E), flat(prod), flat(fused)


@pytest.mark.parametrize("name,trans_a", [("mat64", 0), ("mat64", 1), ("matschool", 0)])
def test_matrix_products_with_a_past_2_32_bytes(T, torch, name, trans_a):
    r = case_of(name)
    q, n, io, count = r["q"], r["n"], r["io_bits"], r["count"]
    A, Bm, _, prod, _ = matrix_period(r, trans_a, 41)
    L.room(torch, count * n * 8 * 8)
    ab = bb = ob = None
    try:
        ab, ap = tiled(torch, A, count, io)
        bb, bp = tiled(torch, Bm, count, io)
        ob, op = L.out_buffer(torch, count * 2 * n * 8, 8)
        T.rq.matpoly_mul_dev(ap, bp, op, q, n, count, 2, 2, 1, a_stride=4, trans_a=trans_a, io_bits=io)
        result(torch, ob, count, 2 * n, io, (name, trans_a), prod)
    finally:
        ab = bb = ob = None
        release(torch)


def test_fused_matrix_product_in_place_with_a_past_2_32_bytes(T, torch):
    """C = E - A B with d_e == d_c: the output starts as E between its guards"""
    r = case_of("mat64")
    q, n, io, count = r["q"], r["n"], r["io_bits"], r["count"]
    A, Bm, E, _, fused = matrix_period(r, 0, 43)
    L.room(torch, count * n * 8 * 8)
    ab = bb = ob = None
    try:
        ab, ap = tiled(torch, A, count, io)
        bb, bp = tiled(torch, Bm, count, io)
        ob, op = L.out_buffer(torch, count * 2 * n * 8, 8)
        L.tile_into(torch, ob[L.GUARD + 8:L.GUARD + 8 + count * 2 * n * 8].view(torch.int64), dev(torch, E, io).reshape(-1))
        T.rq.matpoly_mul_add_dev(ap, bp, op, op, q, n, count, 2, 2, 1, a_stride=4, trans_a=0, sign=-1, io_bits=io)
        result(torch, ob, count, 2 * n, io, "mul_add in place", fused)
    finally:
        ab = bb = ob = None
        release(torch)


def test_matrix_product_from_images_past_2_32_bytes(T, torch):
    """matpoly_mul_hat_dev at 16-bit words, hat_stride = 4 n: the images of A (4 KiB per batch) pass 2^32 bytes"""
    r = case_of("mathat16")
    q, n, io, count = r["q"], r["n"], r["io_bits"], r["count"]
    A, Bm, _, prod, _ = matrix_period(r, 0, 45)
    L.room(torch, count * n * (8 + 16 + 4 + 4))
    ab = bb = hb = ob = None
    try:
        ab, ap = tiled(torch, A, count, io)
        hb, hp = L.out_buffer(torch, count * 4 * n * 4, 4)
        T.gadget.ntt_forward_dev(ap, hp, q, n, count * 4, io_bits=io)
        L.written(torch, hb, count * 4 * n * 4, 4, "the images of A")
        ab = None
        release(torch)
        bb, bp = tiled(torch, Bm, count, io)
        ob, op = L.out_buffer(torch, count * 2 * n * 2, 2)
        T.rq.matpoly_mul_hat_dev(hp, bp, op, q, n, count, 2, 2, 1, hat_stride=4 * n, trans_a=0, io_bits=io)
        result(torch, ob, count, 2 * n, io, "matpoly_mul_hat", prod)
    finally:
        ab = bb = hb = ob = None
        release(torch)
