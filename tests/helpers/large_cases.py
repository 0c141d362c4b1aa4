"""What the suites that run the general-purpose units past 2^32 bytes and words share (tests/test_gpu_sample_fill_large.py,
test_gpu_compression_large.py, test_gpu_hash_large.py, test_gpu_rq_large.py; checked without a GPU by tests/test_large_cases_cpu.py): the
periods of the inputs, the counts at which an array crosses 2^32 with their assertions, the shapes of every case, the windows in which a fill
is compared with the model, and the guarded device buffers.  Nothing here imports torch or the library: both are arguments.

Periods.  An index that wrapped at 2^32 reads or writes inside the same buffer, so nothing faults; it is seen only if the data at the wrapped
place differs.  Batches of instances repeat with period 7 (2^k mod 7 is never 0), flat arrays of values with period 8 * 8191 = 65 528 (a
whole number of bytes at every width d; 2^32 mod 65 528 = 64), per-element centres with period 65 521 (a prime).  `period_ok` asserts, in
every unit a kernel might index by, that 2^32 is not a whole number of periods."""
import random

TWO32 = 1 << 32
INSTANCES = 7                      # period of a batch of instances
INSTANCES_B = 13                   # the same where 7 divides the count: 2^k + 3 for k = 20 and 23 (2^23 + 3 is a multiple of 11 too); 2^k mod 13 is never 0
VALUES = 8 * 8191                  # period of a flat array of values: 65 528
CENTRES = 65521                    # period of the per-element centres (prime)
GUARD, FILL = 64, 0xA5             # guard bytes on each side of an output, and the byte every output is prefilled with
WINDOW = 512                       # coefficients per model window
CHUNK = 1 << 18                    # polynomials per small fill of the concatenation a large fill is compared with


# ---- periods and crossings ---------------------------------------------------------------------------------------------------------------------
def period_ok(period, *unit_sizes):
    """2^32 is not a whole number of periods, counted in items and in every given size of an item (its bytes, its words)"""
    for size in (1,) + tuple(unit_sizes):
        assert size >= 1 and TWO32 % (period * size) != 0, (period, size)
    return True


def crossing_count(per_item, target=TWO32):
    """the smallest count at which an array of `per_item` units per item reaches `target` units, plus 3"""
    return (target + per_item - 1) // per_item + 3


def crossing(count, per_item, period=INSTANCES, target=TWO32):
    """`count` is the smallest batch at which the array reaches 2^32 units, plus 3: a ragged last wave, workgroup and period"""
    assert per_item * (count - 3) >= target > per_item * (count - 4), (count, per_item)
    assert count % 64 != 0 and count % 256 != 0 and count % period != 0, count
    return True


def ragged(length, num, den=1, period=VALUES):
    """a flat array of `length` values of num / den units each (bytes of a word, bytes of a d-bit field, 1 for words) passes 2^32 units by less than
    78 values, and its length is a multiple of neither 64, nor 256, nor the period"""
    assert length * num > TWO32 * den >= (length - 78) * num, (length, num, den)
    assert length % 64 != 0 and length % 256 != 0 and length % period != 0, length
    return True


def encoded_len(d, extra=77):
    """the smallest number of d-bit values whose encoding reaches 2^32 bytes, plus 77"""
    return (TWO32 * 8 + d - 1) // d + extra


# ---- the shapes of every case ------------------------------------------------------------------------------------------------------------------
# fills: name -> (n, io_bits, count, unit the crossing is counted in, units per polynomial)
FILLS = {
    "F1": dict(n=256, io_bits=64, count=(1 << 21) + 3, unit="bytes", per_item=256 * 8),
    "F2": dict(n=256, io_bits=16, count=(1 << 24) + 3, unit="words", per_item=256),
    "F3": dict(n=TWO32 - 1, io_bits=16, count=2, unit="words", per_item=TWO32 - 1),
}
F1_KINDS = [("uniform", dict(q=3329)), ("cbd", dict(eta=3)), ("gauss", dict(s=8.0, center=0.5)), ("gauss", dict(s=400.0, center=0.5))]
F2_KINDS = [("uniform", dict(q=3329)), ("cbd", dict(eta=3)), ("gauss", dict(s=8.0, center=0.5))]
F3_KINDS = [("uniform", dict(q=3329)), ("cbd", dict(eta=2))]

# compression and byte encodings: the length, and num / den = the units per value of the array that crosses (words, bytes of a word, bytes of a field)
MAPS = {
    "compress16": dict(q=3329, d=10, io_bits=16, length=TWO32 + 77, num=1, den=1),                                # 2^32 words (8 GiB)
    "compress64": dict(q=3329, d=11, io_bits=64, length=(1 << 29) + 77, num=8, den=1),
    "digits64": dict(q=3329, base=4, io_bits=64, length=(1 << 29) + 77, num=8, den=1),
    "bytes12": dict(q=3329, d=12, io_bits=16, length=encoded_len(12), num=12, den=8),                             # the bytes pass 2^32
    "bytes1": dict(q=0, d=1, io_bits=16, length=TWO32 + 77, num=1, den=1),                                        # the values pass 2^32 words
    "fused10": dict(q=3329, d=10, io_bits=16, length=encoded_len(10), num=10, den=8),
}

# hashes, FIPS 203 samplers and image interop: count and the bytes per instance of the array that crosses
HASHES = {
    "keccak": dict(count=(1 << 20) + 3, per_item=4096, in_len=33, out_len=32),
    "sha256": dict(count=(1 << 20) + 3, per_item=4096, in_len=65, out_len=32),
    "sha512": dict(count=(1 << 20) + 3, per_item=4096, in_len=65, out_len=64),
    "sample_ntt": dict(count=(1 << 21) + 3, per_item=256 * 8),
    "sample_cbd": dict(count=(1 << 21) + 3, per_item=256 * 8),
    "image": dict(count=(1 << 22) + 3, per_item=256 * 4),
}

# R_q products: count and the bytes per instance of the array that crosses
RQ = {
    "wave64": dict(q=3329, n=256, io_bits=64, count=(1 << 21) + 3, per_item=256 * 8),
    "wave16": dict(q=3329, n=256, io_bits=16, count=(1 << 23) + 3, per_item=256 * 2),
    "lds": dict(q=3329, n=2048, io_bits=64, count=(1 << 18) + 3, per_item=2048 * 8),
    "school": dict(q=1 << 30, n=64, io_bits=64, count=(1 << 23) + 3, per_item=64 * 8),
    "hat16": dict(q=3329, n=256, io_bits=16, count=(1 << 22) + 3, per_item=256 * 4),                              # the images
    "mat64": dict(q=3329, n=256, io_bits=64, count=(1 << 19) + 3, per_item=4 * 256 * 8, rows=2, inner=2, cols=1),  # A
    "mathat16": dict(q=3329, n=256, io_bits=16, count=(1 << 20) + 3, per_item=4 * 256 * 4, rows=2, inner=2, cols=1),  # the images of A
    "matschool": dict(q=1 << 30, n=64, io_bits=64, count=(1 << 21) + 3, per_item=4 * 64 * 8, rows=2, inner=2, cols=1),
}

for _case in list(HASHES.values()) + list(RQ.values()):                  # the period of each batch of instances: 7, or 13 where 7 divides the count
    _case["period"] = INSTANCES_B if _case["count"] % INSTANCES == 0 else INSTANCES

# the limits of the entry points (include/psf_mi355x.h and the checks in front of every launch)
MAX_GRID = (1 << 31) - 1           # workgroups of one launch
FILL_INDEX_CAP = 1 << 56


def within_limits():
    """every listed count is one its entry point accepts, in plain arithmetic (tests/test_large_cases_cpu.py also asks the entry points)"""
    for f in FILLS.values():
        assert 0 < f["n"] < TWO32 and f["count"] * f["n"] <= (1 << 64) // 16 and f["count"] <= FILL_INDEX_CAP
    for m in MAPS.values():
        assert m["length"] * max(m.get("d", 1), m["io_bits"] // 8) < 1 << 64
    for h in HASHES.values():
        assert (h["count"] + 63) // 64 <= MAX_GRID
    for r in RQ.values():
        assert r["n"] <= 8192 and r["count"] * r.get("rows", 1) * r.get("cols", 1) <= MAX_GRID       # the schoolbook pair kernel: one workgroup per pair
    return True


# ---- period builders ----------------------------------------------------------------------------------------------------------------------------
def value_period(q, seed, bits=16):
    """65 528 values below q (q = 0: any value of `bits` bits), among them 0, 1, q - 1 and the neighbours of q / 2; a numpy uint64 array"""
    import numpy as np
    rng = np.random.default_rng(seed)
    top = q if q else 1 << bits
    v = rng.integers(0, top, size=VALUES, dtype=np.uint64)
    edge = [0, 1, top - 1, top // 2, top // 2 + 1, max(top // 2 - 1, 0)]
    v[:len(edge)] = edge
    return v


def centre_period(seed=2024):
    """65 521 centres: fractions in (-50, 50) with runs of exact integers and of half-integers"""
    import numpy as np
    rng = np.random.default_rng(seed)
    cen = rng.uniform(-50.0, 50.0, size=CENTRES)
    cen[1000:1256] = np.round(cen[1000:1256])
    cen[2000:2256] = np.floor(cen[2000:2256]) + 0.5
    return cen


def poly_period(q, n, seed, signed, period=INSTANCES):
    """`period` polynomials of n coefficients: residues in [0, q), or (signed) integers in (-q, q); a numpy int64 array (period, n)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    lo = -(q - 1) if signed else 0
    p = rng.integers(lo, q, size=(period, n), dtype=np.int64)
    p[0, 0], p[1, n - 1], p[2, 0] = q - 1, q - 1, lo
    return p


def byte_period(size, seed, period=INSTANCES):
    """`period` byte strings of `size` bytes"""
    rng = random.Random(seed)
    return [rng.randbytes(size) for _ in range(period)]


# ---- windows ------------------------------------------------------------------------------------------------------------------------------------
def window_starts(total, word_bytes, seed, also=(), width=WINDOW, extra=8):
    """where a fill of `total` words is compared with the model, as sorted flat offsets of windows of `width` words: the first window, the one that holds
    the word at byte 2^32 - 1 and the next, the last, those in `also` and `extra` at seeded pseudo-random places"""
    assert total >= 2 * width
    at = (TWO32 - 1) // word_bytes // width * width
    starts = {0, total - width} | set(also)
    if at + 2 * width <= total:
        starts |= {at, at + width}
    rng = random.Random(seed)
    starts |= {rng.randrange(0, total - width) for _ in range(extra)}
    assert all(0 <= s <= total - width for s in starts)
    return sorted(starts)


def pieces(e0, e1, n):
    """the flat offsets [e0, e1) of a fill of polynomials of n coefficients as (polynomial, i0, i1) runs"""
    out = []
    while e0 < e1:
        c, i0 = divmod(e0, n)
        i1 = min(n, i0 + (e1 - e0))
        out.append((c, i0, i1))
        e0 += i1 - i0
    return out


def f3_windows(n, seed, width=WINDOW):
    """the windows of a fill of two polynomials of n coefficients: the start, around coefficient 2^31, the last of polynomial 0 with the first of
    polynomial 1, the last of polynomial 1 and eight seeded ones"""
    rng = random.Random(seed)
    starts = {0, (1 << 31) - width // 2, n - width, n, 2 * n - width} | {rng.randrange(0, 2 * n - width) for _ in range(8)}
    return sorted(starts)


# ---- device buffers (torch is an argument) ------------------------------------------------------------------------------------------------------
def room(torch, need):
    """skip when the device has less free memory than the case allocates (never on a 288 GB MI355X: the largest case takes under 40 GB)"""
    import pytest
    free, _ = torch.cuda.mem_get_info()
    if free < need + (2 << 30):
        pytest.skip(f"{free} bytes of device memory are free; the test needs {need} bytes plus {2 << 30}")


def out_buffer(torch, nbytes, off):
    """`nbytes` prefilled with the guard byte between two guards, the first byte `off` bytes past a 16-byte boundary; (tensor, pointer)"""
    buf = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + GUARD + off


def written(torch, buf, nbytes, off, what, dtype=None):
    """the nbytes a call wrote as a view of the buffer (of `dtype` words), after checking on the device that both guards are untouched"""
    torch.cuda.synchronize()
    lo = GUARD + off
    assert bool((buf[:lo] == FILL).all().item()), (what, "wrote before the output")
    assert bool((buf[lo + nbytes:] == FILL).all().item()), (what, "wrote beyond the output")
    part = buf[lo:lo + nbytes]
    return part if dtype is None else part.view(dtype)


def in_buffer(torch, nbytes, off):
    """an input buffer whose first byte is `off` bytes past a 16-byte boundary: (tensor, the nbytes as a view, pointer)"""
    buf = torch.zeros((16 + off + nbytes,), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + nbytes], buf.data_ptr() + off


def tile_into(torch, dst, period):
    """dst[i] = period[i mod len(period)] for a flat device tensor dst, without a temporary of dst's size"""
    p, total = period.numel(), dst.numel()
    full = total // p
    if full:
        dst[:full * p].view(full, p).copy_(period.view(1, p).expand(full, p))
    if total % p:
        dst[full * p:].copy_(period[:total % p])


def same_tiled(torch, got, period, what, slab=1 << 27):
    """got[i] == period[i mod len(period)] for a flat device tensor, compared on the device slab by slab; names the first places that differ"""
    p, total = period.numel(), got.numel()
    rows_per = max(1, slab // p)
    want = period.view(1, p).expand(rows_per, p)
    full = total // p
    bad = []
    for lo in range(0, full, rows_per):
        k = min(rows_per, full - lo)
        ne = got[lo * p:(lo + k) * p].view(k, p) != want[:k]
        if bool(ne.any().item()):
            bad += [lo * p + int(i) for i in ne.view(-1).nonzero().flatten()[:8].tolist()]
            break
    if not bad and total % p:
        ne = got[full * p:] != period[:total % p]
        if bool(ne.any().item()):
            bad += [full * p + int(i) for i in ne.nonzero().flatten()[:8].tolist()]
    assert not bad, (what, "first differing places:", bad[:8], "of", total)


def same_flat(torch, a, b, what, slab=1 << 28):
    """two flat device tensors of one length are equal, compared slab by slab; names the first place that differs"""
    assert a.numel() == b.numel(), (what, a.numel(), b.numel())
    for lo in range(0, a.numel(), slab):
        x, y = a[lo:lo + slab], b[lo:lo + slab]
        if not torch.equal(x, y):
            first = lo + int((x != y).nonzero().flatten()[0].item())
            raise AssertionError((what, "first differing place:", first, "of", a.numel()))
