"""Models of the sample fills (psf_sample_*, include/psf_mi355x.h) over the CPU oracle.

The centred-binomial contract (DESIGN.md "Randomness contract") is written here once, coefficient by coefficient over `oracle.philox`
(cbd_coeff); cbd_fill is the same rule vectorised over a numpy Philox (philox_np, itself checked against oracle.philox in the CPU suite).
uniform_fill and gauss_fill call the oracle's own orc_uniform_mod / orc_sample_z per coefficient; gauss_narrow_trace replays the narrow
SampleZ attempts in numpy to count the ties and Lemire voids a fill meets."""
import math

import numpy as np

M32 = 0xFFFFFFFF


def tag_word(tag, index):
    return (tag | ((index >> 32) << 8)) & M32


def cbd_position(i, eta):
    """(block, word, slot) of coefficient i"""
    sw = 16 // eta
    return i // (4 * sw), (i // sw) % 4, i % sw


def cbd_value(field, eta):
    """popcount(low eta bits) - popcount(high eta bits) of a 2 eta-bit field"""
    return bin(field & ((1 << eta) - 1)).count("1") - bin(field >> eta).count("1")


def cbd_coeff(seed, tag, idx, i, eta):
    """coefficient i of polynomial idx: the definition"""
    from oracle import oracle as O
    blk, word, slot = cbd_position(i, eta)
    w = O.philox(seed, blk, idx & M32, 0, tag_word(tag, idx))[word]
    return cbd_value((w >> (2 * eta * slot)) & ((1 << (2 * eta)) - 1), eta)


def philox_np(seed, c0, c1, c2, c3):
    """Philox4x32-10 over arrays (uint64 arithmetic on 32-bit values); returns four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(M32) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = seed & M32, (seed >> 32) & M32
    m = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


_POP16 = np.array([bin(v).count("1") for v in range(1 << 16)], dtype=np.int64)


def _popcount(x):
    """of values below 2^16 (a half field has at most 16 bits)"""
    return _POP16[x.astype(np.int64)]


def cbd_fill(seed, tag, first_index, count, n, eta):
    """int64 (count, n): cbd_coeff for every (first_index + c, i), vectorised"""
    sw = 16 // eta
    i = np.arange(n, dtype=np.uint64)[None, :]
    idx = (np.uint64(first_index) + np.arange(count, dtype=np.uint64))[:, None]
    tw = np.uint64(tag) | ((idx >> np.uint64(32)) << np.uint64(8))
    words = philox_np(seed, i // np.uint64(4 * sw), idx, np.uint64(0), tw)
    sel = ((i // np.uint64(sw)) % np.uint64(4)) + np.zeros_like(idx)
    w = np.choose(sel.astype(np.int64), [np.broadcast_to(x, sel.shape) for x in words])
    f = (w >> (np.uint64(2 * eta) * (i % np.uint64(sw)))) & np.uint64((1 << (2 * eta)) - 1)
    return _popcount(f & np.uint64((1 << eta) - 1)) - _popcount(f >> np.uint64(eta))


def uniform_fill(seed, tag, first_index, count, n, q):
    """uint64 (count, n) by orc_uniform_mod(seed, tag word, i, (uint32) index, q)"""
    from oracle import oracle as O
    f = O.lib().orc_uniform_mod
    out = np.empty((count, n), dtype=np.uint64)
    for c in range(count):
        idx = first_index + c
        tw, lo = tag_word(tag, idx), idx & M32
        out[c] = [f(seed, tw, i, lo, q) for i in range(n)]
    return out


def gauss_fill(seed, tag, first_index, count, n, s, center=0.0, centers=None):
    """(int64 (count, n), failed) by orc_sample_z; failed: the oracle's attempt-cap counter moved (cap, or a centre at or beyond 2^62)"""
    from oracle import oracle as O
    L = O.lib()
    f = L.orc_sample_z
    L.orc_sample_z_cap_hits.restype = __import__("ctypes").c_ulong
    cap0 = L.orc_sample_z_cap_hits()
    out = np.empty((count, n), dtype=np.int64)
    cen = None if centers is None else np.asarray(centers, dtype=np.float64).reshape(count, n)
    for c in range(count):
        idx = first_index + c
        if cen is None:
            out[c] = [f(seed, tag, idx, i, center, s) for i in range(n)]
        else:
            row = cen[c]
            out[c] = [f(seed, tag, idx, i, float(row[i]), s) for i in range(n)]
    return out, L.orc_sample_z_cap_hits() != cap0


def gauss_narrow_trace(seed, tag, first_index, count, n, center, s, stats=None):
    """The narrow SampleZ (at most 4096 candidates) of one shared centre, attempt by attempt in numpy with the exact thresholds from the
    oracle's det_exp.  Returns (values int64 (count, n), ties, voids): ties = attempts evaluated with wb == floor(rho 2^16), voids = attempts
    evaluated that Lemire's threshold discarded; `stats` (a dict) also receives "groups", the groups of four attempts drawn in all.  Every sample
    must accept within 4096 groups (true for the widths used in the tests)."""
    from oracle import oracle as O
    c6, f6 = math.ceil(6.0 * s), math.floor(6.0 * s)
    assert c6 + f6 + 1 <= 4096
    lo = math.ceil(center) - c6
    N = math.floor(center) + f6 - lo + 1
    thr = 65536 % N
    inv_s = 1.0 / s
    ru = np.empty(N, dtype=np.int64)
    tie = np.empty(N, dtype=np.int64)
    for k in range(N):
        a = (float(lo + k) - center) * inv_s
        rs = O.det_exp(-3.14159265358979323846 * (a * a)) * 65536.0
        rf = math.floor(rs)
        ru[k], tie[k] = int(rf), int(math.floor((rs - rf) * 4294967296.0))
    total = count * n
    e = np.arange(total, dtype=np.uint64)
    idx = np.uint64(first_index) + e // np.uint64(n)
    coord = e % np.uint64(n)
    tw = np.uint64(tag) | ((idx >> np.uint64(32)) << np.uint64(8))
    out = np.zeros(total, dtype=np.int64)
    todo = np.arange(total)
    ties = voids = groups = 0
    g = 0
    while todo.size:
        assert g < 4096, "a sample did not accept"
        groups += int(todo.size)
        words = philox_np(seed, coord[todo], idx[todo], np.uint64(g), tw[todo])
        done = np.zeros(todo.size, dtype=bool)
        for j in range(4):
            w = words[j].astype(np.int64)
            prod = (w >> 16) * N
            wb = w & 0xFFFF
            live = ~done
            void = live & ((prod & 0xFFFF) < thr)
            voids += int(void.sum())
            ci = prod >> 16
            is_tie = live & ~void & (wb == ru[ci])
            ties += int(is_tie.sum())
            acc = live & ~void & (wb < ru[ci])
            if is_tie.any():
                k = np.nonzero(is_tie)[0]
                side = philox_np(seed, coord[todo[k]], idx[todo[k]], np.uint64(0x80000000 | (4 * g + j)), tw[todo[k]])[0].astype(np.int64)
                acc[k] = side < tie[ci[k]]
            out[todo[acc]] = lo + ci[acc]
            done |= acc
        todo = todo[~done]
        g += 1
    if stats is not None:
        stats["groups"] = groups
    return out.reshape(count, n), ties, voids


# ---- windows: coefficients [i0, i1) of one polynomial without the rest (fills of up to 2^32 - 1 coefficients) -----------------------------------

def uniform_window(seed, tag, idx, i0, i1, q):
    """uint64 (i1 - i0,): uniform_fill's coefficients [i0, i1) of polynomial idx"""
    from oracle import oracle as O
    f = O.lib().orc_uniform_mod
    tw, lo = tag_word(tag, idx), idx & M32
    return np.array([f(seed, tw, i, lo, q) for i in range(i0, i1)], dtype=np.uint64)


def cbd_window(seed, tag, idx, i0, i1, eta):
    """int64 (i1 - i0,): cbd_fill's coefficients [i0, i1) of polynomial idx -- only the Philox blocks that meet the window are drawn"""
    sw = 16 // eta
    i = np.arange(i0, i1, dtype=np.uint64)
    words = philox_np(seed, i // np.uint64(4 * sw), np.uint64(idx & M32), np.uint64(0), np.uint64(tag_word(tag, idx)))
    sel = ((i // np.uint64(sw)) % np.uint64(4)).astype(np.int64)
    w = np.choose(sel, list(words))
    f = (w >> (np.uint64(2 * eta) * (i % np.uint64(sw)))) & np.uint64((1 << (2 * eta)) - 1)
    return _popcount(f & np.uint64((1 << eta) - 1)) - _popcount(f >> np.uint64(eta))


def gauss_window(seed, tag, idx, i0, i1, s, center=0.0, centers=None):
    """(int64 (i1 - i0,), failed): gauss_fill's coefficients [i0, i1) of polynomial idx; `centers`: the i1 - i0 centres of the window"""
    from oracle import oracle as O
    L = O.lib()
    f = L.orc_sample_z
    L.orc_sample_z_cap_hits.restype = __import__("ctypes").c_ulong
    cap0 = L.orc_sample_z_cap_hits()
    cen = None if centers is None else np.asarray(centers, dtype=np.float64).reshape(i1 - i0)
    out = np.array([f(seed, tag, idx, i, center if cen is None else float(cen[i - i0]), s) for i in range(i0, i1)], dtype=np.int64)
    return out, L.orc_sample_z_cap_hits() != cap0
