"""tests/helpers/mldsa_model.py pinned by what FIPS 204 fixes.  No implementation of ML-DSA is at hand to compare with, so the model is held to the
standard's own numbers and identities: the sizes of Table 2, the first zetas of Appendix B, NTT^-1 o NTT = id and the convolution property, the
recomposition rules of Power2Round and Decompose (with the wrap at r1 = (q - 1) / (2 gamma2)), UseHint(MakeHint(z, r), r) = HighBits(r + z), the
round trips of every packing at its extreme values, HintBitPack / HintBitUnpack with the four malformed shapes, verify(sign) = 1, every single-bit
change tried gives 0, and the layout of sk with tr = H(pk)."""
import random

import pytest

from tests.helpers import mldsa_model as M

Q = M.Q
NAMES = sorted(M.PARAMS)


def test_sizes_and_parameters():
    assert {n: tuple(M.sizes(n).values()) for n in NAMES} == {"ML-DSA-44": (1312, 2560, 2420), "ML-DSA-65": (1952, 4032, 3309), "ML-DSA-87": (2592, 4896, 4627)}
    assert (Q, M.N, M.D) == (8380417, 256, 13) and Q - 1 == (1 << 13) * 1023
    assert M.PARAMS["ML-DSA-44"][6] == 95232 and M.PARAMS["ML-DSA-65"][6] == 261888 == M.PARAMS["ML-DSA-87"][6]
    for k, l, eta, tau, cb, g1, g2, beta, omega in M.PARAMS.values():
        assert beta == tau * eta


def test_zetas():
    assert M.ZETAS[1:5] == [4808194, 3765607, 3761513, 5178923]
    assert M.ZETAS[0] == 1 and pow(M.ZETA, 256, Q) == Q - 1                # 1753 is a primitive 512th root of unity
    assert pow(256, Q - 2, Q) == 8347681


def test_ntt_is_invertible_and_multiplicative():
    rng = random.Random(1)
    for _ in range(3):
        f = [rng.randrange(Q) for _ in range(256)]
        g = [rng.randrange(-4, 5) for _ in range(256)]
        assert M.ntt_inv(M.ntt(f)) == f
        assert M.ntt(M.ntt_inv(f)) == f
        assert M.ntt_inv(M.pointwise(M.ntt(f), M.ntt(g))) == M.schoolbook(f, g)
    one = [1] + [0] * 255
    assert M.ntt(one) == [1] * 256


def test_power2round_recomposes():
    rng = random.Random(2)
    for r in [0, 1, 4095, 4096, 4097, 8191, 8192, Q - 1, Q - 4096, Q - 4097] + [rng.randrange(Q) for _ in range(3000)]:
        r1, r0 = M.power2round(r)
        assert r1 * (1 << 13) + r0 == r and -(1 << 12) < r0 <= (1 << 12)
        assert 0 <= r1 < (1 << 10)
    assert M.power2round(-1) == M.power2round(Q - 1)


def test_decompose_recomposes_with_the_wrap():
    rng = random.Random(3)
    for g2 in (95232, 261888):
        m = (Q - 1) // (2 * g2)
        edge = [i * 2 * g2 + d for i in range(m + 1) for d in (-g2 - 1, -g2, -g2 + 1, -1, 0, 1, g2 - 1, g2, g2 + 1) if 0 <= i * 2 * g2 + d < Q]
        for r in edge + [rng.randrange(Q) for _ in range(3000)]:
            r1, r0 = M.decompose(r, g2)
            assert 0 <= r1 < m and -g2 <= r0 <= g2
            assert (r1 * 2 * g2 + r0) % Q == r
            if r > Q - 1 - g2:
                assert r1 == 0 and r0 == r - Q < 0                         # the wrap: r - r0 = q - 1 becomes r1 = 0, r0 - 1
            else:
                assert -g2 < r0
        assert M.decompose(Q - 1, g2) == (0, -1) and M.decompose(Q - g2, g2) == (0, -g2)


def test_use_hint_of_make_hint():
    rng = random.Random(4)
    for g2 in (95232, 261888):
        cases = [(rng.randrange(-g2, g2 + 1), rng.randrange(Q)) for _ in range(4000)]
        cases += [(z, r) for z in (-g2, -1, 0, 1, g2) for r in (0, 1, g2, g2 + 1, Q - 1, Q - g2, Q - g2 - 1, 2 * g2, 2 * g2 - 1)]
        for z, r in cases:
            assert M.use_hint(M.make_hint(z, r, g2), r, g2) == M.high_bits(r + z, g2), (g2, z, r)


def test_packings_round_trip_at_their_extremes():
    rng = random.Random(5)
    for a, b in ((2, 2), (4, 4), ((1 << 12) - 1, 1 << 12), ((1 << 17) - 1, 1 << 17), ((1 << 19) - 1, 1 << 19)):
        for w in ([-a] * 256, [b] * 256, [-a, b] * 128, [rng.randint(-a, b) for _ in range(256)]):
            data = M.bit_pack(w, a, b)
            assert len(data) == 32 * (a + b).bit_length() and M.bit_unpack(data, a, b) == w
    for b in (1023, 43, 15):
        for w in ([0] * 256, [b] * 256, [0, b] * 128, [rng.randint(0, b) for _ in range(256)]):
            data = M.simple_bit_pack(w, b)
            assert len(data) == 32 * b.bit_length() and M.simple_bit_unpack(data, b) == w
    assert M.simple_bit_pack([1] + [0] * 255, 1023)[:2] == b"\x01\x00" and M.bit_pack([2] + [2] * 255, 2, 2) == bytes(96)


def test_hint_round_trip_and_the_four_malformed_shapes():
    from tests.test_mldsa_core_cpu import malformed_hints
    rng = random.Random(6)
    for name in NAMES:
        k, omega = M.PARAMS[name][0], M.PARAMS[name][8]
        h, y, bad = malformed_hints(k, omega, rng)
        assert len(y) == omega + k and M.hint_bit_unpack(y, k, omega) == h
        assert M.hint_bit_pack(M.hint_bit_unpack(y, k, omega), omega) == y
        assert [M.hint_bit_unpack(b, k, omega) for b in bad] == [None] * 4
        full = [[0] * 256 for _ in range(k)]
        for j in range(omega):
            full[k - 1][j] = 1
        assert M.hint_bit_unpack(M.hint_bit_pack(full, omega), k, omega) == full


@pytest.fixture(scope="module")
def signed():
    out = {}
    for i, name in enumerate(NAMES):
        rng = random.Random(70 + i)
        pk, sk = M.keygen_internal(rng.randbytes(32), name)
        msg = rng.randbytes(40)
        out[name] = (pk, sk, msg, M.sign_internal(sk, msg, rng.randbytes(32), name))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_sign_then_verify_and_single_bit_changes(signed, name):
    pk, sk, msg, sig = signed[name]
    sz = M.sizes(name)
    assert (len(pk), len(sk), len(sig)) == (sz["pk"], sz["sk"], sz["sig"])
    assert M.verify_internal(pk, msg, sig, name) and M.verify_why(pk, msg, sig, name) == 0
    assert M.verify_internal(pk, msg, sig, name, mu=M.H(M.H(pk, 64) + msg, 64))
    rng = random.Random(7)

    def flip(data, pos, bit):
        b = bytearray(data)
        b[pos] ^= 1 << bit
        return bytes(b)
    for pos in [0, 31, 32, len(pk) - 1] + [rng.randrange(len(pk)) for _ in range(3)]:
        assert not M.verify_internal(flip(pk, pos, rng.randrange(8)), msg, sig, name), ("pk", pos)
    for pos in [0, len(msg) - 1, rng.randrange(len(msg))]:
        assert not M.verify_internal(pk, flip(msg, pos, rng.randrange(8)), sig, name), ("msg", pos)
    cb, omega, k = M.PARAMS[name][4], M.PARAMS[name][8], M.PARAMS[name][0]
    for pos in [0, cb - 1, cb, len(sig) - omega - k - 1, len(sig) - omega - k, len(sig) - 1] + [rng.randrange(len(sig) - omega - k) for _ in range(3)]:
        assert not M.verify_internal(pk, msg, flip(sig, pos, rng.randrange(8)), name), ("sig", pos)
    assert M.verify(pk, b"abc", M.sign(sk, b"abc", b"ctx", bytes(32), name), b"ctx", name)
    assert not M.verify(pk, b"abc", M.sign(sk, b"abc", b"ctx", bytes(32), name), b"cty", name)


@pytest.mark.parametrize("name", NAMES)
def test_sk_layout_and_tr(signed, name):
    pk, sk, _, _ = signed[name]
    k, l, eta = M.PARAMS[name][:3]
    parts = {}
    xi = random.Random(70 + NAMES.index(name)).randbytes(32)
    assert M.keygen_internal(xi, name, parts) == (pk, sk)
    eb = 32 * (2 * eta).bit_length()
    assert sk[:32] == pk[:32] == parts["rho"] and sk[32:64] == parts["K"] and sk[64:128] == M.H(pk, 64) == parts["tr"]
    assert sk[128:128 + eb * l] == b"".join(M.bit_pack(p, eta, eta) for p in parts["s1"])
    assert sk[128 + eb * l:128 + eb * (l + k)] == b"".join(M.bit_pack(p, eta, eta) for p in parts["s2"])
    assert sk[128 + eb * (l + k):] == b"".join(M.bit_pack(p, 4095, 4096) for p in parts["t0"]) and len(sk) == 128 + eb * (l + k) + 416 * k
    rho, K, tr, s1, s2, t0 = M.sk_decode(sk, name)
    assert (rho, K, tr, s1, s2, t0) == (parts["rho"], parts["K"], parts["tr"], parts["s1"], parts["s2"], parts["t0"])
    assert all(abs(x) <= eta for p in s1 + s2 for x in p)
    # t = A s1 + s2 by schoolbook products of the coefficient-domain A
    A = [[M.ntt_inv(a) for a in row] for row in M.expand_a(rho, k, l)]
    t_row0 = [0] * 256
    for a, s in zip(A[0], s1):
        t_row0 = M.poly_add(t_row0, M.schoolbook(a, s))
    t_row0 = M.poly_add(t_row0, s2[0])
    assert t_row0 == parts["t"][0]
    assert [(a << 13) + b for a, b in zip(parts["t1"][0], parts["t0"][0])] == t_row0
