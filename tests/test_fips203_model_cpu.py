"""Self-checks of the pure-Python FIPS 203 model (tests/helpers/fips203_kpke_model.py), the anchor the device results are compared with: the zeta
table of Appendix A, NTT^-1 after NTT, MultiplyNTTs against the schoolbook product, and Decrypt(Encrypt(m)) = m for the three parameter sets."""
import random

import pytest

from tests.helpers import fips203_kpke_model as M


def test_zeta_tables_of_appendix_a():
    assert M.ZETAS[:8] == [1, 1729, 2580, 3289, 2642, 630, 1897, 848]
    assert M.GAMMAS[:4] == [17, 3312, 2761, 568]                       # 17, -17, ...
    assert pow(17, 128, M.Q) == M.Q - 1 and 3303 * 128 % M.Q == 1


def test_ntt_inverse_of_ntt_is_the_identity():
    rng = random.Random(1)
    for f in ([rng.randrange(M.Q) for _ in range(256)], [0] * 256, [M.Q - 1] * 256, [1] + [0] * 255):
        assert M.ntt_inv(M.ntt(f)) == f
        assert M.ntt(M.ntt_inv(f)) == f


def test_multiply_ntts_is_the_negacyclic_product():
    rng = random.Random(2)
    for _ in range(3):
        a = [rng.randrange(M.Q) for _ in range(256)]
        b = [rng.randrange(-M.Q + 1, M.Q) for _ in range(256)]
        assert M.ntt_inv(M.multiply_ntts(M.ntt(a), M.ntt(b))) == M.schoolbook(a, b)
    x255 = [0] * 255 + [1]
    assert M.schoolbook(x255, [0, 1] + [0] * 254) == [M.Q - 1] + [0] * 255        # X^255 X = -1


def test_samplers_on_inputs_worked_by_hand():
    assert M.sample_poly_cbd(2, bytes([0b0111_0010] + [0] * 127))[:3] == [1, 1, 0]      # fields 0010 and 0111: 1 - 0, 2 - 1
    assert M.sample_poly_cbd(3, bytes([0b11_000_111, 0b0000_1110] + [0] * 190))[:2] == [3, -1]  # bits 0-2 = 111, 3-5 = 000: 3 - 0; bits 6-8 = 110, 9-11 = 111: 2 - 3
    seed = bytes(range(32)) + bytes([62, 5])
    coef, blocks, failed = M.sample_ntt_blocks(seed)
    assert blocks == 4 and not failed and all(0 <= c < M.Q for c in coef)
    capped, _, failed3 = M.sample_ntt_blocks(seed, 3)
    assert failed3 and capped[-1] == 0 and capped[:200] == coef[:200]


@pytest.mark.parametrize("name", sorted(M.PARAMS))
def test_decrypt_of_encrypt_returns_the_message(name):
    rng = random.Random(sorted(M.PARAMS).index(name))
    d, m, r = (bytes(rng.randrange(256) for _ in range(32)) for _ in range(3))
    k, _, _, du, dv = M.PARAMS[name]
    ek, dk = M.kpke_keygen(d, name)
    assert len(ek) == 384 * k + 32 and len(dk) == 384 * k
    c = M.kpke_encrypt(ek, m, r, name)
    assert len(c) == 32 * (du * k + dv)
    assert M.kpke_decrypt(dk, c, name) == m
