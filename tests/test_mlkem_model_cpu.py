"""The pure-Python ML-KEM model of tests/helpers/mlkem_model.py (the reference of tests/test_gpu_mlkem.py) against the properties FIPS 203 gives
the outer layer: the sizes, decapsulation of an honest ciphertext, implicit rejection, and the two input checks.  No GPU, no library."""
import random

import pytest

from tests.helpers import fips203_kpke_model as M
from tests.helpers import mlkem_model as K

NAMES = sorted(M.PARAMS)


def _instance(name, salt=0):
    rng = random.Random(7 + 31 * NAMES.index(name) + salt)
    d, z, m = rng.randbytes(32), rng.randbytes(32), rng.randbytes(32)
    ek, dk = K.keygen_internal(d, z, name)
    return ek, dk, z, m


def test_sizes_table():
    assert K.sizes("ML-KEM-512") == {"ek": 800, "dk": 1632, "ct": 768, "ss": 32}
    assert K.sizes("ML-KEM-768") == {"ek": 1184, "dk": 2400, "ct": 1088, "ss": 32}
    assert K.sizes("ML-KEM-1024") == {"ek": 1568, "dk": 3168, "ct": 1568, "ss": 32}


@pytest.mark.parametrize("name", NAMES)
def test_decaps_of_encaps_returns_the_key_and_a_flipped_bit_the_rejection_key(name):
    ek, dk, z, m = _instance(name)
    sz = K.sizes(name)
    assert len(ek) == sz["ek"] and len(dk) == sz["dk"]
    k = M.PARAMS[name][0]
    assert dk[384 * k:768 * k + 32] == ek and dk[768 * k + 32:768 * k + 64] == M.H(ek) and dk[768 * k + 64:] == z
    key, c = K.encaps_internal(ek, m, name)
    assert len(key) == 32 and len(c) == sz["ct"]
    assert K.decaps_internal(dk, c, name) == key
    for pos in (0, len(c) - 1):
        bad = bytearray(c)
        bad[pos] ^= 0x10
        got = K.decaps_internal(dk, bytes(bad), name)
        assert got == M.J(z + bytes(bad)) == K.rejection_key(dk, bytes(bad), name)
        assert got != key


@pytest.mark.parametrize("name", NAMES)
def test_check_ek_rejects_q_and_4095_and_accepts_q_minus_1(name):
    ek, _, _, _ = _instance(name, 1)
    k = M.PARAMS[name][0]
    assert K.check_ek(ek, name)
    for index in (0, 1, 256 * k - 1):
        assert K.check_ek(K.set_field(ek, index, M.Q - 1), name)
        assert not K.check_ek(K.set_field(ek, index, M.Q), name)
        assert not K.check_ek(K.set_field(ek, index, 4095), name)
        changed = K.set_field(ek, index, M.Q)
        assert (int.from_bytes(changed, "little") >> (12 * index)) & 0xFFF == M.Q
        assert sum(a != b for a, b in zip(changed, ek)) <= 2
    rho_changed = bytearray(ek)
    rho_changed[-1] ^= 0xFF                                                # rho is not part of the modulus check
    assert K.check_ek(bytes(rho_changed), name)


@pytest.mark.parametrize("name", NAMES)
def test_check_dk_rejects_a_flipped_byte_of_h_and_of_the_embedded_ek(name):
    _, dk, _, _ = _instance(name, 2)
    k = M.PARAMS[name][0]
    assert K.check_dk(dk, name)
    for pos in (768 * k + 32, 768 * k + 63, 384 * k, 768 * k + 31):
        bad = bytearray(dk)
        bad[pos] ^= 1
        assert not K.check_dk(bytes(bad), name), pos
    for pos in (0, 384 * k - 1, 768 * k + 64, 768 * k + 95):              # dk_pke and z are outside the hash check
        other = bytearray(dk)
        other[pos] ^= 1
        assert K.check_dk(bytes(other), name), pos
