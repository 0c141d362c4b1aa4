"""Pins the pure-Python model of SLH-DSA (tests/helpers/slhdsa_model.py) that the device and the C++ core are compared with: the sizes of FIPS 205
Table 2, the digest length formula, base_2b and the WOTS+ checksum on hand-computed inputs, sign -> verify, the identity pkFromSig(sign(.)) = node for
every leaf of the toy set's XMSS and FORS trees, rejection of a flipped bit in every region of a signature, in M and in pk, and the 64-bit idx_tree of
SLH-DSA-SHAKE-256f.  No other SLH-DSA implementation exists on the hosts the suite runs on: these identities, and the independent restatement in C++
(tests/test_slhdsa_cpu.py), are what stands behind "equal to the model"."""
import random

import pytest

from tests.helpers import slhdsa_cases as K
from tests.helpers import slhdsa_model as M

TABLE2 = {  # name: (n, h, d, h', a, k, m, pk bytes, sig bytes)
    "SLH-DSA-SHAKE-128s": (16, 63, 7, 9, 12, 14, 30, 32, 7856),
    "SLH-DSA-SHAKE-128f": (16, 66, 22, 3, 6, 33, 34, 32, 17088),
    "SLH-DSA-SHAKE-192s": (24, 63, 7, 9, 14, 17, 39, 48, 16224),
    "SLH-DSA-SHAKE-192f": (24, 66, 22, 3, 8, 33, 42, 48, 35664),
    "SLH-DSA-SHAKE-256s": (32, 64, 8, 8, 14, 22, 47, 64, 29792),
    "SLH-DSA-SHAKE-256f": (32, 68, 17, 4, 9, 35, 49, 64, 49856),
}
F128 = "SLH-DSA-SHAKE-128f"


def test_sizes_of_table_2():
    assert sorted(TABLE2) == sorted(M.NAMES)
    for name, (n, h, d, hp, a, k, m, pk, sig) in TABLE2.items():
        assert tuple(M.PARAMS[name]) == (n, h, d, hp, a, k, m)
        assert h == d * hp
        assert M.sizes(name) == {"pk": pk, "sk": 2 * pk, "sig": sig}
        assert M.wots_len(name) == (2 * n, 3, 2 * n + 3)
        assert M.IDS[name] == list(TABLE2).index(name)


def test_the_digest_length_formula():
    for name, s in M.PARAMS.items():
        assert s.m == -(-s.k * s.a // 8) - (-(s.h - s.hp) // 8) - (-s.hp // 8), name


def test_base_2b_on_hand_computed_inputs():
    assert M.base_2b(bytes([0x12, 0x34]), 4, 4) == [1, 2, 3, 4]
    assert M.base_2b(bytes([0b10110011, 0b01000000]), 3, 3) == [0b101, 0b100, 0b110]
    assert M.base_2b(bytes([0xAB, 0xCD, 0xEF]), 12, 2) == [0xABC, 0xDEF]
    assert M.base_2b(bytes([0xFF, 0x00, 0xFF]), 6, 4) == [0b111111, 0b110000, 0b000011, 0b111111]
    assert M.base_2b(bytes([0x80, 0x01]), 14, 1) == [0x2000]
    assert M.to_byte(0x0102, 4) == bytes([0, 0, 1, 2]) and M.to_int(bytes([1, 2, 3])) == 0x010203


def test_the_checksum_on_hand_computed_inputs():
    for name in M.NAMES:
        n = M.PARAMS[name].n
        len1 = 2 * n
        zero, ones = M.wots_digits(name, bytes(n)), M.wots_digits(name, bytes([0xFF] * n))
        csum = 15 * len1                                                   # all-zero digest: every digit contributes w - 1
        assert zero == [0] * len1 + [csum >> 8, (csum >> 4) & 15, csum & 15]
        assert ones == [15] * len1 + [0, 0, 0]                             # all-0xFF digest: csum 0
    # n = 16: 0x01 0x23 ... : digits are the nibbles; csum = sum(15 - d)
    m1 = bytes([0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF] * 2)
    csum = 2 * sum(15 - d for d in range(16))
    assert csum == 240
    assert M.wots_digits(F128, m1) == list(range(16)) * 2 + [0x0, 0xF, 0x0]


@pytest.mark.parametrize("name", [F128, "toy"])
def test_sign_then_verify_hedged_and_deterministic(name):
    n = M.PARAMS[name].n
    rng = random.Random(31)
    sk, pk = M.keygen_internal(name, rng.randbytes(n), rng.randbytes(n), rng.randbytes(n))
    msg = b"sign, then verify"
    det = M.sign_internal(name, msg, sk)
    assert det == M.sign_internal(name, msg, sk) and len(det) == M.sizes(name)["sig"]
    hedged = M.sign_internal(name, msg, sk, rng.randbytes(n))
    assert hedged != det
    assert M.verify_internal(name, msg, det, pk) and M.verify_internal(name, msg, hedged, pk)
    assert not M.verify_internal(name, msg + b"!", det, pk)
    ctx = b"context"
    sig = M.sign(name, msg, ctx, sk)
    assert M.verify(name, msg, sig, ctx, pk) and not M.verify(name, msg, sig, b"", pk) and not M.verify(name, msg, sig, bytes(256), pk)
    with pytest.raises(ValueError):
        M.sign(name, msg, bytes(256), sk)


def test_every_leaf_of_the_toy_xmss_trees():
    s = M.PARAMS["toy"]
    rng = random.Random(32)
    sk_seed, pk_seed = rng.randbytes(s.n), rng.randbytes(s.n)
    for layer, tree in ((0, 0), (0, 3), (1, 0)):
        adrs = M.Adrs()
        adrs.set_layer(layer)
        adrs.set_tree(tree)
        root = M.xmss_node("toy", sk_seed, 0, s.hp, pk_seed, adrs.copy())
        for idx in range(1 << s.hp):
            m1 = rng.randbytes(s.n)
            sig = M.xmss_sign("toy", m1, sk_seed, idx, pk_seed, adrs.copy())
            assert M.xmss_pk_from_sig("toy", idx, sig, m1, pk_seed, adrs.copy()) == root, (layer, tree, idx)
            assert M.xmss_pk_from_sig("toy", idx ^ 1, sig, m1, pk_seed, adrs.copy()) != root


def test_every_leaf_of_the_toy_fors_trees():
    s = M.PARAMS["toy"]
    rng = random.Random(33)
    sk_seed, pk_seed = rng.randbytes(s.n), rng.randbytes(s.n)
    adrs = M.Adrs()
    adrs.set_tree(2)
    adrs.set_type_and_clear(M.FORS_TREE)
    adrs.set_keypair(1)
    roots = b"".join(M.fors_node("toy", sk_seed, i, s.a, pk_seed, adrs.copy()) for i in range(s.k))
    pk_adrs = adrs.copy()
    pk_adrs.set_type_and_clear(M.FORS_ROOTS)
    pk_adrs.set_keypair(1)
    pk_fors = M.T("toy", pk_seed, pk_adrs, roots)
    seen = set()
    for v in list(range(1 << s.a)) + [rng.randrange(1 << (s.a * s.k)) for _ in range(24)]:
        bits = v if v >= (1 << s.a) else sum(v << (s.a * t) for t in range(s.k))        # every tree at leaf v, then mixed
        md = M.to_byte(bits << (16 - s.a * s.k), 2)
        idx = M.base_2b(md, s.a, s.k)
        seen.update(enumerate(idx))
        sig = M.fors_sign("toy", md, sk_seed, pk_seed, adrs.copy())
        assert len(sig) == s.k * (1 + s.a) * s.n
        assert M.fors_pk_from_sig("toy", sig, md, pk_seed, adrs.copy()) == pk_fors, idx
    assert len(seen) == s.k << s.a                                         # every leaf of every tree


def test_a_flipped_bit_in_each_region_in_the_message_and_in_the_key_rejects():
    name = F128
    pk, msg, sig = K.signed(name)[0]
    assert M.verify_internal(name, msg, sig, pk)
    positions = K.region_positions(name)
    s = M.PARAMS[name]
    assert len(positions) == 1 + 2 * s.k + 2 * s.d
    for what, pos in positions:
        assert not M.verify_internal(name, msg, K.flip(sig, pos, pos % 8), pk), what
    assert not M.verify_internal(name, K.flip(msg, 0), sig, pk)
    assert not M.verify_internal(name, msg, sig, K.flip(pk, 1))            # PK.seed
    assert not M.verify_internal(name, msg, sig, K.flip(pk, s.n + 1))      # PK.root
    assert not M.verify_internal(name, msg, sig[:-1], pk)


def test_idx_tree_is_a_full_64_bit_value_at_256f():
    for name in M.NAMES:
        s = M.PARAMS[name]
        c1, c2, c3 = -(-s.k * s.a // 8), -(-(s.h - s.hp) // 8), -(-s.hp // 8)
        digest = bytes(c1) + bytes([0xFF] * c2) + bytes(c3)
        md, idx_tree, idx_leaf = M.split_digest(name, digest)
        assert (md, idx_tree, idx_leaf) == (bytes(c1), (1 << (s.h - s.hp)) - 1, 0), name
        md, idx_tree, idx_leaf = M.split_digest(name, bytes([0xFF] * s.m))
        assert idx_tree == (1 << (s.h - s.hp)) - 1 and idx_leaf == (1 << s.hp) - 1
    assert M.split_digest("SLH-DSA-SHAKE-256f", bytes(40) + bytes([0xFF] * 8) + bytes(1))[1] == 0xFFFFFFFFFFFFFFFF
    # the hypertree of 256f is walked with all 64 bits of idx_tree
    name = "SLH-DSA-SHAKE-256f"
    pk, msg, sig = K.signed(name)[0]
    assert M.verify_internal(name, msg, sig, pk)
