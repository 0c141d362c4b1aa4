"""Pins the pure-Python model of SLH-DSA's SHA-2 parameter sets (tests/helpers/slhdsa_sha2_model.py) that the device and the C++ core are compared with:
the sizes of FIPS 205 Table 2, the compressed address against its byte definition, MGF1 against a restatement, sign -> verify and the identity
pkFromSig(sign(.)) = node for every leaf of a toy set on the n = 16 path (SHA-256 throughout) and of a toy set with n = 24 (H and T_l on SHA-512),
rejection of a flipped bit in every region, and the structural pin: the same Scheme code with section 11.1's SHAKE functions plugged in reproduces
tests/helpers/slhdsa_model.py's keys and signatures byte for byte, so what is new here is section 11.2's functions alone.  No other SLH-DSA
implementation exists on the hosts the suite runs on: these identities, and the independent restatement in C++ (tests/test_slhdsa_sha2_cpu.py), are
what stands behind "equal to the model"."""
import hashlib
import hmac
import random

import pytest

from tests.helpers import slhdsa_model as S
from tests.helpers import slhdsa_sha2_model as M

TABLE2 = {  # name: (n, h, d, h', a, k, m, pk bytes, sig bytes)
    "SLH-DSA-SHA2-128s": (16, 63, 7, 9, 12, 14, 30, 32, 7856),
    "SLH-DSA-SHA2-128f": (16, 66, 22, 3, 6, 33, 34, 32, 17088),
    "SLH-DSA-SHA2-192s": (24, 63, 7, 9, 14, 17, 39, 48, 16224),
    "SLH-DSA-SHA2-192f": (24, 66, 22, 3, 8, 33, 42, 48, 35664),
    "SLH-DSA-SHA2-256s": (32, 64, 8, 8, 14, 22, 47, 64, 29792),
    "SLH-DSA-SHA2-256f": (32, 68, 17, 4, 9, 35, 49, 64, 49856),
}


def test_sizes_of_table_2():
    assert sorted(TABLE2) == sorted(M.NAMES)
    for name, (n, h, d, hp, a, k, m, pk, sig) in TABLE2.items():
        assert tuple(M.PARAMS[name]) == (n, h, d, hp, a, k, m)
        assert h == d * hp
        assert M.sizes(name) == {"pk": pk, "sk": 2 * pk, "sig": sig}
        assert M.wots_len(name) == (2 * n, 3, 2 * n + 3)
        assert M.IDS[name] == list(TABLE2).index(name)
        assert tuple(M.PARAMS[name]) == tuple(S.PARAMS[name.replace("SHA2", "SHAKE")])      # the SHAKE sets' numbers


def test_the_compressed_address_against_its_byte_definition():
    a = M.Adrs()
    a.set_layer(0x01020304)
    a.set_tree(0x05060708090A0B0C0D0E0F10)
    a.set_type_and_clear(M.WOTS_HASH)
    a.b[16:20] = bytes([0x11, 0x12, 0x13, 0x14])                           # a type with all four bytes set: only the last survives
    a.set_keypair(0x15161718)
    a.set_chain(0x191A1B1C)
    a.set_hash(0x1D1E1F20)
    assert bytes(a.b) == bytes(range(1, 33))
    c = M.adrs_c(a)
    # layer: 1 byte (the least significant) || tree: the low 8 of 12 || type: 1 byte || the last 12 bytes unchanged
    assert c == bytes([4]) + bytes(range(9, 17)) + bytes([0x14]) + bytes(range(0x15, 0x21)) and len(c) == 22


def test_mgf1_against_a_restatement():
    def restated(h, seed, n):
        t = b""
        for c in range(-(-n // h().digest_size)):
            t += h(seed + c.to_bytes(4, "big")).digest()
        return t[:n]
    rng = random.Random(5)
    for h in (hashlib.sha256, hashlib.sha512):
        for seed_len in (0, 1, 64, 112, 128):
            for n in (1, 30, 32, 33, 34, 47, 49, 64, 65, 200):
                seed = rng.randbytes(seed_len)
                assert M.mgf1(h, seed, n) == restated(h, seed, n)
    assert M.mgf1(hashlib.sha256, b"", 34)[32:] == hashlib.sha256(bytes([0, 0, 0, 1])).digest()[:2]   # SHA2-128f: the second counter


def test_the_section_11_2_functions_against_their_formulas():
    rng = random.Random(6)
    for name in ("SLH-DSA-SHA2-128f", "SLH-DSA-SHA2-192f", "SLH-DSA-SHA2-256s"):
        s = M.PARAMS[name]
        f = M.Sha2(s)
        n = s.n
        seed, x, y, r, root, msg = (rng.randbytes(k) for k in (n, n, n, n, n, 50))
        a = M.Adrs(rng.randbytes(32))
        big, block = (hashlib.sha256, 64) if n == 16 else (hashlib.sha512, 128)
        assert f.F(seed, a, x) == f.prf(seed, x, a) == hashlib.sha256(seed + bytes(64 - n) + M.adrs_c(a) + x).digest()[:n]
        assert f.H(seed, a, x + y) == big(seed + bytes(block - n) + M.adrs_c(a) + x + y).digest()[:n]
        assert f.T(seed, a, x * 5) == big(seed + bytes(block - n) + M.adrs_c(a) + x * 5).digest()[:n]
        assert f.prf_msg(x, y, msg) == hmac.new(x, y + msg, big).digest()[:n]
        assert f.h_msg(r, seed, root, msg) == M.mgf1(big, r + seed + big(r + seed + root + msg).digest(), s.m) and len(f.h_msg(r, seed, root, msg)) == s.m


@pytest.mark.parametrize("toy", ["toy", "toy24"])
def test_sign_verify_and_pk_from_sig_over_every_leaf_of_a_toy_set(toy):
    """toy: n = 16, everything on SHA-256; toy24: n = 24, H and T_l on SHA-512 beside F and PRF on SHA-256"""
    s = M.PARAMS[toy]
    sch = M.Scheme(toy)
    n = s.n
    rng = random.Random(21 + n)
    sk_seed, sk_prf, pk_seed = rng.randbytes(n), rng.randbytes(n), rng.randbytes(n)
    sk, pk = sch.keygen_internal(sk_seed, sk_prf, pk_seed)
    assert sk == sk_seed + sk_prf + pk_seed + pk[n:] and pk[:n] == pk_seed
    # XMSS: every leaf of the top tree signs, and pkFromSig leads to the root
    for idx in range(1 << s.hp):
        adrs = M.Adrs()
        adrs.set_layer(s.d - 1)
        m1 = rng.randbytes(n)
        sig = sch.xmss_sign(m1, sk_seed, idx, pk_seed, adrs)
        adrs = M.Adrs()
        adrs.set_layer(s.d - 1)
        assert sch.xmss_pk_from_sig(idx, sig, m1, pk_seed, adrs) == pk[n:], (toy, idx)
    # FORS: every index of every tree; the public key from the signature is the one from the nodes
    for trial in range(1 << s.a):
        md = bytes([(trial * 73 + 5 * i) % 256 for i in range(-(-s.k * s.a // 8))])
        adrs = sch._fors_adrs(3, 1)
        sig = sch.fors_sign(md, sk_seed, pk_seed, adrs)
        roots = b"".join(sch.fors_node(sk_seed, i, s.a, pk_seed, sch._fors_adrs(3, 1)) for i in range(s.k))
        want = sch.f.T(pk_seed, sch._sub(sch._fors_adrs(3, 1), M.FORS_ROOTS), roots)
        assert sch.fors_pk_from_sig(sig, md, pk_seed, sch._fors_adrs(3, 1)) == want, (toy, trial)
    # whole signatures: many messages (every leaf of the hypertree is reached with high probability), hedged and deterministic
    seen = set()
    for t in range(48):
        msg = rng.randbytes(t)
        sig = sch.sign_internal(msg, sk, rng.randbytes(n) if t % 2 else None)
        assert len(sig) == M.sizes(toy)["sig"]
        assert sch.verify_internal(msg, sig, pk) and sch.root_from_sig(msg, sig, pk) == pk[n:]
        seen.add(M.split_digest(toy, sch.f.h_msg(sig[:n], pk[:n], pk[n:], msg))[1:])
        assert not sch.verify_internal(msg + b"x", sig, pk)
    assert len(seen) > (1 << s.h) // 2
    # one flipped bit per region
    msg = b"regions"
    sig = sch.sign_internal(msg, sk)
    reg = M.regions(toy)
    spots = [reg["R"][0]] + [a for a, _ in reg["fors_sk"]] + [a for a, _ in reg["fors_auth"]] + [a for a, _ in reg["wots"]] + [a for a, _ in reg["auth"]]
    for pos in spots:
        bad = bytearray(sig)
        bad[pos] ^= 0x10
        assert not sch.verify_internal(msg, bytes(bad), pk), (toy, pos)
    assert not sch.verify_internal(msg, sig, pk[:n] + bytes([pk[n] ^ 1]) + pk[n + 1:])
    assert not sch.verify_internal(msg, sig[:-1], pk)
    assert sch.verify(b"m", sch.sign(b"m", b"ctx", sk), b"ctx", pk) and not sch.verify(b"m", sch.sign(b"m", b"ctx", sk), b"cty", pk)
    with pytest.raises(ValueError):
        sch.sign(b"m", bytes(256), sk)


def test_with_the_shake_functions_the_scheme_is_the_pinned_model():
    """the structural pin: Scheme(set, Shake) = tests/helpers/slhdsa_model.py on its toy set (keys, hedged and deterministic signatures, verdicts) and
    on SLH-DSA-SHAKE-128f (a key and a signature)"""
    rng = random.Random(31)
    sch = M.Scheme(S.PARAMS["toy"], M.Shake)
    for t in range(6):
        a, b, c = rng.randbytes(16), rng.randbytes(16), rng.randbytes(16)
        sk, pk = sch.keygen_internal(a, b, c)
        assert (sk, pk) == S.keygen_internal("toy", a, b, c)
        msg, rnd = rng.randbytes(t * 7), (rng.randbytes(16) if t % 2 else None)
        sig = sch.sign_internal(msg, sk, rnd)
        assert sig == S.sign_internal("toy", msg, sk, rnd)
        assert sch.verify_internal(msg, sig, pk) and S.verify_internal("toy", msg, sig, pk)
        assert sch.sign(msg, b"c", sk) == S.sign("toy", msg, b"c", sk)
    name = "SLH-DSA-SHAKE-128f"
    big = M.Scheme(S.PARAMS[name], M.Shake)
    a, b, c = rng.randbytes(16), rng.randbytes(16), rng.randbytes(16)
    sk, pk = big.keygen_internal(a, b, c)
    assert (sk, pk) == S.keygen_internal(name, a, b, c)
    assert big.sign_internal(b"pin", sk) == S.sign_internal(name, b"pin", sk)
