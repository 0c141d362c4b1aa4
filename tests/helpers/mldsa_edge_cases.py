"""Case tables of the ML-DSA edge tests (tests/test_gpu_mldsa_edges.py), pinned to the model by tests/test_mldsa_edge_cases_cpu.py.

every_sig_byte(name)     an honest (pk, M', sigma) and, for every byte b of sigma, sigma with bit b mod 8 of that byte flipped.  The expected `why`
                         comes from a rule (`flipped`) that needs no verification: a byte of c~ gives HASH; a byte of z gives HASH, plus NORM iff the
                         coefficient that holds the bit now has |value| >= gamma1 - beta; a hint byte gives HINT | HASH iff HintBitUnpack rejects the
                         new bytes, else HASH.  (A changed z changes A z everywhere, and UseHint with h = 1 always changes w1: the hash never
                         survives.)  The CPU test proves the rule against M.verify_why at `proof_positions`.
every_z_position(name)   the norm bound at the positions k_unpack's threads see: for ML-DSA-44 every coefficient of z in turn at +-(gamma1 - beta),
                         for -65 and -87 the first and last coefficient of every group of 8 of the first and the last polynomial; and per group
                         one coefficient at +-(gamma1 - beta - 1), which is inside the bound.
extreme(name)            signatures of all 0x00 / all 0xFF, honest signatures whose z is all-zero / all-one fields (z = gamma1 / -(gamma1 - 1)
                         everywhere), and a key whose t1 is all 0xFF (t1 = 1023, t1 2^d = q - 1) under an honest signature; `why` from M.verify_why.
odd_sk(name)             secret keys with eta-fields that KeyGen never writes: 7 (eta = 2) and 15 (eta = 4), which skDecode reads as -5 and -11.
                         Three keys: the first 8 fields of s1[0], the last 8 fields of s2[k - 1], every field of s1 and s2.  Six mu each, rnd = 0.
ct0_*                    an ML-DSA-44 signing instance in which ||c t0||_inf >= gamma2 fires, once alone and once with other tests.  t0 is 13-bit
                         fields that cover -4095 ... 4096; a key whose t0 sits at those extremes is a well-formed sk, Sign_internal is defined on
                         it, and ||c t0||_inf can reach tau 4096.  For ML-DSA-65 and -87 that is 200 704 and 245 760, below gamma2 = 261 888: the
                         test cannot fire there for any encodable t0, so the searched case is ML-DSA-44 only (tau 4096 = 159 744 >= 95 232).
                         The key: KeyGen_internal(bytes(range(32))) with rows 0 and 1 of t0 replaced by 4096 / -4095 at the bits of
                         random.Random(5); mu = SHAKE256(b"x" || i, 64), rnd = 0.  Of i < 256, instance 135 has an attempt in which the test
                         fires alone and one in which it fires with others, and signs at its 16th attempt."""
import functools
import hashlib
import random

from tests.helpers import mldsa_model as M
from tests.helpers import mldsa_sign_model as S
from tests.helpers.mldsa_gpu import flip, keys, layout, triples, with_z_coefficient

HINT, NORM, HASH = M.HINT, M.NORM, M.HASH
MSG_LEN = 136
MAX_ATTEMPTS = 64


def honest(name):
    """(pk, M', sigma) of the model"""
    return triples(name, MSG_LEN)[0]


def z_field(name, sig, poly, index):
    """coefficient `index` of polynomial `poly` of z, read from the four bytes that hold its field"""
    g1, lay = M.PARAMS[name][5], layout(name)
    bits = lay["zb"] // 32
    at = lay["z"] + lay["zb"] * poly + bits * index // 8
    return g1 - ((int.from_bytes(sig[at:at + 4], "little") >> (bits * index % 8)) & ((1 << bits) - 1))


def flipped(name, sig, pos, bit):
    """(sigma with that bit flipped, the `why` the rule expects of it) for an honest sigma"""
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    lay = layout(name)
    new = flip(sig, pos, bit)
    if pos < cb:
        return new, HASH
    if pos < lay["hint"]:
        poly, rel = divmod(pos - lay["z"], lay["zb"])
        v = z_field(name, new, poly, (8 * rel + bit) // (lay["zb"] // 32))
        return new, HASH | (NORM if abs(v) >= g1 - beta else 0)
    return new, HASH | (HINT if M.hint_bit_unpack(new[lay["hint"]:], k, omega) is None else 0)


@functools.lru_cache(maxsize=None)
def every_sig_byte(name):
    """(pk, M', [sigma, sigma with byte 0 changed, byte 1, ...], [why of each])"""
    pk, msg, sig = honest(name)
    pairs = [flipped(name, sig, b, b % 8) for b in range(len(sig))]
    return pk, msg, [sig] + [p[0] for p in pairs], [0] + [p[1] for p in pairs]


def proof_positions(name):
    """the bytes at which the CPU test runs the model: every byte of c~, every hint byte, the first and last byte of every polynomial of z, every 16th z byte"""
    l, lay, size = M.PARAMS[name][1], layout(name), M.sizes(name)["sig"]
    pos = set(range(lay["z"])) | set(range(lay["hint"], size)) | set(range(lay["z"], lay["hint"], 16))
    for p in range(l):
        pos |= {lay["z"] + lay["zb"] * p, lay["z"] + lay["zb"] * (p + 1) - 1}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def every_z_position(name):
    """(pk, M', [sigma ...], [why ...], [(poly, index, value) ...])"""
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    pk, msg, sig = honest(name)
    where = []
    for poly in (range(l) if name == "ML-DSA-44" else (0, l - 1)):
        for group in range(32):
            at = range(8 * group, 8 * group + 8) if name == "ML-DSA-44" else (8 * group, 8 * group + 7)
            where += [(poly, i, (g1 - beta) * (-1) ** (i + poly)) for i in at]
            where.append((poly, 8 * group + (group + poly) % 8, (g1 - beta - 1) * (-1) ** group))
    sigs = [with_z_coefficient(name, sig, p, i, v) for p, i, v in where]
    want = [(HASH if s != sig else 0) | (NORM if abs(v) >= g1 - beta else 0) for s, (p, i, v) in zip(sigs, where)]
    return pk, msg, sigs, want, where


@functools.lru_cache(maxsize=None)
def extreme(name):
    """([(pk, M', sigma) ...], [why ...]): all 0x00, all 0xFF, z of all-zero fields, z of all-one fields, t1 of all 0xFF"""
    pk, msg, sig = honest(name)
    lay, n = layout(name), len(sig)
    inst = [(pk, msg, bytes(n)), (pk, msg, b"\xff" * n),
            (pk, msg, sig[:lay["z"]] + bytes(lay["hint"] - lay["z"]) + sig[lay["hint"]:]),
            (pk, msg, sig[:lay["z"]] + b"\xff" * (lay["hint"] - lay["z"]) + sig[lay["hint"]:]),
            (pk[:32] + b"\xff" * (len(pk) - 32), msg, sig)]
    return inst, [M.verify_why(p, m, s, name) for p, m, s in inst]


def odd_keys(name):
    """the three keys of odd_sk"""
    k, l, eta = M.PARAMS[name][:3]
    eb = M.bitlen(2 * eta)                                                  # bits of a field = bytes of 8 fields
    sk = keys(name, 1)["sk"][0]
    end = 128 + 32 * eb * (l + k)
    return [sk[:128] + b"\xff" * eb + sk[128 + eb:], sk[:end - eb] + b"\xff" * eb + sk[end:], sk[:128] + b"\xff" * (end - 128) + sk[end:]]


def odd_sk(name):
    """[(sk, mu, rnd) ...]: key 0 with six mu, then key 1, then key 2"""
    return [(sk, hashlib.shake_256(b"psf-mldsa-odd-sk" + name.encode() + bytes([n, i])).digest(64), bytes(32)) for n, sk in enumerate(odd_keys(name)) for i in range(6)]


# ---- the c t0 case ------------------------------------------------------------------------------------------------------------------------------------
CT0_NAME, CT0_XI, CT0_ROWS, CT0_SEED, CT0_I = "ML-DSA-44", bytes(range(32)), (0, 1), 5, 135


@functools.lru_cache(maxsize=None)
def ct0_key():
    eta = M.PARAMS[CT0_NAME][2]
    rho, K, tr, s1, s2, t0 = M.sk_decode(M.keygen_internal(CT0_XI, CT0_NAME)[1], CT0_NAME)
    rng = random.Random(CT0_SEED)
    for r in CT0_ROWS:
        t0[r] = [4096 if rng.getrandbits(1) else -4095 for _ in range(256)]
    return M.sk_encode(rho, K, tr, s1, s2, t0, eta)


def ct0_instance(i=CT0_I):
    """(sk, mu, rnd) number i under the crafted key"""
    return ct0_key(), hashlib.shake_256(b"x" + bytes([i])).digest(64), bytes(32)


def ct0_instances():
    """the searched instance between its neighbours i - 1 and i + 1, which are ordinary instances of the same key"""
    return [ct0_instance(CT0_I - 1), ct0_instance(CT0_I), ct0_instance(CT0_I + 1)]


@functools.lru_cache(maxsize=None)
def ct0_trace(i=CT0_I):
    sk, mu, rnd = ct0_instance(i)
    return S.sign_trace(sk, CT0_NAME, mu=mu, rnd=rnd, max_attempts=MAX_ATTEMPTS)


def check():
    for name, (k, l, eta, tau, cb, g1, g2, beta, omega) in M.PARAMS.items():
        assert (tau * 4096 >= g2) == (name == CT0_NAME), name
    sig, attempts, fired = ct0_trace()
    assert S.FIRED_CT0 in fired, "no attempt in which ||c t0|| fires alone"
    assert any(f & S.FIRED_CT0 and f != S.FIRED_CT0 for f in fired), "no attempt in which ||c t0|| fires with another test"
    assert sig is not None and 1 <= attempts <= MAX_ATTEMPTS
    for i in (CT0_I - 1, CT0_I + 1):
        assert ct0_trace(i)[0] is not None, i
