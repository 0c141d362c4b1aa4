"""Signing instances (xi, mu, rnd) with a stated property, shared by tests/test_mldsa_sign_cpu.py and tests/test_gpu_mldsa_sign.py.  They were found
by a search over instance(name, i) with the restated signer (tests/helpers/mldsa_sign_model.py); check() asserts that each still has its property.

Per parameter set: an instance accepted at its first attempt; one that needs at least 16 attempts; and instances with an attempt in which exactly one
of the tests fires: ||z|| alone, ||LowBits(r)|| alone, the hint count alone (the last fired alone in 11 / 1 / 2 of 4530 / 3627 / 2412 attempts).

What these keys cannot show: ||c t0||_inf >= gamma2 fired in none of 10569 attempts of the model under keys that KeyGen made.  It does fire under a
well-formed ML-DSA-44 key whose t0 sits at the ends of its 13-bit fields: that instance is searched and checked in
tests/helpers/mldsa_edge_cases.py (ct0_instance) and signed on the device by tests/test_gpu_mldsa_edges.py; for ML-DSA-65 and -87 no encodable t0
reaches gamma2.  Crafted residues on both sides of gamma2 go through tests/cpp/mldsa_sign_host_check.cpp as well."""
import functools
import hashlib

from tests.helpers import mldsa_model as M
from tests.helpers import mldsa_sign_model as S


def seed(tag, i, n):
    return hashlib.shake_256(b"psf-mldsa-" + tag + i.to_bytes(4, "little")).digest(n)


def instance(name, i):
    """(xi, mu, rnd) number i of a parameter set; 256 consecutive instances share a key"""
    t = name.encode()
    return seed(b"sign-xi" + t, i // 256, 32), seed(b"sign-mu" + t, i, 64), seed(b"sign-rnd" + t, i, 32)


@functools.lru_cache(maxsize=None)
def sk_of(name, xi):
    return M.keygen_internal(xi, name)[1]


# name: {property: i}
CASES = {
    "ML-DSA-44": {"first": 1, "long": 2, "z_alone": 2, "r0_alone": 2, "hint_alone": 31},
    "ML-DSA-65": {"first": 0, "long": 2, "z_alone": 2, "r0_alone": 2, "hint_alone": 396},
    "ML-DSA-87": {"first": 3, "long": 47, "z_alone": 0, "r0_alone": 0, "hint_alone": 25},
}
LONG = 16


def case_instances(name):
    """the distinct case instances of a set as [(sk, mu, rnd)]"""
    out = []
    for i in sorted(set(CASES[name].values())):
        xi, mu, rnd = instance(name, i)
        out.append((sk_of(name, xi), mu, rnd))
    return out


@functools.lru_cache(maxsize=None)
def trace(name, i):
    xi, mu, rnd = instance(name, i)
    return S.sign_trace(sk_of(name, xi), name, mu=mu, rnd=rnd)


def check():
    for name, cases in CASES.items():
        assert trace(name, cases["first"])[1] == 1, name
        assert trace(name, cases["long"])[1] >= LONG, name
        for prop, bit in (("z_alone", S.FIRED_Z), ("r0_alone", S.FIRED_R0), ("hint_alone", S.FIRED_HINT)):
            assert bit in trace(name, cases[prop])[2], (name, prop)
