"""Algorithm 7 (ML-DSA.Sign_internal) restated over the functions of tests/helpers/mldsa_model.py so that every attempt is visible: per instance the
signature, the number of attempts and, for each attempt, which of the four tests fired.  M.sign_internal leaves an attempt at the first pair of
tests that fires; here all four are evaluated in every attempt (the device does the same: no early exit over secret data), which changes no
signature.  tests/test_mldsa_sign_cpu.py asserts that the bytes equal M.sign_internal's."""
import functools

from tests.helpers import mldsa_model as M

FIRED_Z, FIRED_R0, FIRED_CT0, FIRED_HINT = 1, 2, 4, 8


@functools.lru_cache(maxsize=64)
def key_context(sk, name):
    """what the loop reads of a secret key: decoded once per key"""
    k, l = M.PARAMS[name][:2]
    rho, K, tr, s1, s2, t0 = M.sk_decode(sk, name)
    return {"K": K, "tr": tr, "A_hat": M.expand_a(rho, k, l), "s1_hat": [M.ntt(p) for p in s1], "s2_hat": [M.ntt(p) for p in s2],
            "t0_hat": [M.ntt(p) for p in t0]}


def attempt(ctx, mu, rho_pp, kappa, name):
    """one pass of the loop at counter kappa: (fired, signature or None)"""
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    y = M.expand_mask(rho_pp, kappa, l, g1)
    w = [M.ntt_inv(p) for p in M.mat_vec_hat(ctx["A_hat"], [M.ntt(p) for p in y])]
    w1 = [[M.high_bits(x, g2) for x in p] for p in w]
    ct = M.H(mu + M.w1_encode(w1, g2), cb)
    c_hat = M.ntt(M.sample_in_ball(ct, tau))
    z = [M.poly_add(a, M.ntt_inv(M.pointwise(c_hat, p))) for a, p in zip(y, ctx["s1_hat"])]
    wm = [M.poly_sub(a, M.ntt_inv(M.pointwise(c_hat, p))) for a, p in zip(w, ctx["s2_hat"])]
    ct0 = [M.ntt_inv(M.pointwise(c_hat, p)) for p in ctx["t0_hat"]]
    h = [[M.make_hint(-a, b + a, g2) for a, b in zip(p0, pw)] for p0, pw in zip(ct0, wm)]
    fired = 0
    if M.inf_norm(z) >= g1 - beta:
        fired |= FIRED_Z
    if max(abs(M.low_bits(x, g2)) for p in wm for x in p) >= g2 - beta:
        fired |= FIRED_R0
    if M.inf_norm(ct0) >= g2:
        fired |= FIRED_CT0
    if sum(sum(p) for p in h) > omega:
        fired |= FIRED_HINT
    return fired, (None if fired else M.sig_encode(ct, z, h, name))


def sign_trace(sk, name, m_prime=None, rnd=bytes(32), mu=None, max_attempts=None):
    """(signature, attempts, [fired of each attempt]); with max_attempts reached first: (None, 0, [fired ...])"""
    ctx = key_context(bytes(sk), name)
    l = M.PARAMS[name][1]
    if mu is None:
        mu = M.H(ctx["tr"] + bytes(m_prime), 64)
    rho_pp = M.H(ctx["K"] + bytes(rnd) + bytes(mu), 64)
    trace = []
    while max_attempts is None or len(trace) < max_attempts:
        fired, sig = attempt(ctx, bytes(mu), rho_pp, l * len(trace), name)
        trace.append(fired)
        if sig is not None:
            return sig, len(trace), trace
    return None, 0, trace


def sign_batch(name, sks, msgs, rnds=None, msg_is_mu=False):
    """per instance (signature, attempts, trace); `sks` one key (bytes) for all or a list"""
    one = isinstance(sks, (bytes, bytearray))
    out = []
    for i, m in enumerate(msgs):
        sk = sks if one else sks[i]
        rnd = bytes(32) if rnds is None else rnds[i]
        out.append(sign_trace(sk, name, mu=m, rnd=rnd) if msg_is_mu else sign_trace(sk, name, m_prime=m, rnd=rnd))
    return out
