"""ML-DSA (FIPS 204, August 2024) in pure Python over hashlib: the model the device code is compared with (tests/test_gpu_fips204.py,
tests/test_gpu_mldsa.py, tests/test_mldsa_core_cpu.py).  Every algorithm is written the way the standard writes it, one function per algorithm,
lists of Python ints for polynomials; nothing is tuned.  The zetas are computed from 1753.  tests/test_mldsa_model_cpu.py pins this file by what
the standard fixes (sizes, Appendix B's first zetas, the algebraic identities, round trips, sign-then-verify and bit flips)."""
import hashlib

Q, N, D, ZETA = 8380417, 256, 13, 1753
# name: (k, l, eta, tau, lambda / 4, gamma1, gamma2, beta, omega)
PARAMS = {
    "ML-DSA-44": (4, 4, 2, 39, 32, 1 << 17, (Q - 1) // 88, 78, 80),
    "ML-DSA-65": (6, 5, 4, 49, 48, 1 << 19, (Q - 1) // 32, 196, 55),
    "ML-DSA-87": (8, 7, 2, 60, 64, 1 << 19, (Q - 1) // 32, 120, 75),
}
HINT, NORM, HASH = 1, 2, 4                                                # the bits of `why` (psf_mi355x.h)


def brv8(x):
    return int(f"{x:08b}"[::-1], 2)


ZETAS = [pow(ZETA, brv8(k), Q) for k in range(256)]


def bitlen(x):
    return x.bit_length()


def sizes(name):
    k, l, eta, tau, cb, g1, g2, beta, omega = PARAMS[name]
    return {"pk": 32 + 32 * k * (bitlen(Q - 1) - D),
            "sk": 32 + 32 + 64 + 32 * ((k + l) * bitlen(2 * eta) + D * k),
            "sig": cb + l * 32 * (1 + bitlen(g1 - 1)) + omega + k}


def H(data, n):
    return hashlib.shake_256(bytes(data)).digest(n)


def G(data, n):
    return hashlib.shake_128(bytes(data)).digest(n)


def mod_pm(r, a):
    """r mod+- a: the representative in (-a/2, a/2]"""
    r %= a
    return r - a if r > a // 2 else r


# ---- Algorithms 41, 42 and the arithmetic ----------------------------------------------------------------------------------------------------------

def ntt(w):
    w = [x % Q for x in w]
    m, ln = 0, 128
    while ln >= 1:
        start = 0
        while start < N:
            m += 1
            z = ZETAS[m]
            for j in range(start, start + ln):
                t = z * w[j + ln] % Q
                w[j + ln] = (w[j] - t) % Q
                w[j] = (w[j] + t) % Q
            start += 2 * ln
        ln //= 2
    return w


def ntt_inv(w):
    w = [x % Q for x in w]
    m, ln = 256, 1
    while ln < N:
        start = 0
        while start < N:
            m -= 1
            z = -ZETAS[m]
            for j in range(start, start + ln):
                t = w[j]
                w[j] = (t + w[j + ln]) % Q
                w[j + ln] = (t - w[j + ln]) * z % Q
            start += 2 * ln
        ln *= 2
    f = pow(256, Q - 2, Q)                                                # 8347681
    return [x * f % Q for x in w]


def pointwise(a, b):
    return [x * y % Q for x, y in zip(a, b)]


def poly_add(a, b):
    return [(x + y) % Q for x, y in zip(a, b)]


def poly_sub(a, b):
    return [(x - y) % Q for x, y in zip(a, b)]


def schoolbook(a, b):
    """a b mod (X^256 + 1, q)"""
    out = [0] * N
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < N:
                    out[i + j] += x * y
                else:
                    out[i + j - N] -= x * y
    return [v % Q for v in out]


def mat_vec_hat(A_hat, v_hat):
    """rows of A_hat times the vector v_hat, all in the NTT domain"""
    out = []
    for row in A_hat:
        acc = [0] * N
        for a, v in zip(row, v_hat):
            acc = poly_add(acc, pointwise(a, v))
        out.append(acc)
    return out


# ---- Algorithms 16 to 19: bit packing -----------------------------------------------------------------------------------------------------------------

def _pack_fields(vals, bits):
    acc = 0
    for i, v in enumerate(vals):
        assert 0 <= v < (1 << bits), (v, bits)
        acc |= v << (bits * i)
    return acc.to_bytes(len(vals) * bits // 8, "little")


def _unpack_fields(data, bits, count=N):
    acc = int.from_bytes(data, "little")
    return [(acc >> (bits * i)) & ((1 << bits) - 1) for i in range(count)]


def simple_bit_pack(w, b):
    return _pack_fields(w, bitlen(b))


def simple_bit_unpack(v, b):
    return _unpack_fields(v, bitlen(b))


def bit_pack(w, a, b):
    return _pack_fields([b - x for x in w], bitlen(a + b))


def bit_unpack(v, a, b):
    return [b - z for z in _unpack_fields(v, bitlen(a + b))]


def hint_bit_pack(h, omega):
    k = len(h)
    y = bytearray(omega + k)
    index = 0
    for i in range(k):
        for j in range(N):
            if h[i][j]:
                y[index] = j
                index += 1
        y[omega + i] = index
    return bytes(y)


def hint_bit_unpack(y, k, omega):
    """Algorithm 21; None stands for the standard's bottom"""
    h = [[0] * N for _ in range(k)]
    index = 0
    for i in range(k):
        if y[omega + i] < index or y[omega + i] > omega:
            return None
        first = index
        while index < y[omega + i]:
            if index > first and y[index - 1] >= y[index]:
                return None
            h[i][y[index]] = 1
            index += 1
    for i in range(index, omega):
        if y[i] != 0:
            return None
    return h


# ---- Algorithms 29 to 34: the samplers ----------------------------------------------------------------------------------------------------------------

def sample_in_ball(rho, tau, stats=None):
    c = [0] * N
    need = 8 + 4 * 136                                                   # squeezed lazily below; SHAKE output is a prefix-stable stream
    stream = H(rho, need)
    h = int.from_bytes(stream[:8], "little")
    pos = 8
    for i in range(256 - tau, 256):
        while True:
            if pos >= len(stream):
                need += 136
                stream = H(rho, need)
            j = stream[pos]
            pos += 1
            if j <= i:
                break
        c[i] = c[j]
        c[j] = -1 if (h >> (i + tau - 256)) & 1 else 1
    if stats is not None:
        stats["bytes"] = pos
        stats["blocks"] = (pos + 135) // 136
    return c


def rej_ntt_poly(seed, stats=None):
    """Algorithm 30 from the 34-byte seed; stats: the blocks of 168 bytes read and, per block, how many candidates were rejected"""
    out, blocks, rejected = [], 0, []
    while len(out) < N:
        blocks += 1
        block = G(seed, 168 * blocks)[168 * (blocks - 1):]
        rejected.append(0)
        for t in range(0, 168, 3):
            if len(out) == N:
                break
            z = block[t] | (block[t + 1] << 8) | ((block[t + 2] & 127) << 16)
            if z < Q:
                out.append(z)
            else:
                rejected[-1] += 1
    if stats is not None:
        stats["blocks"], stats["rejected"] = blocks, rejected
    return out


def coeff_from_half_byte(b, eta):
    if eta == 2 and b < 15:
        return 2 - (b % 5)
    if eta == 4 and b < 9:
        return 4 - b
    return None


def rej_bounded_poly(seed, eta, stats=None):
    """Algorithm 31 from the 66-byte seed; stats as in rej_ntt_poly with blocks of 136 bytes"""
    out, blocks, rejected = [], 0, []
    while len(out) < N:
        blocks += 1
        block = H(seed, 136 * blocks)[136 * (blocks - 1):]
        rejected.append(0)
        for z in block:
            for half in (z & 15, z >> 4):
                if len(out) == N:
                    break
                v = coeff_from_half_byte(half, eta)
                if v is None:
                    rejected[-1] += 1
                else:
                    out.append(v)
    if stats is not None:
        stats["blocks"], stats["rejected"] = blocks, rejected
    return out


def expand_a(rho, k, l):
    return [[rej_ntt_poly(rho + bytes([s, r])) for s in range(l)] for r in range(k)]


def expand_s(rho_p, k, l, eta):
    s1 = [rej_bounded_poly(rho_p + r.to_bytes(2, "little"), eta) for r in range(l)]
    s2 = [rej_bounded_poly(rho_p + (r + l).to_bytes(2, "little"), eta) for r in range(k)]
    return s1, s2


def expand_mask(rho, mu, l, g1):
    c = 1 + bitlen(g1 - 1)
    return [bit_unpack(H(rho + (mu + r).to_bytes(2, "little"), 32 * c), g1 - 1, g1) for r in range(l)]


# ---- Algorithms 35 to 40: rounding and hints --------------------------------------------------------------------------------------------------------------

def power2round(r):
    rp = r % Q
    r0 = mod_pm(rp, 1 << D)
    return (rp - r0) >> D, r0


def decompose(r, g2):
    rp = r % Q
    r0 = mod_pm(rp, 2 * g2)
    if rp - r0 == Q - 1:
        return 0, r0 - 1
    return (rp - r0) // (2 * g2), r0


def high_bits(r, g2):
    return decompose(r, g2)[0]


def low_bits(r, g2):
    return decompose(r, g2)[1]


def make_hint(z, r, g2):
    return int(high_bits(r, g2) != high_bits(r + z, g2))


def use_hint(h, r, g2):
    m = (Q - 1) // (2 * g2)
    r1, r0 = decompose(r, g2)
    if h == 1 and r0 > 0:
        return (r1 + 1) % m
    if h == 1 and r0 <= 0:
        return (r1 - 1) % m
    return r1


def w1_encode(w1, g2):
    return b"".join(simple_bit_pack(w, (Q - 1) // (2 * g2) - 1) for w in w1)


def inf_norm(vec):
    return max(abs(mod_pm(x, Q)) for p in vec for x in p)


# ---- Algorithms 22 to 28: encodings -------------------------------------------------------------------------------------------------------------------------

def pk_encode(rho, t1):
    return rho + b"".join(simple_bit_pack(p, (1 << (bitlen(Q - 1) - D)) - 1) for p in t1)


def pk_decode(pk, k):
    return pk[:32], [simple_bit_unpack(pk[32 + 320 * i:32 + 320 * (i + 1)], 1023) for i in range(k)]


def sk_encode(rho, K, tr, s1, s2, t0, eta):
    return (rho + K + tr + b"".join(bit_pack(p, eta, eta) for p in s1) + b"".join(bit_pack(p, eta, eta) for p in s2)
            + b"".join(bit_pack(p, (1 << (D - 1)) - 1, 1 << (D - 1)) for p in t0))


def sk_decode(sk, name):
    k, l, eta = PARAMS[name][:3]
    eb = 32 * bitlen(2 * eta)
    rho, K, tr = sk[:32], sk[32:64], sk[64:128]
    at = 128
    s1 = [bit_unpack(sk[at + eb * i:at + eb * (i + 1)], eta, eta) for i in range(l)]
    at += eb * l
    s2 = [bit_unpack(sk[at + eb * i:at + eb * (i + 1)], eta, eta) for i in range(k)]
    at += eb * k
    t0 = [bit_unpack(sk[at + 416 * i:at + 416 * (i + 1)], (1 << (D - 1)) - 1, 1 << (D - 1)) for i in range(k)]
    return rho, K, tr, s1, s2, t0


def sig_encode(ct, z, h, name):
    g1, omega = PARAMS[name][5], PARAMS[name][8]
    return ct + b"".join(bit_pack([mod_pm(x, Q) for x in p], g1 - 1, g1) for p in z) + hint_bit_pack(h, omega)


def sig_decode(sig, name):
    k, l, eta, tau, cb, g1, g2, beta, omega = PARAMS[name]
    zb = 32 * (1 + bitlen(g1 - 1))
    ct = sig[:cb]
    z = [bit_unpack(sig[cb + zb * i:cb + zb * (i + 1)], g1 - 1, g1) for i in range(l)]
    return ct, z, hint_bit_unpack(sig[cb + zb * l:], k, omega)


# ---- Algorithms 6, 7 and 8 ------------------------------------------------------------------------------------------------------------------------------------

def keygen_internal(xi, name, parts=None):
    k, l, eta = PARAMS[name][:3]
    seed = H(xi + bytes([k, l]), 128)
    rho, rho_p, K = seed[:32], seed[32:96], seed[96:]
    A_hat = expand_a(rho, k, l)
    s1, s2 = expand_s(rho_p, k, l, eta)
    t = [poly_add(ntt_inv(p), e) for p, e in zip(mat_vec_hat(A_hat, [ntt(p) for p in s1]), s2)]
    t1, t0 = [], []
    for p in t:
        pairs = [power2round(x) for x in p]
        t1.append([a for a, _ in pairs])
        t0.append([b for _, b in pairs])
    pk = pk_encode(rho, t1)
    tr = H(pk, 64)
    if parts is not None:
        parts.update(rho=rho, rho_p=rho_p, K=K, tr=tr, s1=s1, s2=s2, t=t, t1=t1, t0=t0)
    return pk, sk_encode(rho, K, tr, s1, s2, t0, eta)


def sign_internal(sk, m_prime, rnd, name, mu=None):
    k, l, eta, tau, cb, g1, g2, beta, omega = PARAMS[name]
    rho, K, tr, s1, s2, t0 = sk_decode(sk, name)
    s1_hat, s2_hat, t0_hat = [ntt(p) for p in s1], [ntt(p) for p in s2], [ntt(p) for p in t0]
    A_hat = expand_a(rho, k, l)
    if mu is None:
        mu = H(tr + m_prime, 64)
    rho_pp = H(K + rnd + mu, 64)
    kappa = 0
    while True:
        y = expand_mask(rho_pp, kappa, l, g1)
        kappa += l
        w = [ntt_inv(p) for p in mat_vec_hat(A_hat, [ntt(p) for p in y])]
        w1 = [[high_bits(x, g2) for x in p] for p in w]
        ct = H(mu + w1_encode(w1, g2), cb)
        c_hat = ntt(sample_in_ball(ct, tau))
        cs1 = [ntt_inv(pointwise(c_hat, p)) for p in s1_hat]
        cs2 = [ntt_inv(pointwise(c_hat, p)) for p in s2_hat]
        z = [poly_add(a, b) for a, b in zip(y, cs1)]
        wm = [poly_sub(a, b) for a, b in zip(w, cs2)]
        r0 = [[low_bits(x, g2) for x in p] for p in wm]
        if inf_norm(z) >= g1 - beta or max(abs(x) for p in r0 for x in p) >= g2 - beta:
            continue
        ct0 = [ntt_inv(pointwise(c_hat, p)) for p in t0_hat]
        h = [[make_hint(-a, b + a, g2) for a, b in zip(p0, pw)] for p0, pw in zip(ct0, wm)]
        if inf_norm(ct0) >= g2 or sum(sum(p) for p in h) > omega:
            continue
        return sig_encode(ct, z, h, name)


def verify_why(pk, m_prime, sig, name, mu=None):
    """Algorithm 8 with the reason: an OR of HINT, NORM and HASH as the library's `why` byte defines them (0: the signature verifies)"""
    k, l, eta, tau, cb, g1, g2, beta, omega = PARAMS[name]
    rho, t1 = pk_decode(pk, k)
    ct, z, h = sig_decode(sig, name)
    why = NORM if inf_norm(z) >= g1 - beta else 0
    if h is None:
        return why | HINT | HASH
    A_hat = expand_a(rho, k, l)
    if mu is None:
        mu = H(H(pk, 64) + m_prime, 64)
    c_hat = ntt(sample_in_ball(ct, tau))
    az = mat_vec_hat(A_hat, [ntt(p) for p in z])
    w = [ntt_inv(poly_sub(a, pointwise(c_hat, ntt([x << D for x in p])))) for a, p in zip(az, t1)]
    w1 = [[use_hint(hb, x, g2) for hb, x in zip(hp, p)] for hp, p in zip(h, w)]
    if H(mu + w1_encode(w1, g2), cb) != ct:
        why |= HASH
    return why


def verify_internal(pk, m_prime, sig, name, mu=None):
    return verify_why(pk, m_prime, sig, name, mu) == 0


# ---- Algorithms 2 and 3: the external forms (rnd given) ---------------------------------------------------------------------------------------------------

def format_message(M, ctx=b""):
    assert len(ctx) <= 255
    return bytes([0, len(ctx)]) + ctx + M


def sign(sk, M, ctx, rnd, name):
    return sign_internal(sk, format_message(M, ctx), rnd, name)


def verify(pk, M, sig, ctx, name):
    if len(ctx) > 255:
        return False
    return verify_internal(pk, format_message(M, ctx), sig, name)
