"""FIPS 203 in pure Python over hashlib: the independent anchor of the byte-exact device functions (tools_amd/fips203.py).

G, H, J, PRF and the XOF (section 4.1), Algorithms 5 to 11 (ByteEncode / ByteDecode, SampleNTT, SamplePolyCBD, NTT, NTT^-1, MultiplyNTTs) and
K-PKE.KeyGen / Encrypt / Decrypt (Algorithms 13 to 15).  Polynomials are lists of 256 Python integers in [0, q); NTT-domain polynomials are in
FIPS 203's own representation (the order Algorithm 9 leaves them in).  Nothing here knows the library."""
import hashlib

Q = 3329
N = 256

# (k, eta1, eta2, du, dv)
PARAMS = {"ML-KEM-512": (2, 3, 2, 10, 4), "ML-KEM-768": (3, 2, 2, 10, 4), "ML-KEM-1024": (4, 2, 2, 11, 5)}


def bitrev7(i):
    return int(format(i, "07b")[::-1], 2)


ZETAS = [pow(17, bitrev7(i), Q) for i in range(128)]                 # Appendix A, first table
GAMMAS = [pow(17, 2 * bitrev7(i) + 1, Q) for i in range(128)]       # Appendix A, second table


# ---- section 4.1 ---------------------------------------------------------------------------------------------------------------------------------
def G(c):
    h = hashlib.sha3_512(bytes(c)).digest()
    return h[:32], h[32:]


def H(s):
    return hashlib.sha3_256(bytes(s)).digest()


def J(s):
    return hashlib.shake_256(bytes(s)).digest(32)


def PRF(eta, s, b):
    assert len(s) == 32 and 0 <= b < 256
    return hashlib.shake_256(bytes(s) + bytes([b])).digest(64 * eta)


# ---- Algorithms 5, 6 -----------------------------------------------------------------------------------------------------------------------------
def byte_encode(F, d):
    total = 0
    for i, v in enumerate(F):
        assert 0 <= v < (1 << d)
        total |= v << (i * d)
    return total.to_bytes(len(F) * d // 8, "little")


def byte_decode(B, d, count=N):
    total = int.from_bytes(bytes(B), "little")
    m = Q if d == 12 else 1 << d
    return [((total >> (i * d)) & ((1 << d) - 1)) % m for i in range(count)]


def compress(x, d):
    return ((x << d) + Q // 2) // Q % (1 << d)


def decompress(y, d):
    return (y * Q + (1 << (d - 1))) >> d


# ---- Algorithm 7 ---------------------------------------------------------------------------------------------------------------------------------
def sample_ntt_blocks(B, max_blocks=None):
    """(coefficients, SHAKE128 blocks consumed, failed).  max_blocks = None: the standard's unbounded loop; otherwise a polynomial that is still
    short after that many 168-byte blocks gets zeros for the rest (the library's cap)."""
    assert len(B) == 34
    a, pos, size = [], 0, 168 * 8
    stream = hashlib.shake_128(bytes(B)).digest(size)
    while len(a) < N:
        if max_blocks is not None and pos >= 168 * max_blocks:
            return a + [0] * (N - len(a)), max_blocks, True
        if pos + 3 > len(stream):
            size *= 2
            stream = hashlib.shake_128(bytes(B)).digest(size)
        c0, c1, c2 = stream[pos], stream[pos + 1], stream[pos + 2]
        pos += 3
        d1 = c0 + 256 * (c1 % 16)
        d2 = c1 // 16 + 16 * c2
        if d1 < Q:
            a.append(d1)
        if d2 < Q and len(a) < N:
            a.append(d2)
    return a, (pos + 167) // 168, False


def sample_ntt(B):
    return sample_ntt_blocks(B)[0]


# ---- Algorithm 8 ---------------------------------------------------------------------------------------------------------------------------------
def sample_poly_cbd(eta, B):
    """signed coefficients in [-eta, eta]"""
    assert len(B) == 64 * eta
    bits = int.from_bytes(bytes(B), "little")
    out = []
    for i in range(N):
        x = sum((bits >> (2 * i * eta + j)) & 1 for j in range(eta))
        y = sum((bits >> (2 * i * eta + eta + j)) & 1 for j in range(eta))
        out.append(x - y)
    return out


# ---- Algorithms 9, 10, 11 --------------------------------------------------------------------------------------------------------------------------
def ntt(f):
    f = [v % Q for v in f]
    i, length = 1, 128
    while length >= 2:
        for start in range(0, N, 2 * length):
            z = ZETAS[i]
            i += 1
            for j in range(start, start + length):
                t = z * f[j + length] % Q
                f[j + length] = (f[j] - t) % Q
                f[j] = (f[j] + t) % Q
        length //= 2
    return f


def ntt_inv(fh):
    f = [v % Q for v in fh]
    i, length = 127, 2
    while length <= 128:
        for start in range(0, N, 2 * length):
            z = ZETAS[i]
            i -= 1
            for j in range(start, start + length):
                t = f[j]
                f[j] = (t + f[j + length]) % Q
                f[j + length] = z * (f[j + length] - t) % Q
        length *= 2
    return [v * 3303 % Q for v in f]


def multiply_ntts(fh, gh):
    h = [0] * N
    for i in range(128):
        a0, a1, b0, b1, g = fh[2 * i], fh[2 * i + 1], gh[2 * i], gh[2 * i + 1], GAMMAS[i]
        h[2 * i] = (a0 * b0 + a1 * b1 % Q * g) % Q
        h[2 * i + 1] = (a0 * b1 + a1 * b0) % Q
    return h


def schoolbook(a, b):
    """a b in Z_q[X] / (X^256 + 1), coefficients of either sign"""
    out = [0] * N
    for i, x in enumerate(a):
        if x == 0:
            continue
        for j, y in enumerate(b):
            if i + j < N:
                out[i + j] += x * y
            else:
                out[i + j - N] -= x * y
    return [v % Q for v in out]


def poly_add(a, b):
    return [(x + y) % Q for x, y in zip(a, b)]


def poly_sub(a, b):
    return [(x - y) % Q for x, y in zip(a, b)]


# ---- Algorithms 13, 14, 15 ---------------------------------------------------------------------------------------------------------------------------
def sample_matrix(rho, k):
    """A_hat[i][j] = SampleNTT(rho || j || i)"""
    return [[sample_ntt(bytes(rho) + bytes([j, i])) for j in range(k)] for i in range(k)]


def kpke_keygen(d, name):
    k, eta1, _, _, _ = PARAMS[name]
    rho, sigma = G(bytes(d) + bytes([k]))
    A = sample_matrix(rho, k)
    s = [sample_poly_cbd(eta1, PRF(eta1, sigma, n)) for n in range(k)]
    e = [sample_poly_cbd(eta1, PRF(eta1, sigma, k + n)) for n in range(k)]
    sh = [ntt(p) for p in s]
    eh = [ntt(p) for p in e]
    th = []
    for i in range(k):
        acc = eh[i]
        for j in range(k):
            acc = poly_add(acc, multiply_ntts(A[i][j], sh[j]))
        th.append(acc)
    ek = b"".join(byte_encode(p, 12) for p in th) + rho
    dk = b"".join(byte_encode(p, 12) for p in sh)
    return ek, dk


def kpke_encrypt(ek, m, r, name):
    k, eta1, eta2, du, dv = PARAMS[name]
    th = [byte_decode(ek[384 * i:384 * (i + 1)], 12) for i in range(k)]
    rho = ek[384 * k:]
    A = sample_matrix(rho, k)
    y = [sample_poly_cbd(eta1, PRF(eta1, r, n)) for n in range(k)]
    e1 = [sample_poly_cbd(eta2, PRF(eta2, r, k + n)) for n in range(k)]
    e2 = sample_poly_cbd(eta2, PRF(eta2, r, 2 * k))
    yh = [ntt(p) for p in y]
    u = []
    for i in range(k):
        acc = [0] * N
        for j in range(k):
            acc = poly_add(acc, multiply_ntts(A[j][i], yh[j]))      # A^T
        u.append(poly_add(ntt_inv(acc), e1[i]))
    mu = [decompress(b, 1) for b in byte_decode(m, 1)]
    acc = [0] * N
    for j in range(k):
        acc = poly_add(acc, multiply_ntts(th[j], yh[j]))
    v = poly_add(poly_add(ntt_inv(acc), e2), mu)
    c1 = b"".join(byte_encode([compress(x, du) for x in p], du) for p in u)
    c2 = byte_encode([compress(x, dv) for x in v], dv)
    return c1 + c2


def kpke_decrypt(dk, c, name):
    k, _, _, du, dv = PARAMS[name]
    u = [[decompress(y, du) for y in byte_decode(c[32 * du * i:32 * du * (i + 1)], du)] for i in range(k)]
    v = [decompress(y, dv) for y in byte_decode(c[32 * du * k:], dv)]
    sh = [byte_decode(dk[384 * i:384 * (i + 1)], 12) for i in range(k)]
    acc = [0] * N
    for j in range(k):
        acc = poly_add(acc, multiply_ntts(sh[j], ntt(u[j])))
    w = poly_sub(v, ntt_inv(acc))
    return byte_encode([compress(x, 1) for x in w], 1)
