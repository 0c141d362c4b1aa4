"""The four R_q coefficient maps of include/psf_mi355x.h in Python integers: the big-integer definitions the device results are compared with.

compress   lossy_compression_fips203.rs:89-112   y = floor((x 2^d + floor(q/2)) / q) mod 2^d, x read mod q
decompress lossy_compression_fips203.rs:143-172  x = floor((y q + 2^(d-1)) / 2^d) mod q (least non-negative residue)
encode     common_encodings.rs:49-91             out = digit floor(q/base) mod q, digits of the value least significant first
decode     common_encodings.rs:125-151           digit = floor((base c + floor(q/(2 base))) / q) mod base, c read mod q; composed most significant first
"""


def compress(x, d, q):
    x = int(x) % q
    return ((x << d) + q // 2) // q % (1 << d)


def decompress(y, d, q):
    return (int(y) * q + (1 << (d - 1))) // (1 << d) % q


def encode(digit, base, q):
    return int(digit) * (q // base) % q


def decode(c, base, q):
    c = int(c) % q
    return (base * c + q // (2 * base)) // q % base


def digits_of(value, base):
    """base-`base` digits of a non-negative integer, least significant first (common_encodings.rs:71-77); 0 has none"""
    out = []
    while value > 0:
        value, r = divmod(value, base)
        out.append(r)
    return out


def encode_value(value, base, q, n):
    """encode_value_in_polynomialringzq: the n coefficients, or None where the reference returns an error"""
    if value < 0 or base < 2:
        return None
    ds = digits_of(value, base)
    if len(ds) > n:
        return None
    return [encode(v, base, q) for v in ds] + [0] * (n - len(ds))


def decode_value(coeffs, base, q):
    """decode_value_from_polynomialringzq"""
    out = 0
    for c in reversed(list(coeffs)):
        out = out * base + decode(c, base, q)
    return out
