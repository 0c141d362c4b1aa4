"""ML-KEM in pure Python over hashlib: ML-KEM.KeyGen_internal, Encaps_internal and Decaps_internal (FIPS 203 Algorithms 16 to 18) and the two
input checks of sections 7.2 and 7.3, on top of the K-PKE model of tests/helpers/fips203_kpke_model.py.  Written from the text of the standard;
nothing here knows the library.

No external known answers for ML-KEM are available to this suite (no ACVP vector file, and the system's OpenSSL predates ML-KEM), so this model,
hashlib and the algorithm text are the reference: the K-PKE layer below is itself checked against hashlib, schoolbook products and its own
inverse maps (tests/test_fips203_model_cpu.py), and tests/test_mlkem_model_cpu.py checks the properties the outer layer must have."""
from tests.helpers import fips203_kpke_model as M

Q = M.Q
PARAMS = M.PARAMS


def sizes(name):
    """{"ek", "dk", "ct", "ss"} in bytes"""
    k, _, _, du, dv = PARAMS[name]
    return {"ek": 384 * k + 32, "dk": 768 * k + 96, "ct": 32 * (du * k + dv), "ss": 32}


def keygen_internal(d, z, name):
    """Algorithm 16: (ek, dk) with dk = dk_pke || ek || H(ek) || z"""
    assert len(d) == 32 and len(z) == 32
    ek, dk_pke = M.kpke_keygen(d, name)
    return ek, dk_pke + ek + M.H(ek) + bytes(z)


def encaps_internal(ek, m, name):
    """Algorithm 17: (K, c) with (K, r) = G(m || H(ek)) and c = K-PKE.Encrypt(ek, m, r)"""
    assert len(m) == 32 and len(ek) == sizes(name)["ek"]
    K, r = M.G(bytes(m) + M.H(ek))
    return K, M.kpke_encrypt(ek, m, r, name)


def decaps_internal(dk, c, name):
    """Algorithm 18"""
    k = PARAMS[name][0]
    assert len(dk) == sizes(name)["dk"] and len(c) == sizes(name)["ct"]
    dk_pke = dk[0:384 * k]
    ek = dk[384 * k:768 * k + 32]
    h = dk[768 * k + 32:768 * k + 64]
    z = dk[768 * k + 64:768 * k + 96]
    m2 = M.kpke_decrypt(dk_pke, c, name)
    K2, r2 = M.G(m2 + h)
    K_bar = M.J(z + bytes(c))
    c2 = M.kpke_encrypt(ek, m2, r2, name)
    return K2 if c2 == bytes(c) else K_bar


def rejection_key(dk, c, name):
    """J(z || c): what decapsulation returns for a ciphertext that does not re-encrypt to itself"""
    k = PARAMS[name][0]
    return M.J(dk[768 * k + 64:768 * k + 96] + bytes(c))


def check_ek(ek, name):
    """section 7.2, the modulus check: ByteEncode_12(ByteDecode_12(ek[0 : 384 k])) = ek[0 : 384 k], i.e. every 12-bit field is below q"""
    k = PARAMS[name][0]
    body = bytes(ek[:384 * k])
    again = b"".join(M.byte_encode(M.byte_decode(body[384 * i:384 * (i + 1)], 12), 12) for i in range(k))
    return again == body


def check_dk(dk, name):
    """section 7.3, the hash check: H(dk[384 k : 768 k + 32]) = dk[768 k + 32 : 768 k + 64]"""
    k = PARAMS[name][0]
    return M.H(dk[384 * k:768 * k + 32]) == bytes(dk[768 * k + 32:768 * k + 64])


def set_field(ek, index, value):
    """ek with its 12-bit field `index` (coefficient index of t_hat, 0 ... 256 k - 1) replaced by `value`"""
    b = bytearray(ek)
    bit = 12 * index
    word = int.from_bytes(b[bit // 8:bit // 8 + 2], "little")
    sh = bit % 8
    word = (word & ~(0xFFF << sh)) | ((value & 0xFFF) << sh)
    b[bit // 8:bit // 8 + 2] = word.to_bytes(2, "little")
    return bytes(b)
