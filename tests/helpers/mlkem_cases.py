"""Case tables for the ML-KEM device tests, built from the pure-Python model alone (tests/helpers/mlkem_model.py): every function returns
(inputs, expected) and knows nothing of the library.  tests/test_mlkem_cases_cpu.py checks on the CPU that each table has the property it
claims; tests/test_gpu_mlkem_edges.py and tests/test_gpu_mlkem_large.py run every instance of every table on the device.

  every_ct_byte   one flipped bit in every byte of a ciphertext: the comparison of c with c' at every position
  every_ek_field  one 12-bit field of an encapsulation key set to a value, at every field: the modulus check at every field
  every_dk_byte   one flipped bit in every byte of a decapsulation key: the hash check at every byte, inside and outside the hashed range
  lifted          keys whose 12-bit fields v <= 4095 - q are written as v + q: the reduction that FIPS 203 defines for ByteDecode_12
  extreme_ct      ciphertexts of all 0x00, all 0xFF and an honest c1 with c2 all 0xFF
  tiled           instance i is instance i mod period of the cached model run: large batches as a period and an index rule"""
import functools
import random
from collections import namedtuple

from tests.helpers import fips203_kpke_model as M
from tests.helpers import mlkem_model as R
from tests.helpers.mlkem_gpu import NAMES, flip, model

Q = M.Q
LIFT_MAX = 4095 - Q                                                      # 766: the fields that have a second 12-bit spelling


def honest(name, salt):
    """one honest instance from a fixed seed: {"d", "z", "m", "ek", "dk", "K", "c"}"""
    rng = random.Random(5003 * NAMES.index(name) + 17 * salt + 3)
    d, z, m = rng.randbytes(32), rng.randbytes(32), rng.randbytes(32)
    ek, dk = R.keygen_internal(d, z, name)
    key, c = R.encaps_internal(ek, m, name)
    return {"d": d, "z": z, "m": m, "ek": ek, "dk": dk, "K": key, "c": c}


def raw_fields(body):
    """the 12-bit fields of `body` as they are written, not reduced"""
    total = int.from_bytes(bytes(body), "little")
    return [(total >> (12 * i)) & 0xFFF for i in range(len(body) * 2 // 3)]


def pack_fields(fields):
    total = 0
    for i, v in enumerate(fields):
        assert 0 <= v < 4096
        total |= v << (12 * i)
    return total.to_bytes(len(fields) * 3 // 2, "little")


def lift(body):
    """`body` (a multiple of 384 bytes) with every field v <= 4095 - q written as v + q"""
    return pack_fields([v + Q if v <= LIFT_MAX else v for v in raw_fields(body)])


@functools.lru_cache(maxsize=None)
def every_ct_byte(name):
    h = honest(name, 1)
    n = R.sizes(name)["ct"]
    cts = [flip(h["c"], i, i % 8) for i in range(n)] + [h["c"]] * 3
    want = [R.rejection_key(h["dk"], c, name) for c in cts[:n]] + [h["K"]] * 3
    return {"dk": [h["dk"]] * (n + 3), "ct": cts}, want


@functools.lru_cache(maxsize=None)
def every_ek_field(name, value):
    h = honest(name, 2)
    n = 256 * M.PARAMS[name][0]
    eks = [R.set_field(h["ek"], i, value) for i in range(n)] + [h["ek"]]
    return {"ek": eks}, [0 if value >= Q else 1] * n + [1]


@functools.lru_cache(maxsize=None)
def every_dk_byte(name):
    h = honest(name, 3)
    k = M.PARAMS[name][0]
    n = R.sizes(name)["dk"]
    dks = [flip(h["dk"], i, i % 8) for i in range(n)]
    return {"dk": dks}, [0 if 384 * k <= i < 768 * k + 64 else 1 for i in range(n)]


@functools.lru_cache(maxsize=None)
def lifted(name, count):
    """`count` honest instances and two whose t_hat is constant, 766 (written 4095) and 0 (written q), all in the lifted spelling.
    inputs: "ek" and "dk" lifted (ek[0 : 384 k] and dk[0 : 768 k]; rho, h and z as they are), "m", "ct" the ciphertext of the CANONICAL key, and
    "ek0", "dk0", "K0" the canonical key pair and shared secret.  expected: "K", "c" Encaps on the lifted ek; "decaps" Decaps of "ct" with the lifted dk;
    "check_ek" and "check_dk"."""
    k = M.PARAMS[name][0]
    inst = [honest(name, 10 + i) for i in range(count)]
    for i, const in enumerate((LIFT_MAX, 0)):                            # the two special keys: s_hat, rho and z of an honest one, t_hat constant
        base = honest(name, 50 + i)
        ek = pack_fields([const] * (256 * k)) + base["ek"][384 * k:]
        dk = base["dk"][:384 * k] + ek + M.H(ek) + base["z"]
        key, c = R.encaps_internal(ek, base["m"], name)
        inst.append({"m": base["m"], "ek": ek, "dk": dk, "K": key, "c": c})
    eks = [lift(h["ek"][:384 * k]) + h["ek"][384 * k:] for h in inst]
    dks = [lift(h["dk"][:768 * k]) + h["dk"][768 * k:] for h in inst]
    enc = [R.encaps_internal(ek, h["m"], name) for ek, h in zip(eks, inst)]
    inputs = {"ek": eks, "dk": dks, "m": [h["m"] for h in inst], "ct": [h["c"] for h in inst],
              "ek0": [h["ek"] for h in inst], "dk0": [h["dk"] for h in inst], "K0": [h["K"] for h in inst]}
    expected = {"K": [e[0] for e in enc], "c": [e[1] for e in enc], "decaps": [R.decaps_internal(dk, h["c"], name) for dk, h in zip(dks, inst)],
                "check_ek": [0] * len(inst), "check_dk": [0] * len(inst)}
    return inputs, expected


@functools.lru_cache(maxsize=None)
def extreme_ct(name):
    h = honest(name, 4)
    k, _, _, du, _ = M.PARAMS[name]
    n, c1 = R.sizes(name)["ct"], 32 * du * k
    cts = [bytes(n), bytes([0xFF] * n), h["c"][:c1] + bytes([0xFF] * (n - c1))]
    return {"dk": [h["dk"]] * 3, "ct": cts, "K0": h["K"]}, [R.decaps_internal(h["dk"], c, name) for c in cts]


class Tiled(namedtuple("Tiled", "name period count fields")):
    """instance i of field f is fields[f][index(i)]: `fields` holds the `period` instances of model(name, period), never `count` objects"""

    def index(self, i):
        return i % self.period

    def item(self, field, i):
        return self.fields[field][self.index(i)]

    def items(self, field):
        """all `count` items as a list: for small counts only"""
        return [self.item(field, i) for i in range(self.count)]


def tiled(name, period, count):
    """(inputs, expected) as one Tiled: the fields "d", "z", "m", "ek", "dk", "c" are inputs of one operation or expected outputs of another"""
    t = Tiled(name, period, count, model(name, period))
    return t, t
