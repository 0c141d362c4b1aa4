"""ML-KEM on the MI355X at the inputs where psf_mlkem.hip takes another path, against the pure-Python model, byte for byte over every instance.

Alignment.  The unit branches on pointer alignment in four places: CatReader::le64 (8-byte loads), kc::PtrReader for H, put_words (8-byte stores) and
the word-wise comparison of c with c' in k_decaps_tail (4-byte loads).  tests/test_gpu_mlkem.py puts every buffer one byte past a 16-byte boundary,
which takes the byte-wise branch of all four; here the three algorithms run with every buffer at 0, 4 and 8, and with mixes in which one input of a
reader is aligned and the other is not, at one, two and five waves of instances.

Positions and values.  The case tables of tests/helpers/mlkem_cases.py (checked against the model by tests/test_mlkem_cases_cpu.py): a flipped bit
in every byte of a ciphertext, q, 4095 and q - 1 in every field of an encapsulation key, a flipped bit in every byte of a decapsulation key, keys
whose fields are written v + q, and ciphertexts of all 0x00 / 0xFF.  Every instance of every table is compared.

Every call keeps the assertions of tests/test_gpu_mlkem.py: guard bytes on both sides of every output, the workspace all zero afterwards, the
sampler flag unchanged (tests/helpers/mlkem_gpu.py)."""
import pytest

from tests.helpers import fips203_kpke_model as M
from tests.helpers import mlkem_cases as C
from tests.helpers import mlkem_model as R
from tests.helpers.mlkem_gpu import NAMES, _run_check, dev_decaps, dev_encaps, dev_keygen, flip, model, offsets

pytestmark = pytest.mark.gpu

SHAPES = [("ML-KEM-768", 67), ("ML-KEM-512", 259), ("ML-KEM-1024", 3)]
PATTERNS = {
    "all0": offsets(0, 0),
    "all4": offsets(4, 4),                                               # the word-wise comparison with the byte-wise readers and writers
    "all8": offsets(8, 8),
    "in0_out1": offsets(0, 1),
    "in1_out0": offsets(1, 0),
    "m1_ek0": offsets(0, 0, in_m=1),                                     # k_encaps_hash: H reads ek through a fast PtrReader, G reads m || h through a slow CatReader
    "dk0_ct4": offsets(0, 0, in_ct=4),                                   # k_decaps_tail: c against c' by words, J(z || c) by bytes
    "dk4_ct0": offsets(0, 0, in_dk=4),                                   # k_g reads h from dk by bytes; so does J its z
}


@pytest.fixture(scope="module")
def K():
    import tools_amd
    return tools_amd.mlkem


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def differing(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


# ---- alignment ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("name,count", SHAPES)
def test_round_trip_equals_the_model_bytes_at_every_alignment(K, torch, name, count, pattern):
    offs = PATTERNS[pattern]
    ref = model(name, count)
    ek, dk, (bek, pek) = dev_keygen(torch, K, name, ref["d"], ref["z"], flag=0, offs=offs)
    assert ek == ref["ek"], (name, count, pattern, differing(ek, ref["ek"]))
    assert dk == ref["dk"], (name, count, pattern, differing(dk, ref["dk"]))
    ss, ct = dev_encaps(torch, K, name, None, ref["m"], flag=4, ek_ptr=pek, offs=offs)       # from the device's own ek, where keygen left it ("out_ek")
    assert ct == ref["c"], (name, count, pattern, differing(ct, ref["c"]))
    assert ss == ref["K"], (name, count, pattern, differing(ss, ref["K"]))
    ss2, ct2 = dev_encaps(torch, K, name, ref["ek"], ref["m"], flag=0, offs=offs)            # from the model's ek ("in_ek")
    assert ct2 == ref["c"], (name, count, pattern, differing(ct2, ref["c"]))
    assert ss2 == ref["K"], (name, count, pattern, differing(ss2, ref["K"]))
    got = dev_decaps(torch, K, name, ref["dk"], ref["c"], flag=4, offs=offs)
    assert got == ref["K"], (name, count, pattern, differing(got, ref["K"]))
    del bek


def mixed_batch(torch, K, count, tampered, offs):
    """valid and tampered ciphertexts side by side in the waves of k_decaps_tail, then the complement; instance i is instance i mod 67 of the model's run"""
    name = "ML-KEM-768"
    ref, _ = C.tiled(name, 67, count)
    dks, cs, keys = ref.items("dk"), ref.items("c"), ref.items("K")
    pos = R.sizes(name)["ct"] // 2
    for chosen in (tampered, set(range(count)) - tampered):
        cts = [flip(c, pos + i % 7, i % 8) if i in chosen else c for i, c in enumerate(cs)]
        want = [R.rejection_key(dks[i], cts[i], name) if i in chosen else keys[i] for i in range(count)]
        for i in sorted(chosen)[:5]:
            assert R.decaps_internal(dks[i], cts[i], name) == want[i]
        got = dev_decaps(torch, K, name, dks, cts, offs=offs)
        assert got == want, (count, offs, differing(got, want))


@pytest.mark.parametrize("off", [0, 4])
def test_decaps_of_a_mixed_batch_at_aligned_pointers(K, torch, off):
    mixed_batch(torch, K, 67, {0, 5, 63, 64, 66}, off)


@pytest.mark.parametrize("off", [0, 1])
def test_decaps_of_a_mixed_batch_with_seventeen_instances_in_the_last_workgroup(K, torch, off):
    """81 = 64 + 17: in the last workgroup np = 17, so the second wave's clamp `first + u < np ? first + u : np - 1` cuts inside its first group of eight"""
    mixed_batch(torch, K, 81, {0, 5, 63, 64, 66, 79, 80}, off)


# ---- positions and values ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_a_flipped_bit_in_every_ciphertext_byte_gives_the_rejection_key(K, torch, name, off):
    inputs, want = C.every_ct_byte(name)
    assert len(want) == R.sizes(name)["ct"] + 3 <= 3200
    got = dev_decaps(torch, K, name, inputs["dk"], inputs["ct"], offs=offsets(1, 1, in_ct=off))
    assert got == want, (name, off, "ciphertext bytes whose flip went unnoticed, or honest instances rejected:", differing(got, want))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("value", [M.Q, 4095, M.Q - 1])
@pytest.mark.parametrize("name", NAMES)
def test_check_ek_at_every_field(K, torch, name, value, off):
    inputs, want = C.every_ek_field(name, value)
    assert len(want) == 256 * M.PARAMS[name][0] + 1 <= 3200
    got = _run_check(torch, K.check_ek_dev, name, inputs["ek"], offs=off)
    assert got == want, (name, value, off, "fields:", differing(got, want))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_check_dk_at_every_byte(K, torch, name, off):
    inputs, want = C.every_dk_byte(name)
    assert len(want) == R.sizes(name)["dk"] <= 3200
    got = _run_check(torch, K.check_dk_dev, name, inputs["dk"], offs=off)
    assert got == want, (name, off, "bytes:", differing(got, want))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_fields_written_above_q_are_reduced(K, torch, name, off):
    """ByteDecode_12 reduces mod q (FIPS 203 Algorithm 6); Encaps does not check ek, so it must take a field v + q for v"""
    inputs, want = C.lifted(name, 3)
    ss, ct = dev_encaps(torch, K, name, inputs["ek"], inputs["m"], offs=off)
    assert ct == want["c"], (name, off, differing(ct, want["c"]))
    assert ss == want["K"], (name, off, differing(ss, want["K"]))
    got = dev_decaps(torch, K, name, inputs["dk"], inputs["ct"], offs=off)
    assert got == want["decaps"], (name, off, differing(got, want["decaps"]))
    assert got[:3] == inputs["K0"][:3]
    assert _run_check(torch, K.check_ek_dev, name, inputs["ek"], offs=off) == want["check_ek"] == [0] * 5
    assert _run_check(torch, K.check_dk_dev, name, inputs["dk"], offs=off) == want["check_dk"] == [0] * 5
    assert _run_check(torch, K.check_ek_dev, name, inputs["ek0"], offs=off) == [1] * 5               # the canonical spellings of the same keys pass
    assert _run_check(torch, K.check_dk_dev, name, inputs["dk0"], offs=off) == [1] * 5


@pytest.mark.parametrize("name", NAMES)
def test_decaps_of_extreme_ciphertexts(K, torch, name):
    inputs, want = C.extreme_ct(name)
    for off in (0, 1):
        got = dev_decaps(torch, K, name, inputs["dk"], inputs["ct"], offs=off)
        assert got == want, (name, off, differing(got, want))
