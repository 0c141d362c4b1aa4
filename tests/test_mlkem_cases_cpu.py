"""The case tables of tests/helpers/mlkem_cases.py against the pure-Python model, instance by instance: the conditions that keep the device tests
that run these tables (tests/test_gpu_mlkem_edges.py, tests/test_gpu_mlkem_large.py) honest.  No GPU, no library."""
import pytest

from tests.helpers import fips203_kpke_model as M
from tests.helpers import mlkem_cases as C
from tests.helpers import mlkem_model as R
from tests.helpers.mlkem_gpu import NAMES, flip, model, offsets

Q = M.Q


@pytest.mark.parametrize("name", NAMES)
def test_flipped_and_extreme_ciphertexts_are_rejected_with_the_rejection_key(name):
    h = C.honest(name, 1)
    k, _, _, du, _ = M.PARAMS[name]
    n, c1 = R.sizes(name)["ct"], 32 * du * k
    spread = sorted({0, 1, c1 // 3, c1 // 2, c1 - 2, c1 - 1, c1, c1 + 1, c1 + (n - c1) // 2, n - 2, n - 1} | {(i * n) // 9 for i in range(1, 9)})
    assert len(spread) >= 16 and sum(p < c1 for p in spread) >= 6 and sum(p >= c1 for p in spread) >= 5
    for pos in spread:
        bad = flip(h["c"], pos, pos % 8)
        got = R.decaps_internal(h["dk"], bad, name)
        assert got == R.rejection_key(h["dk"], bad, name) and got != h["K"], (name, pos)
    inputs, want = C.extreme_ct(name)
    assert inputs["ct"][0] == bytes(n) and inputs["ct"][1] == bytes([0xFF] * n)
    assert inputs["ct"][2][:c1] == C.honest(name, 4)["c"][:c1] and set(inputs["ct"][2][c1:]) == {0xFF}
    for dk, c, w in zip(inputs["dk"], inputs["ct"], want):
        assert w == R.decaps_internal(dk, c, name) == R.rejection_key(dk, c, name) and w != inputs["K0"], name
    assert len(set(want)) == 3


@pytest.mark.parametrize("name", NAMES)
def test_every_ct_byte_equals_decaps_on_a_sample_and_both_ends(name):
    inputs, want = C.every_ct_byte(name)
    n = R.sizes(name)["ct"]
    h = C.honest(name, 1)
    assert len(want) == len(inputs["ct"]) == len(inputs["dk"]) == n + 3
    for i in range(n):                                                   # exactly bit i mod 8 of byte i differs
        diff = [(p, a ^ b) for p, (a, b) in enumerate(zip(inputs["ct"][i], h["c"])) if a != b]
        assert diff == [(i, 1 << (i % 8))], (name, i)
    assert inputs["ct"][n:] == [h["c"]] * 3 and want[n:] == [h["K"]] * 3
    assert len(set(want[:n])) == n and h["K"] not in want[:n]
    for i in sorted(set(range(0, n, 16)) | {0, 1, n - 2, n - 1, n, n + 2}):
        assert R.decaps_internal(inputs["dk"][i], inputs["ct"][i], name) == want[i], (name, i)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("value", [Q, 4095, Q - 1])
def test_every_ek_field_equals_check_ek(name, value):
    inputs, want = C.every_ek_field(name, value)
    n = 256 * M.PARAMS[name][0]
    ek = C.honest(name, 2)["ek"]
    assert len(want) == len(inputs["ek"]) == n + 1 and inputs["ek"][n] == ek
    for i in range(n):
        fields = C.raw_fields(inputs["ek"][i][:n * 3 // 2])
        assert fields[i] == value and fields[:i] + fields[i + 1:] == C.raw_fields(ek[:n * 3 // 2])[:i] + C.raw_fields(ek[:n * 3 // 2])[i + 1:], (name, i)
        assert inputs["ek"][i][n * 3 // 2:] == ek[n * 3 // 2:]
    assert want == [1 if R.check_ek(e, name) else 0 for e in inputs["ek"]]
    assert want == ([0] * n + [1] if value >= Q else [1] * (n + 1))


@pytest.mark.parametrize("name", NAMES)
def test_every_dk_byte_equals_check_dk(name):
    inputs, want = C.every_dk_byte(name)
    k = M.PARAMS[name][0]
    n = R.sizes(name)["dk"]
    assert len(want) == len(inputs["dk"]) == n
    assert want == [1 if R.check_dk(dk, name) else 0 for dk in inputs["dk"]]
    assert want.count(0) == 384 * k + 64 and want.index(0) == 384 * k and want[768 * k + 63] == 0 and want[768 * k + 64] == 1
    dk = C.honest(name, 3)["dk"]
    assert all(sum(a != b for a, b in zip(x, dk)) == 1 and x[i] == dk[i] ^ (1 << (i % 8)) for i, x in enumerate(inputs["dk"]))


@pytest.mark.parametrize("name", NAMES)
def test_lifted_keys_decode_to_the_canonical_ones_and_keep_the_shared_secret(name):
    k = M.PARAMS[name][0]
    inputs, want = C.lifted(name, 3)
    assert len(inputs["ek"]) == 5
    seen = []
    for i in range(5):
        ek, ek0, dk, dk0 = inputs["ek"][i], inputs["ek0"][i], inputs["dk"][i], inputs["dk0"][i]
        assert ek[384 * k:] == ek0[384 * k:] and dk[768 * k:] == dk0[768 * k:] and dk[384 * k:768 * k] == ek[:384 * k]
        assert R.check_ek(ek0, name) and R.check_dk(dk0, name)
        for body, body0 in ((ek[:384 * k], ek0[:384 * k]), (dk[:768 * k], dk0[:768 * k])):
            for p in range(0, len(body), 384):
                raw, raw0 = C.raw_fields(body[p:p + 384]), C.raw_fields(body0[p:p + 384])
                assert M.byte_decode(body[p:p + 384], 12) == raw0 == M.byte_decode(body0[p:p + 384], 12)
                assert all(a == (b + Q if b <= C.LIFT_MAX else b) for a, b in zip(raw, raw0))          # every field that can be lifted is
                assert sum(a >= Q for a in raw) >= 32, (name, i, p)
            seen.append(sum(a >= Q for a in C.raw_fields(body)))
        assert (want["check_ek"][i], want["check_dk"][i]) == (0, 0) == (int(R.check_ek(ek, name)), int(R.check_dk(dk, name)))
        assert (want["K"][i], want["c"][i]) == R.encaps_internal(ek, inputs["m"][i], name)
        assert want["K"][i] != inputs["K0"][i] and want["c"][i] != inputs["ct"][i]            # H(ek) differs
        assert (inputs["K0"][i], inputs["ct"][i]) == R.encaps_internal(ek0, inputs["m"][i], name)
        assert want["decaps"][i] == R.decaps_internal(dk, inputs["ct"][i], name) == R.decaps_internal(dk0, inputs["ct"][i], name)
        if i < 3:
            assert want["decaps"][i] == inputs["K0"][i]
    assert C.raw_fields(inputs["ek"][3][:384 * k]) == [4095] * (256 * k) and C.raw_fields(inputs["ek0"][3][:384 * k]) == [766] * (256 * k)
    assert C.raw_fields(inputs["ek"][4][:384 * k]) == [Q] * (256 * k) and C.raw_fields(inputs["ek0"][4][:384 * k]) == [0] * (256 * k)
    print(name, "lifted fields per ek / dk body:", seen)


def test_tiled_indexes_the_period():
    t, same = C.tiled("ML-KEM-1024", 7, 174766)
    assert same is t and t.period == 7 and t.count == 174766 and t.fields is model("ML-KEM-1024", 7)
    assert all(len(t.fields[f]) == 7 for f in ("d", "z", "m", "ek", "dk", "K", "c"))
    for i in (0, 6, 7, 8, 63, 64, 255, 256, 174762, 174765):
        assert t.index(i) == i % 7 and t.item("dk", i) is model("ML-KEM-1024", 7)["dk"][i % 7]
    assert len({t.item("c", i) for i in range(7)}) == 7                  # the period is a true period: no two of its instances agree
    assert (2 ** 32) % R.sizes("ML-KEM-1024")["ct"] != 0 and (2 ** 32) % 24576 != 0       # a 2^32-byte wrap is no whole number of instances
    small, _ = C.tiled("ML-KEM-768", 67, 81)
    assert small.items("K") == [model("ML-KEM-768", 67)["K"][i % 67] for i in range(81)] and len(small.items("K")) == 81


def test_offsets_name_every_buffer():
    o = offsets(0, 1, in_m=4)
    assert o["in_m"] == 4 and o["in_ek"] == 0 and o["out_ok"] == 1 and len(o) == 11
    with pytest.raises(AssertionError):
        offsets(in_x=1)
