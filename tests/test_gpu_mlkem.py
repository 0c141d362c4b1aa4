"""Batched ML-KEM on the MI355X (tools_amd/mlkem.py, psf_mlkem_*) against the pure-Python model of tests/helpers/mlkem_model.py: KeyGen_internal,
Encaps_internal and Decaps_internal byte for byte, implicit rejection alone and mixed with valid ciphertexts inside one wave, the two input checks
per instance, and the buffer rules.  Every comparison is exact equality over every instance; every output sits between guard bytes at a pointer
one byte past an aligned address; after every call the workspace is all zero and the sampler flag is what it was.  The harness is
tests/helpers/mlkem_gpu.py; the aligned paths, the position sweeps and the large batches are tests/test_gpu_mlkem_edges.py and _large.py."""
import pytest

from tests.helpers import fips203_kpke_model as M
from tests.helpers import mlkem_model as R
from tests.helpers.mlkem_gpu import NAMES, Scratch, _out, _put, _run_check, _take, dev_decaps, dev_encaps, dev_keygen, flip, model

pytestmark = pytest.mark.gpu

SHAPES = [(n, c) for c in (1, 3) for n in NAMES] + [("ML-KEM-768", 67), ("ML-KEM-512", 259)]


@pytest.fixture(scope="module")
def K():
    import tools_amd
    return tools_amd.mlkem


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


# ---- the three algorithms ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,count", SHAPES)
def test_keygen_encaps_decaps_equal_the_model_bytes(K, torch, name, count):
    ref = model(name, count)
    ek, dk, (bek, pek) = dev_keygen(torch, K, name, ref["d"], ref["z"], flag=0)
    assert ek == ref["ek"], (name, count, [i for i in range(count) if ek[i] != ref["ek"][i]][:8])
    assert dk == ref["dk"], (name, count, [i for i in range(count) if dk[i] != ref["dk"][i]][:8])
    ss, ct = dev_encaps(torch, K, name, None, ref["m"], flag=4, ek_ptr=pek)            # from the device's own ek, where keygen left it
    assert ct == ref["c"], (name, count, [i for i in range(count) if ct[i] != ref["c"][i]][:8])
    assert ss == ref["K"], (name, count)
    ss2, ct2 = dev_encaps(torch, K, name, ref["ek"], ref["m"], flag=0)                 # from the model's ek
    assert ct2 == ref["c"] and ss2 == ref["K"], (name, count)
    got = dev_decaps(torch, K, name, ref["dk"], ref["c"], flag=4)
    assert got == ref["K"], (name, count, [i for i in range(count) if got[i] != ref["K"][i]][:8])
    del bek


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("count", [1, 3])
def test_decaps_of_a_tampered_ciphertext_is_the_rejection_key(K, torch, name, count):
    ref = model(name, count)
    k, _, _, du, _ = M.PARAMS[name]
    c1 = 32 * du * k
    for pos, bit in ((0, 0), (c1 - 1, 7), (c1, 3), (R.sizes(name)["ct"] - 1, 5)):
        bad = [flip(c, pos, bit) for c in ref["c"]]
        want = [R.decaps_internal(dk, c, name) for dk, c in zip(ref["dk"], bad)]
        assert want == [R.rejection_key(dk, c, name) for dk, c in zip(ref["dk"], bad)]
        assert all(w != key for w, key in zip(want, ref["K"]))
        assert dev_decaps(torch, K, name, ref["dk"], bad) == want, (name, count, pos)


def test_decaps_of_a_mixed_batch_shares_waves_between_both_cases(K, torch):
    name, count = "ML-KEM-768", 67
    ref = model(name, count)
    tampered = {0, 5, 63, 64, 66}
    pos = R.sizes(name)["ct"] // 2
    for chosen in (tampered, set(range(count)) - tampered):
        cts = [flip(c, pos + i % 7, i % 8) if i in chosen else c for i, c in enumerate(ref["c"])]
        want = [R.rejection_key(ref["dk"][i], cts[i], name) if i in chosen else ref["K"][i] for i in range(count)]
        for i in sorted(chosen)[:5]:
            assert R.decaps_internal(ref["dk"][i], cts[i], name) == want[i]
        got = dev_decaps(torch, K, name, ref["dk"], cts)
        assert got == want, [i for i in range(count) if got[i] != want[i]]


# ---- the input checks ----------------------------------------------------------------------------------------------------------------------------------

def test_check_ek_per_instance(K, torch):
    name, count = "ML-KEM-768", 67
    k = M.PARAMS[name][0]
    ref = model(name, count)
    last = 256 * k - 1
    cases = {0: (0, M.Q), 63: (last, 4095), 64: (last, M.Q), 66: (0, 4095)}
    eks = [R.set_field(ek, *cases[i]) if i in cases else ek for i, ek in enumerate(ref["ek"])]
    eks[1] = R.set_field(eks[1], 0, M.Q - 1)                               # the largest valid field, first and last coefficient
    eks[65] = R.set_field(eks[65], last, M.Q - 1)
    eks[2] = eks[2][:-32] + bytes([0xFF] * 32)                             # rho is not checked
    want = [1 if R.check_ek(ek, name) else 0 for ek in eks]
    assert want == [0 if i in cases else 1 for i in range(count)]
    assert _run_check(torch, K.check_ek_dev, name, eks) == want
    swapped = {i: (last - f, v) for i, (f, v) in cases.items()}            # the same values at the other end
    eks = [R.set_field(ek, *swapped[i]) if i in swapped else ek for i, ek in enumerate(ref["ek"])]
    assert _run_check(torch, K.check_ek_dev, name, eks) == want
    assert _run_check(torch, K.check_ek_dev, name, ref["ek"]) == [1] * count
    for other in NAMES:
        three = model(other, 3)
        bad = [three["ek"][0], R.set_field(three["ek"][1], 256 * M.PARAMS[other][0] - 1, M.Q), three["ek"][2]]
        assert _run_check(torch, K.check_ek_dev, other, bad) == [1, 0, 1]


def test_check_dk_per_instance(K, torch):
    name, count = "ML-KEM-768", 67
    k = M.PARAMS[name][0]
    ref = model(name, count)
    cases = {0: 768 * k + 32, 63: 768 * k + 63, 64: 384 * k, 66: 768 * k + 31}          # h first / last byte, embedded ek first / last byte
    dks = [flip(dk, cases[i], i % 8) if i in cases else dk for i, dk in enumerate(ref["dk"])]
    dks[1] = flip(dks[1], 0)                                               # dk_pke and z are outside the hash check
    dks[65] = flip(dks[65], 768 * k + 95, 7)
    want = [1 if R.check_dk(dk, name) else 0 for dk in dks]
    assert want == [0 if i in cases else 1 for i in range(count)]
    assert _run_check(torch, K.check_dk_dev, name, dks) == want
    for other in NAMES:
        three = model(other, 3)
        ko = M.PARAMS[other][0]
        bad = [three["dk"][0], three["dk"][1], flip(three["dk"][2], 768 * ko + 40)]
        assert _run_check(torch, K.check_dk_dev, other, bad) == [1, 1, 0]


# ---- streams and host forms --------------------------------------------------------------------------------------------------------------------------

def test_on_a_stream_behind_the_kernel_that_produces_the_inputs(K, torch):
    name, count = "ML-KEM-512", 3
    ref = model(name, count)
    sz = R.sizes(name)
    masked_d = bytes(b ^ 0x3C for b in b"".join(ref["d"]))
    masked_z = bytes(b ^ 0x3C for b in b"".join(ref["z"]))
    src_d, src_z = _put(torch, [masked_d], 0)[0], _put(torch, [masked_z], 0)[0]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_dev = torch.bitwise_xor(src_d, 0x3C)                             # the inputs exist only once this kernel has run on s
        z_dev = torch.bitwise_xor(src_z, 0x3C)
        bek, pek = _out(torch, count * sz["ek"])
        bdk, pdk = _out(torch, count * sz["dk"])
        sc = Scratch(torch, K, name, count, "keygen")
        K.keygen_dev(name, count, d_dev.data_ptr(), z_dev.data_ptr(), pek, pdk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr(), stream=s.cuda_stream)
        bm, pm = _put(torch, ref["m"])
        bss, pss = _out(torch, count * 32)
        bct, pct = _out(torch, count * sz["ct"])
        sc2 = Scratch(torch, K, name, count, "encaps")
        K.encaps_dev(name, count, pek, pm, pss, pct, sc2.ptr, sc2.bytes, stream=s.cuda_stream)       # reads the ek the call before it writes
        bk, pk = _out(torch, count * 32)
        sc3 = Scratch(torch, K, name, count, "decaps")
        K.decaps_dev(name, count, pdk, pct, pk, sc3.ptr, sc3.bytes, stream=s.cuda_stream)
    s.synchronize()
    assert _take(torch, bek, count * sz["ek"], sz["ek"], "ek") == ref["ek"]
    assert _take(torch, bdk, count * sz["dk"], sz["dk"], "dk") == ref["dk"]
    assert _take(torch, bct, count * sz["ct"], sz["ct"], "ct") == ref["c"]
    assert _take(torch, bss, count * 32, 32, "ss") == ref["K"]
    assert _take(torch, bk, count * 32, 32, "decaps") == ref["K"]
    for x in (sc, sc2, sc3):
        x.check("stream")
    del bm


@pytest.mark.parametrize("name", NAMES)
def test_host_forms_equal_the_device_forms(K, torch, name):
    ref = model(name, 3)
    assert K.keygen_internal(name, ref["d"], ref["z"]) == list(zip(ref["ek"], ref["dk"]))
    assert K.encaps_internal(name, ref["ek"], ref["m"]) == list(zip(ref["K"], ref["c"]))
    bad = [ref["c"][0], flip(ref["c"][1], 17, 2), ref["c"][2]]
    want = [ref["K"][0], R.rejection_key(ref["dk"][1], bad[1], name), ref["K"][2]]
    assert K.decaps(name, ref["dk"], bad) == want == dev_decaps(torch, K, name, ref["dk"], bad)
    k = M.PARAMS[name][0]
    assert K.check_ek(name, [ref["ek"][0], R.set_field(ref["ek"][1], 5, M.Q)]) == [True, False]
    assert K.check_dk(name, [flip(ref["dk"][0], 384 * k + 9), ref["dk"][1]]) == [False, True]
    pairs = K.keygen(name, 2)                                              # Algorithms 19 and 20: fresh randomness, so only consistency is checked
    assert pairs[0] != pairs[1] and all(R.check_dk(dk, name) and R.check_ek(ek, name) for ek, dk in pairs)
    enc = K.encaps(name, [ek for ek, _ in pairs])
    assert K.decaps(name, [dk for _, dk in pairs], [c for _, c in enc]) == [key for key, _ in enc]
    with pytest.raises(ValueError):
        K.encaps(name, [R.set_field(pairs[0][0], 0, 4095)])
