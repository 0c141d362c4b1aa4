"""Batched ML-DSA signing on the MI355X (tools_amd/mldsa.py, psf_mldsa_sign_*) against the restated signer of tests/helpers/mldsa_sign_model.py (which
tests/test_mldsa_sign_cpu.py pins to the model's sign_internal): signatures and attempt counts byte for byte over the searched cases and random
instances, one key per instance and one key for all, M' on both sides of a block edge and mu given, rnd given and NULL; the edges of waves and
workgroups, where every signature verifies under psf_mldsa_verify_dev and equals the signature of the same instance in another batch; independence of
the schedule of `active`; max_rounds of the host form; the clearing of the workspace; Algorithm 2 in Python.  Every run goes through
tests/helpers/mldsa_sign_gpu.py, which checks d_live against d_rounds after every round, the guard bytes, the untouched signatures of unsigned
instances, the cleared workspace and the flag."""
import ctypes as C
import random

import numpy as np
import pytest

from tests.helpers import mldsa_model as M
from tests.helpers.mldsa_gpu import NAMES, dev_verify, keys
from tests.helpers.mldsa_sign_gpu import MU, batch, dev_sign, reference, schedule_full, schedule_half, schedule_readback
from tests.helpers.mlkem_gpu import FILL

pytestmark = pytest.mark.gpu

ERR_SAMPLER = 9


@pytest.fixture(scope="module")
def D():
    import tools_amd
    return tools_amd.mldsa


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _differ(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


@pytest.mark.parametrize("one_key", [False, True], ids=["key_per_instance", "one_key"])
@pytest.mark.parametrize("name", NAMES)
def test_signatures_and_attempts_equal_the_model(D, torch, name, one_key):
    """40 instances with mu given and rnd given: the searched cases (first attempt, at least 16 attempts, z alone, r0 alone, the hint count alone) among them"""
    sks, mus, rnds = batch(name, one_key)
    want = [reference(name, sk, mu, rnd, True) for sk, mu, rnd in zip(sks, mus, rnds)]
    assert len(want) == 40 and max(w[1] for w in want) >= 16 and min(w[1] for w in want) == 1
    sigs, rounds, trail = dev_sign(torch, D, name, sks[0] if one_key else list(sks), list(mus), list(rnds), msg_kind=MU)
    assert rounds == [w[1] for w in want], (name, _differ(rounds, [w[1] for w in want]))
    assert sigs == [w[0] for w in want], (name, _differ(sigs, [w[0] for w in want]))
    assert len(trail) == max(rounds) and trail[-1] == 0


@pytest.mark.parametrize("name", NAMES)
def test_message_bytes_on_both_sides_of_a_block_edge_and_the_deterministic_variant(D, torch, name):
    """tr || M' is 64 bytes longer than M': 71 and 72 bytes are the two sides of its first block edge; d_rnd = NULL is rnd = 32 zero bytes"""
    rng = random.Random(313 + NAMES.index(name))
    sk = keys(name, 3)["sk"]
    for msg_len, one_key in ((71, False), (72, True), (0, True), (300, False)):
        msgs = [rng.randbytes(msg_len) for _ in range(6)]
        sks = sk[0] if one_key else [sk[i % 3] for i in range(6)]
        want = [reference(name, sk[0] if one_key else sk[i % 3], m, bytes(32), False) for i, m in enumerate(msgs)]
        sigs, rounds, _ = dev_sign(torch, D, name, sks, msgs, None, off=3)
        assert (sigs, rounds) == ([w[0] for w in want], [w[1] for w in want]), (name, msg_len)
    # mu given at an aligned pointer, a flag that is already raised stays as it is
    mus = [M.H(M.sk_decode(sk[0], name)[2] + m, 64) for m in msgs]
    sigs, rounds, _ = dev_sign(torch, D, name, [sk[i % 3] for i in range(6)], mus, None, msg_kind=MU, off=0, flag=4)
    assert sigs[::3] == [w[0] for w in want][::3] and rounds[::3] == [w[1] for w in want][::3]


def _pool(name, n):
    rng = random.Random(4177 + n)
    return [rng.randbytes(64) for _ in range(n)], [rng.randbytes(32) for _ in range(n)]


_REF = {}


def _separate(torch, D, name, per_key, n=321):
    """the signatures of the pool's instances signed in shuffled order in batches of 17 (cached): what every other batch must reproduce"""
    if (name, per_key) not in _REF:
        mus, rnds = _pool(name, 321)
        sk = keys(name, 3)["sk"]
        order = list(range(n))
        random.Random(9).shuffle(order)
        out = [None] * n
        for at in range(0, n, 17):
            ids = order[at:at + 17]
            sks = [sk[i % 3] for i in ids] if per_key else sk[0]
            sigs, rounds, _ = dev_sign(torch, D, name, sks, [mus[i] for i in ids], [rnds[i] for i in ids], msg_kind=MU)
            assert all(rounds)
            for i, s in zip(ids, sigs):
                out[i] = s
        _REF[(name, per_key)] = out
    return _REF[(name, per_key)]


@pytest.mark.parametrize("count,per_key", [(1, False), (63, False), (64, False), (65, False), (257, False), (321, False), (65, True), (257, True)])
def test_edges_of_waves_and_workgroups(D, torch, count, per_key):
    name = "ML-DSA-44"
    ks = keys(name, 3)
    mus, rnds = _pool(name, 321)
    sks = [ks["sk"][i % 3] for i in range(count)] if per_key else ks["sk"][0]
    sigs, rounds, trail = dev_sign(torch, D, name, sks, mus[:count], rnds[:count], msg_kind=MU)
    assert all(rounds) and trail[-1] == 0 and len(trail) == max(rounds)
    pks = [ks["pk"][i % 3] for i in range(count)] if per_key else ks["pk"][0]
    ok, why = dev_verify(torch, D, name, pks, mus[:count], sigs, msg_kind=MU)
    assert ok == [1] * count and why == [0] * count
    ref = _separate(torch, D, name, per_key, 257 if per_key else 321)
    assert sigs == ref[:count], (count, per_key, _differ(sigs, ref[:count]))


def test_signatures_do_not_depend_on_the_schedule(D, torch):
    name, count = "ML-DSA-44", 129
    ks = keys(name, 3)
    mus, rnds = _pool(name, 321)
    for per_key in (True, False):
        sks = [ks["sk"][i % 3] for i in range(count)] if per_key else ks["sk"][0]
        runs = [dev_sign(torch, D, name, sks, mus[:count], rnds[:count], msg_kind=MU, schedule=s) for s in (schedule_readback, schedule_full, schedule_half)]
        assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][1] == runs[1][1] == runs[2][1]
        assert runs[0][2] == runs[1][2] and len(runs[2][2]) > len(runs[0][2])                  # sitting out costs rounds, not bytes
        assert all(r > 0 for r in runs[0][1])


@pytest.mark.parametrize("name", NAMES)
def test_host_form_and_max_rounds(D, torch, name):
    sks, mus, rnds = batch(name, False)
    want = [reference(name, sk, mu, rnd, True) for sk, mu, rnd in zip(sks, mus, rnds)]
    sigs, rounds = D.sign_internal(name, list(sks), list(mus), list(rnds), msg_kind=MU)
    assert (sigs, rounds) == ([w[0] for w in want], [w[1] for w in want])
    sigs, rounds = D.sign_internal(name, sks[0], list(mus[:30]), list(rnds[:30]), msg_kind=MU, max_rounds=max(w[1] for w in want[:30]))
    assert (sigs, rounds) == ([w[0] for w in want[:30]], [w[1] for w in want[:30]])
    # max_rounds = 1: exactly the instances the model signs at its first attempt; the others zero; PSF_ERR_SAMPLER
    sz = M.sizes(name)
    sk = np.frombuffer(b"".join(sks), np.uint8).copy()
    mu = np.frombuffer(b"".join(mus), np.uint8).copy()
    rnd = np.frombuffer(b"".join(rnds), np.uint8).copy()
    sig, rd = np.full((40, sz["sig"]), 0xEE, np.uint8), np.full(40, 77, np.uint32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    rc = D._lib().psf_mldsa_sign(0, D.PARAM[name], 40, vp(sk), sz["sk"], vp(mu), 64, 64, MU, vp(rnd), vp(sig), 1, vp(rd))
    assert rc == ERR_SAMPLER
    first = [w[1] == 1 for w in want]
    assert 0 < sum(first) < 40
    assert [int(r) for r in rd] == [1 if f else 0 for f in first]
    assert [bytes(s) for s in sig] == [w[0] if f else bytes(sz["sig"]) for w, f in zip(want, first)]
    with pytest.raises(Exception) as ei:
        D.sign_internal(name, list(sks), list(mus), list(rnds), msg_kind=MU, max_rounds=1)
    assert getattr(ei.value, "status", None) == ERR_SAMPLER


def test_end_clears_a_signing_that_was_not_finished(D, torch):
    """three rounds only: instances remain, their signature bytes are untouched, and after end every byte of the workspace is zero"""
    name, count = "ML-DSA-65", 33
    ks = keys(name, 3)
    mus, rnds = _pool(name, 321)
    sigs, rounds, trail = dev_sign(torch, D, name, [ks["sk"][i % 3] for i in range(count)], mus[:count], rnds[:count], msg_kind=MU, max_rounds=3)
    assert len(trail) == 3 and trail[-1] == rounds.count(0) and 0 < trail[-1] < count
    assert all((s == bytes([FILL]) * len(s)) == (r == 0) for s, r in zip(sigs, rounds))
    assert all(0 <= r <= 3 for r in rounds)


@pytest.mark.parametrize("name", NAMES)
def test_python_sign_and_verify_round_trip(D, name):
    ks = keys(name, 3)
    pk, sk = ks["pk"][1], ks["sk"][1]
    msg, ctx = b"a message of the round trip", b"context"
    det = D.sign(name, sk, msg, ctx=ctx, deterministic=True)
    assert det == M.sign(sk, msg, ctx, bytes(32), name) == D.sign(name, sk, msg, ctx=ctx, deterministic=True)
    fixed = bytes(range(32))
    hedged = D.sign(name, sk, msg, ctx=ctx, random=lambda n: fixed[:n])
    assert hedged == M.sign(sk, msg, ctx, fixed, name) and hedged != det
    fresh = D.sign(name, sk, msg, ctx=ctx)
    assert len({det, hedged, fresh}) == 3
    for s in (det, hedged, fresh):
        assert D.verify(name, pk, msg, s, ctx=ctx) is True
        assert D.verify(name, pk, msg, s, ctx=b"another") is False
        assert D.verify(name, ks["pk"][0], msg, s, ctx=ctx) is False
    assert D.verify(name, pk, msg, D.sign(name, sk, msg)) is True
