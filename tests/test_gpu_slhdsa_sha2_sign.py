"""Batched SLH-DSA signing for the SHA-2 sets on the MI355X (tools_amd/slhdsa_sha2.py, psf_slhdsa_sha2_sign_*) against the pure-Python model of
tests/helpers/slhdsa_sha2_model.py: slh_sign_internal byte for byte.  tests/test_gpu_slhdsa_sign.py's plan over the SHA-2 sets.  Every full model signature
compared against comes from the shared fixture (tests/helpers/slhdsa_sha2_cases.py) through tests/helpers/slhdsa_sha2_sign_cases.py, which replays its
(sk, M, addrnd); signatures of other inputs are checked with exact_by_parts, which pins every byte against the model's own parts for about 0.1 s.  Every
comparison is exact and over every instance; every buffer sits one byte past an aligned address, the signatures between guard bytes, and the workspace
is all zero after every call (tests/helpers/slhdsa_sha2_sign_gpu.py)."""
import random

import pytest

from tests.helpers import slhdsa_sha2_cases as K
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers import slhdsa_sha2_sign_cases as S
from tests.helpers.mlkem_gpu import _out, _put, _take
from tests.helpers.slhdsa_gpu import Scratch
from tests.helpers.slhdsa_sha2_sign_gpu import SignScratch, dev_sign

pytestmark = pytest.mark.gpu

F128, F192, F256 = K.F128, K.F192, K.F256
SHAPES = [(n, c) for n in K.F_SETS for c in (1, 3, 67)] + [(n, 1) for n in K.S_SETS]


@pytest.fixture(scope="module")
def D():
    import tools_amd
    return tools_amd.slhdsa_sha2


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="session")
def fixture():
    return K.fixture()


def _bad(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


@pytest.mark.parametrize("name,count", SHAPES)
def test_hedged_signatures_equal_the_model_bytes(D, torch, fixture, name, count):
    """Instance i is triple i mod 3 of the fixture; then the same batch under one key, sk_stride = 0, every instance triple 0.  3 and 67 instances cross a
    workgroup of the packed tree kernel (66 trees at h' = 3 with 64 to a workgroup, 51 at h' = 4 with 32), so trees of different instances and keys share
    a workgroup; SHA2-256s puts two trees in one.  The T_k input of SLH-DSA-SHA2-128s fills its last SHA-256 block to the byte: its case must not be
    dropped to save time."""
    t = S.hedged(name)
    rows = [t[i % len(t)] for i in range(count)]
    want = [r[3] for r in rows]
    assert want == K.tiled(name, count)[2]
    got = dev_sign(torch, D, name, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert got == want, (name, count, "a key per instance", _bad(got, want))
    sk, msg, addrnd, sig = t[0]
    got = dev_sign(torch, D, name, sk, [msg] * count, [addrnd] * count)
    assert got == [sig] * count, (name, count, "sk_stride = 0", _bad(got, [sig] * count))


@pytest.mark.parametrize("name", K.EDGE_SETS)
def test_the_deterministic_variant_around_the_block_edges(D, torch, fixture, name):
    """d_addrnd NULL.  The four messages of the fixture: the padding edges of H_msg's inner hash and the empty message (d_msg NULL), against the model's
    bytes; three more at the padding edges of HMAC's inner hash past its key block (n + |M| = 55, 56, 64 on SHA-256; 111, 112, 128 on SHA-512), by parts."""
    n = M.PARAMS[name].n
    cases = S.edge_inputs(name)
    assert sorted(len(m) for _, m, _ in cases) == sorted(K.edge_lens(name)) and any(len(m) == 0 for _, m, _ in cases)
    for sk, msg, sig in cases:
        assert dev_sign(torch, D, name, [sk], [msg]) == [sig], (name, len(msg))
        assert dev_sign(torch, D, name, sk, [msg] * 2) == [sig] * 2, (name, len(msg), "sk_stride = 0")
    sk = cases[0][0]
    rng = random.Random(515 + n)
    lens = S.prf_edge_lens(name)
    assert [n + ln for ln in lens] == ([55, 56, 64] if n == 16 else [111, 112, 128])
    for ln in lens:
        msgs = [rng.randbytes(ln) for _ in range(2)]
        got = dev_sign(torch, D, name, [sk, sk], msgs)
        assert [S.exact_by_parts(name, sk, m, None, g) for m, g in zip(msgs, got)] == [None, None], (name, ln)


@pytest.mark.parametrize("name", K.S_SETS)
def test_distinct_keys_and_messages_per_instance_on_the_s_sets(D, torch, name):
    """what covers per-instance tree addresses, FORS subtrees and tops where the fixture has a single triple"""
    ks = K.keys(name, 2)
    n = M.PARAMS[name].n
    rng = random.Random(31 * M.IDS[name] + 2)
    msgs, rnds = [rng.randbytes(K.MSG_LEN) for _ in range(2)], [rng.randbytes(n) for _ in range(2)]
    got = dev_sign(torch, D, name, ks["sk"], msgs, rnds)
    assert [S.exact_by_parts(name, *x) for x in zip(ks["sk"], msgs, rnds, got)] == [None] * 2, name
    msgs, rnds = [rng.randbytes(K.MSG_LEN) for _ in range(3)], [rng.randbytes(n) for _ in range(3)]
    sk = ks["sk"][1]
    got = dev_sign(torch, D, name, sk, msgs, rnds)
    assert [S.exact_by_parts(name, sk, m, r, g) for m, r, g in zip(msgs, rnds, got)] == [None] * 3, name
    assert len(set(got)) == 3


def test_a_batch_of_67_distinct_messages_on_192f(D, torch):
    """67 distinct messages over the 3 keys on the set whose kernels hold F on SHA-256 and H on SHA-512: every lane of a wave works in a different tree.
    Every second instance is hedged, the rest have no addrnd: two calls, since d_addrnd is per call."""
    name = F192
    ks = K.keys(name, 3)
    rng = random.Random(67)
    sks = [ks["sk"][i % 3] for i in range(67)]
    msgs = [rng.randbytes(K.MSG_LEN) for _ in range(67)]
    rnds = [rng.randbytes(24) if i % 2 == 0 else None for i in range(67)]
    assert len(set(msgs)) == 67
    even, odd = list(range(0, 67, 2)), list(range(1, 67, 2))
    got = [None] * 67
    for i, g in zip(even, dev_sign(torch, D, name, [sks[i] for i in even], [msgs[i] for i in even], [rnds[i] for i in even])):
        got[i] = g
    for i, g in zip(odd, dev_sign(torch, D, name, [sks[i] for i in odd], [msgs[i] for i in odd])):
        got[i] = g
    bad = [(i, r) for i in range(67) for r in [S.exact_by_parts(name, sks[i], msgs[i], rnds[i], got[i])] if r is not None]
    assert not bad, bad[:8]


def test_on_a_stream_keygen_then_sign_then_verify(D, torch):
    """signing reads the sk that KeyGen writes and Verify the signatures that signing writes, all queued on one non-default stream, all through the sha2
    entry points"""
    name, count = F128, 3
    ref = K.keys(name, 3)
    sz = M.sizes(name)
    rng = random.Random(90)
    msgs = [rng.randbytes(K.MSG_LEN) for _ in range(count)]
    flipped = [msgs[0], K.flip(msgs[1], 5, 2), msgs[2]]
    src = [_put(torch, ref[k], 0)[0] for k in ("sk_seed", "sk_prf", "pk_seed")]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        bpk, ppk = _out(torch, count * sz["pk"])
        bsk, psk = _out(torch, count * sz["sk"])
        sc = Scratch(torch, D, name, count, "keygen")
        D.keygen_dev(name, count, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), ppk, psk, sc.ptr, sc.bytes, stream=st.cuda_stream)
        bm, pm = _put(torch, msgs)
        bf, pf = _put(torch, flipped)
        bsig, psig = _out(torch, count * sz["sig"])
        sc2 = SignScratch(torch, D, name, count)
        D.sign_dev(name, count, psk, pm, K.MSG_LEN, None, psig, sc2.ptr, sc2.bytes, stream=st.cuda_stream)
        bok, pok = _out(torch, count)
        bok2, pok2 = _out(torch, count)
        sc3, sc4 = Scratch(torch, D, name, count, "verify"), Scratch(torch, D, name, count, "verify")
        D.verify_dev(name, count, ppk, pm, K.MSG_LEN, psig, pok, sc3.ptr, sc3.bytes, stream=st.cuda_stream)
        D.verify_dev(name, count, ppk, pf, K.MSG_LEN, psig, pok2, sc4.ptr, sc4.bytes, stream=st.cuda_stream)
    st.synchronize()
    assert _take(torch, bsk, count * sz["sk"], sz["sk"], "sk") == ref["sk"]
    assert [b[0] for b in _take(torch, bok, count, 1, "ok")] == [1] * count
    assert [b[0] for b in _take(torch, bok2, count, 1, "ok")] == [1, 0, 1]
    sigs = _take(torch, bsig, count * sz["sig"], sz["sig"], "sig")
    assert all(M.verify_internal(name, m, s, pk) for m, s, pk in zip(msgs, sigs, ref["pk"]))
    sc.check("stream", cleared=True)
    sc2.check("stream")
    sc3.check("stream", cleared=False)
    del bm, bf, bpk


def test_host_and_python_forms(D, torch, fixture):
    name = F128
    t = S.hedged(name)
    sks, msgs, rnds, sigs = ([r[f] for r in t] for f in range(4))
    assert D.sign_internal(name, sks, msgs, rnds) == dev_sign(torch, D, name, sks, msgs, rnds) == sigs
    one = dev_sign(torch, D, name, sks[0], msgs, rnds)
    assert D.sign_internal(name, sks[0], msgs, rnds) == one and one[0] == sigs[0]
    sk0, m0, s0 = S.edge_inputs(name)[3]
    assert m0 == b"" and D.sign_internal(name, sk0, [m0]) == [s0]         # deterministic, the empty message: two NULL pointers
    # Algorithm 22
    sk = K.keys(K.CTX_SET, K.distinct(K.CTX_SET))["sk"][0]
    assert sorted(fixture["ctx"]) == [0, 1, 255]
    for ln, (pk, msg, ctx, sig) in fixture["ctx"].items():
        assert D.sign(K.CTX_SET, sk, msg, ctx=ctx, deterministic=True) == sig, ln
    pk, msg, ctx, sig = fixture["ctx"][1]
    with pytest.raises(ValueError):
        D.sign(K.CTX_SET, sk, msg, ctx=bytes(256))
    a, b = D.sign(K.CTX_SET, sk, msg, ctx=ctx), D.sign(K.CTX_SET, sk, msg, ctx=ctx)
    assert a != b and a != sig
    assert M.verify(K.CTX_SET, msg, a, ctx, pk) and M.verify(K.CTX_SET, msg, b, ctx, pk)
    assert D.verify(K.CTX_SET, pk, msg, a, ctx=ctx) is True
