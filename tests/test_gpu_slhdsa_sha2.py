"""Batched SLH-DSA for the SHA-2 parameter sets on the MI355X (tools_amd/slhdsa_sha2.py, psf_slhdsa_sha2_*) against the pure-Python model of
tests/helpers/slhdsa_sha2_model.py (pinned by tests/test_slhdsa_sha2_model_cpu.py and tests/test_slhdsa_sha2_cpu.py; there is no other SLH-DSA
implementation to compare with): slh_keygen_internal byte for byte, slh_verify_internal of honest signatures with one key per instance and one key for
all, message lengths around the padding edges of H_msg's inner hash, mixed batches with tampered instances inside one wave on SHA2-128f (SHA-256
throughout) and SHA2-192f (F on SHA-256, H and T_l on SHA-512 in one kernel), the 67 chains and the 64-bit idx_tree of 256f, a stream, the host forms and
Algorithm 24.  Every comparison is exact equality over every instance; every output sits between guard bytes at a pointer one byte past an aligned
address; after KeyGen the workspace is all zero.  The honest signatures come from one session fixture (tests/helpers/slhdsa_sha2_cases.py): three per f
set, one per s set, signed once by the model's sign_internal.  The harness is tests/helpers/slhdsa_sha2_gpu.py."""
import pytest

from tests.helpers import slhdsa_sha2_cases as K
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers.mlkem_gpu import _out, _put, _take
from tests.helpers.slhdsa_gpu import Scratch
from tests.helpers.slhdsa_sha2_gpu import dev_keygen, dev_verify

pytestmark = pytest.mark.gpu

F128, F192, F256 = K.F128, K.F192, K.F256
KEYGEN_SHAPES = [(n, c) for n in K.F_SETS for c in (1, 3, 67)] + [(n, 2) for n in K.S_SETS]
VERIFY_SHAPES = [(n, c) for n in K.F_SETS for c in (1, 3, 67)] + [(n, c) for n in K.S_SETS for c in (1, 5)]


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


@pytest.mark.parametrize("name,count", KEYGEN_SHAPES)
def test_keygen_equals_the_model_bytes(D, torch, name, count):
    """f sets at 1, 3 and 67 instances (67 chains, leaves or instances are past one wave whatever the lane mapping), s sets at 2 instances with
    distinct seeds (512 or 256 leaves: the whole LDS reduction); the workspace is all zero after the call (dev_keygen)"""
    ref = K.keys(name, 67 if name in K.F_SETS else 2)
    seeds = [ref[k][:count] for k in ("sk_seed", "sk_prf", "pk_seed")]
    assert len(set(seeds[0])) == count
    pk, sk = dev_keygen(torch, D, name, *seeds)
    assert pk == ref["pk"][:count], (name, count, [i for i in range(count) if pk[i] != ref["pk"][i]][:8])
    assert sk == ref["sk"][:count], (name, count, [i for i in range(count) if sk[i] != ref["sk"][i]][:8])


@pytest.mark.parametrize("name,count", VERIFY_SHAPES)
def test_verify_of_honest_signatures(D, torch, fixture, name, count):
    """The T_k input of SLH-DSA-SHA2-128s fills its fourth block to the byte (22 + 14 * 16 + 9 = 255 of 256): the 128s cases here are what covers
    that edge, and must not be dropped to save time."""
    pks, msgs, sigs = K.tiled(name, count)
    want = [int(K.expect(name, p, m, s)) for p, m, s in zip(pks, msgs, sigs)]
    assert want == [1] * count
    assert dev_verify(torch, D, name, pks, msgs, sigs) == want, (name, count, "a key per instance")
    pk, msg, sig = fixture["signed"][name][0]                              # one key for all: every instance under the first key
    assert dev_verify(torch, D, name, pk, [msg] * count, [sig] * count) == [1] * count, (name, count, "pk_stride = 0")
    if count > 1 and K.distinct(name) > 1:
        # the signature of instance 0 under the key of instance 1: every byte is well formed, the root differs
        swapped = [pks[1]] + list(pks[1:])
        want = [int(K.expect(name, p, m, s)) for p, m, s in zip(swapped, msgs, sigs)]
        assert want[0] == 0 and dev_verify(torch, D, name, swapped, msgs, sigs) == want


@pytest.mark.parametrize("name", K.EDGE_SETS)
def test_message_lengths_around_the_padding_edges_of_h_msg(D, torch, fixture, name):
    """pad fits / pad spills / exact block / empty: 3 n + len = 55, 56, 64 on SHA2-128f (SHA-256; m = 34, two MGF1 counters), 111, 112, 128 on
    SHA2-256f (SHA-512); each in a batch with a flipped R and a flipped last message byte"""
    n = M.PARAMS[name].n
    lens = K.edge_lens(name)
    assert [3 * n + ln for ln in lens[:3]] == ([55, 56, 64] if n == 16 else [111, 112, 128]) and lens[3] == 0
    for ln in lens:
        pk, msg, sig = fixture["edge"][name][ln]
        assert len(msg) == ln and K.expect(name, pk, msg, sig)
        batch = [(pk, msg, sig), (pk, msg, K.flip(sig, 0)), (pk, msg, sig)]
        if ln:
            batch.append((pk, K.flip(msg, ln - 1, 7), sig))                # the last byte of the message, next to the padding
        want = [int(K.expect(name, *b)) for b in batch]
        assert want == [1, 0, 1] + [0] * (len(batch) - 3)
        assert dev_verify(torch, D, name, [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]) == want, (name, ln)
        assert dev_verify(torch, D, name, pk, [b[1] for b in batch], [b[2] for b in batch]) == want, (name, ln, "pk_stride = 0")


def _mixed_batch(name, count):
    """instance i: untouched when i % 8 == 1, else one flipped bit at the next of the positions: R, every FORS tree's secret value and path, every
    layer's WOTS part and path, PK.seed, PK.root, the message"""
    s = M.PARAMS[name]
    kinds = [("sig", what, pos) for what, pos in K.region_positions(name)] + [("pk", "PK.seed", 5), ("pk", "PK.root", s.n + 2), ("msg", "M", 7)]
    pks, msgs, sigs = K.tiled(name, count)
    batch, used, t = [], set(), 0
    for i in range(count):
        pk, msg, sig = pks[i], msgs[i], sigs[i]
        if i % 8 != 1:
            where, what, pos = kinds[t % len(kinds)]
            t += 1
            used.add(what)
            bit = i % 8
            if where == "sig":
                sig = K.flip(sig, pos, bit)
            elif where == "pk":
                pk = K.flip(pk, pos, bit)
            else:
                msg = K.flip(msg, pos, bit)
        batch.append((pk, msg, sig))
    assert used == {k[1] for k in kinds} and len(kinds) == 1 + 2 * s.k + 2 * s.d + 3
    return batch


@pytest.mark.parametrize("name", [F128, F192])
def test_mixed_batches_share_waves_between_valid_and_tampered_instances(D, torch, name):
    count = 131
    batch = _mixed_batch(name, count)
    want = [int(K.expect(name, *b)) for b in batch]
    assert want == [1 if i % 8 == 1 else 0 for i in range(count)]
    for lo in range(0, count, 64):
        assert {0, 1} <= set(want[lo:lo + 64]), lo                         # both verdicts in every wave-sized group
    ok = dev_verify(torch, D, name, [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch])
    assert ok == want, [(i, ok[i], want[i]) for i in range(count) if ok[i] != want[i]][:8]


def test_256f_has_67_chains_and_a_64_bit_idx_tree(D, torch, fixture):
    name = F256
    s = M.PARAMS[name]
    assert M.wots_len(name)[2] == 67 and s.h - s.hp == 64
    reg = M.regions(name)
    batch = list(fixture["signed"][name])
    assert all(K.expect(name, *b) for b in batch)
    pk, msg, sig = batch[0]
    for layer in (0, s.d - 1):
        for ch in (64, 65, 66):
            batch.append((pk, msg, K.flip(sig, reg["wots"][layer][0] + ch * s.n + (ch % s.n), ch % 8)))
    full = K.full_tree_signed()                                            # idx_tree with its top bit set: all 64 bits of the tree address
    n = s.n
    digest = M.Scheme(name).f.h_msg(full[2][:n], full[0][:n], full[0][n:], full[1])
    assert M.split_digest(name, digest)[1] >> 63 == 1
    batch += [full, (full[0], full[1], K.flip(full[2], reg["auth"][s.d - 1][0] + 1, 3))]
    want = [int(K.expect(name, *b)) for b in batch[:9]]
    assert want == [1, 1, 1] + [0] * 6
    assert dev_verify(torch, D, name, [b[0] for b in batch[:9]], [b[1] for b in batch[:9]], [b[2] for b in batch[:9]]) == want
    want = [int(K.expect(name, *b)) for b in batch[9:]]                    # another message length: a call of its own
    assert want == [1, 0]
    assert dev_verify(torch, D, name, [b[0] for b in batch[9:]], [b[1] for b in batch[9:]], [b[2] for b in batch[9:]]) == want


def test_on_a_stream_behind_the_kernel_that_produces_the_inputs(D, torch, fixture):
    name, count = F128, 3
    ref = K.keys(name, 3)
    pks, msgs, sigs = K.tiled(name, count)
    assert pks == ref["pk"]
    sz = M.sizes(name)
    masked = [bytes(b ^ 0x3C for b in b"".join(ref[k])) for k in ("sk_seed", "sk_prf", "pk_seed")]
    src = [_put(torch, [m], 0)[0] for m in masked]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        seeds = [torch.bitwise_xor(x, 0x3C) for x in src]                  # the seeds exist only once these kernels have run on st
        bpk, ppk = _out(torch, count * sz["pk"])
        bsk, psk = _out(torch, count * sz["sk"])
        sc = Scratch(torch, D, name, count, "keygen")
        D.keygen_dev(name, count, seeds[0].data_ptr(), seeds[1].data_ptr(), seeds[2].data_ptr(), ppk, psk, sc.ptr, sc.bytes, stream=st.cuda_stream)
        bm, pm = _put(torch, msgs)
        bs, ps = _put(torch, sigs)
        bok, pok = _out(torch, count)
        sc2 = Scratch(torch, D, name, count, "verify")
        D.verify_dev(name, count, ppk, pm, K.MSG_LEN, ps, pok, sc2.ptr, sc2.bytes, stream=st.cuda_stream)      # reads the pk the call before it writes
    st.synchronize()
    assert _take(torch, bpk, count * sz["pk"], sz["pk"], "pk") == ref["pk"]
    assert _take(torch, bsk, count * sz["sk"], sz["sk"], "sk") == ref["sk"]
    assert [b[0] for b in _take(torch, bok, count, 1, "ok")] == [1] * count
    sc.check("stream", cleared=True)
    sc2.check("stream", cleared=False)
    del bm, bs


def test_host_forms_equal_the_device_forms(D, torch, fixture):
    name, count = F128, 3
    ref = K.keys(name, 3)
    assert D.keygen_internal(name, ref["sk_seed"], ref["sk_prf"], ref["pk_seed"]) == list(zip(ref["pk"], ref["sk"]))
    assert dev_keygen(torch, D, name, ref["sk_seed"], ref["sk_prf"], ref["pk_seed"]) == (ref["pk"], ref["sk"])
    pks, msgs, sigs = K.tiled(name, count)
    pos = M.regions(name)["wots"][3][0] + 9
    sigs = [sigs[0], K.flip(sigs[1], pos, 2), sigs[2]]
    want = [bool(K.expect(name, p, m, s)) for p, m, s in zip(pks, msgs, sigs)]
    assert want == [True, False, True]
    assert D.verify_internal(name, pks, msgs, sigs) == want == [bool(o) for o in dev_verify(torch, D, name, pks, msgs, sigs)]
    pk, msg, sig = fixture["signed"][name][0]
    assert D.verify_internal(name, pk, [msg] * 3, [sig, K.flip(sig, 0), sig]) == [True, False, True]
    pk0, m0, s0 = fixture["edge"][name][0]                                 # the empty message: no message pointer at all
    assert D.verify_internal(name, pk0, [m0], [s0]) == [True]
    pairs = D.keygen(name, 2)                                              # fresh randomness, so only consistency with the model is checked
    assert pairs[0] != pairs[1]
    for pk, sk in pairs:
        n = len(pk) // 2
        assert M.keygen_internal(name, sk[:n], sk[n:2 * n], sk[2 * n:3 * n]) == (sk, pk)
        assert D.verify(name, pk, b"message", M.sign(name, b"message", b"", sk))


def test_algorithm_24_with_a_context(D, fixture):
    name = K.CTX_SET
    assert sorted(fixture["ctx"]) == [0, 1, 255]
    for ln, (pk, msg, ctx, sig) in fixture["ctx"].items():
        assert len(ctx) == ln and M.verify(name, msg, sig, ctx, pk)
        assert D.verify(name, pk, msg, sig, ctx=ctx) is True
        others = [(msg, ctx + b"x" if ln < 255 else ctx[:-1]), (msg + b"!", ctx)] + ([(msg, bytes(ln))] if bytes(ln) != ctx else [])
        for m2, c2 in others:
            assert D.verify(name, pk, m2, sig, ctx=c2) == M.verify(name, m2, sig, c2, pk) is False
    pk, msg, ctx, sig = fixture["ctx"][0]
    with pytest.raises(ValueError):
        D.verify(name, pk, msg, sig, ctx=bytes(256))
