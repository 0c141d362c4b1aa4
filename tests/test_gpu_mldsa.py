"""Batched ML-DSA on the MI355X (tools_amd/mldsa.py, psf_mldsa_*) against the pure-Python model of tests/helpers/mldsa_model.py: KeyGen_internal byte
for byte, Verify_internal of honest signatures (message lengths on both sides of a SHAKE256 block edge, mu given, one key per instance and one key for
all), mixed batches with tampered instances inside one wave, the malformed hints, the norm bound at its edge, a stream, the host forms and
Algorithm 3.  Every comparison is exact equality over every instance; every output sits between guard bytes at a pointer one byte past an aligned
address; after KeyGen the workspace is all zero, and the sampler flag is what it was.  The harness is tests/helpers/mldsa_gpu.py."""
import random

import pytest

from tests.helpers import mldsa_model as M
from tests.helpers.mldsa_gpu import (DISTINCT, NAMES, Scratch, _out, _put, _take, dev_keygen, dev_verify, flip, keys, layout, mu_of, tiled, triples, why_of,
                                     with_hint, with_z_coefficient)
from tests.test_mldsa_core_cpu import malformed_hints

pytestmark = pytest.mark.gpu

SHAPES = [(n, c) for c in (1, 3) for n in NAMES] + [("ML-DSA-44", 67)]
MSG_LENS = (0, 1, 135, 136, 200, 71, 72)                                  # tr || M' is 64 bytes longer: 71 and 72 are the two sides of its first block edge
HINT, NORM, HASH = M.HINT, M.NORM, M.HASH
MU = 1


@pytest.fixture(scope="module")
def D():
    import tools_amd
    return tools_amd.mldsa


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.mark.parametrize("name,count", SHAPES)
def test_keygen_equals_the_model_bytes(D, torch, name, count):
    ref = keys(name, count)
    pk, sk, _ = dev_keygen(torch, D, name, ref["xi"], flag=0)
    assert pk == ref["pk"], (name, count, [i for i in range(count) if pk[i] != ref["pk"][i]][:8])
    assert sk == ref["sk"], (name, count, [i for i in range(count) if sk[i] != ref["sk"][i]][:8])
    pk2, sk2, _ = dev_keygen(torch, D, name, ref["xi"], flag=4)            # a flag that is already raised stays as it is
    assert pk2 == ref["pk"] and sk2 == ref["sk"]


@pytest.mark.parametrize("name,count", SHAPES)
def test_verify_of_honest_signatures(D, torch, name, count):
    for msg_len in MSG_LENS:
        pks, msgs, sigs = tiled(name, count, msg_len)
        assert dev_verify(torch, D, name, pks, msgs, sigs) == ([1] * count, [0] * count), (name, count, msg_len)
    pks, msgs, sigs = tiled(name, count, 136)
    mus = [mu_of(p, m) for p, m in zip(pks, msgs)]
    assert dev_verify(torch, D, name, pks, mus, sigs, msg_kind=MU, flag=4) == ([1] * count, [0] * count), (name, count, "mu")
    assert dev_verify(torch, D, name, pks, msgs, sigs, with_why=False)[0] == [1] * count
    # one key for all instances
    pks, msgs, sigs = tiled(name, count, 135, one_key=True)
    assert dev_verify(torch, D, name, pks[0], msgs, sigs) == ([1] * count, [0] * count), (name, count, "one key")
    assert dev_verify(torch, D, name, pks[0], [mu_of(pks[0], m) for m in msgs], sigs, msg_kind=MU) == ([1] * count, [0] * count), (name, count, "one key, mu")
    if count > 1:
        # the signature of instance 0 under the key of instance 1: every byte is well formed, the hash differs
        pks, msgs, sigs = tiled(name, count, 1)
        swapped = [pks[1]] + list(pks[1:])
        want = [why_of(name, p, m, s) for p, m, s in zip(swapped, msgs, sigs)]
        assert want[0] == HASH
        assert dev_verify(torch, D, name, swapped, msgs, sigs)[1] == want


def _tamper(name, kind, i, pk, msg, sig):
    lay, bit = layout(name), i % 8
    cb = M.PARAMS[name][4]
    if kind == 0:
        return pk, msg, flip(sig, 0, bit)                                  # first byte of c~
    if kind == 1:
        return pk, msg, flip(sig, cb - 1, bit)                             # last byte of c~
    if kind == 2:
        return pk, msg, flip(sig, lay["z"], bit)                           # first byte of z
    if kind == 3:
        return pk, msg, flip(sig, lay["hint"] - 1, bit)                    # last byte of z
    if kind == 4:
        return pk, msg, flip(sig, lay["hint"] + i % (len(sig) - lay["hint"]), bit)      # a hint byte
    if kind == 5:
        return flip(pk, i % 32, bit), msg, sig                             # rho
    if kind == 6:
        return flip(pk, len(pk) - 1, bit), msg, sig                        # last byte of t1
    return pk, flip(msg, i % len(msg), bit), sig                           # the message


@pytest.mark.parametrize("count", [67, 259])
def test_mixed_batches_share_waves_between_valid_and_tampered_instances(D, torch, count):
    name = "ML-DSA-44"
    pks, msgs, sigs = tiled(name, count, 200)
    tampered = {0, 5, 63, 64, 66}
    for chosen in (tampered, set(range(count)) - tampered):
        inst = []
        for n, i in enumerate(sorted(chosen)):
            inst.append((i, n % 8))
        kind = dict(inst)
        batch = [_tamper(name, kind[i], i, pks[i], msgs[i], sigs[i]) if i in chosen else (pks[i], msgs[i], sigs[i]) for i in range(count)]
        if len(chosen) > 8:
            assert set(kind.values()) == set(range(8))
        want = [why_of(name, p, m, s) for p, m, s in batch]
        assert all((want[i] != 0) == (i in chosen) for i in range(count)), [i for i in range(count) if (want[i] != 0) != (i in chosen)]
        ok, why = dev_verify(torch, D, name, [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch])
        assert why == want, [(i, why[i], want[i]) for i in range(count) if why[i] != want[i]][:8]
        assert ok == [1 if w == 0 else 0 for w in want]
    # every kind of tampering at the five indices in turn
    for shift in range(1, 8):
        kind = {i: (n + shift) % 8 for n, i in enumerate(sorted(tampered))}
        batch = [_tamper(name, kind[i], i, pks[i], msgs[i], sigs[i]) if i in tampered else (pks[i], msgs[i], sigs[i]) for i in range(67)]
        want = [why_of(name, p, m, s) for p, m, s in batch]
        assert all((want[i] != 0) == (i in tampered) for i in range(67))
        assert dev_verify(torch, D, name, [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch])[1] == want, shift


@pytest.mark.parametrize("name", NAMES)
def test_malformed_hints(D, torch, name):
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    pk, msg, sig = triples(name, 136)[0]
    h, y, bad = malformed_hints(k, omega, random.Random(11))
    sigs = [with_hint(name, sig, b) for b in bad]
    sigs += [with_z_coefficient(name, s, 0, 0, g1 - beta) for s in sigs]   # the norm is evaluated whatever the hint says
    # indices that descend across the boundary between two polynomials are valid: not flagged HINT
    h2 = [[0] * 256 for _ in range(k)]
    h2[0][200], h2[0][250], h2[1][3], h2[1][100] = 1, 1, 1, 1
    sigs += [with_hint(name, sig, M.hint_bit_pack(h2, omega)), with_hint(name, sig, y), sig]
    want = [why_of(name, pk, msg, s) for s in sigs]
    assert want[:4] == [HINT | HASH] * 4 and want[4:8] == [HINT | HASH | NORM] * 4 and want[8] & HINT == 0 and want[9] & HINT == 0 and want[10] == 0
    n = len(sigs)
    ok, why = dev_verify(torch, D, name, [pk] * n, [msg] * n, sigs)
    assert why == want and ok == [0] * (n - 1) + [1]
    assert dev_verify(torch, D, name, pk, [msg] * n, sigs)[1] == want      # one key for all


@pytest.mark.parametrize("name", NAMES)
def test_the_norm_bound_at_its_edge(D, torch, name):
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    pk, msg, sig = triples(name, 136)[0]
    sigs, edge = [], []
    for poly, index in ((0, 0), (l - 1, 255)):
        for value in (g1 - beta, -(g1 - beta), g1 - beta - 1, -(g1 - beta - 1)):
            sigs.append(with_z_coefficient(name, sig, poly, index, value))
            edge.append(abs(value) == g1 - beta)
    want = [why_of(name, pk, msg, s) for s in sigs]
    assert [bool(w & NORM) for w in want] == edge
    n = len(sigs)
    ok, why = dev_verify(torch, D, name, [pk] * n, [msg] * n, sigs)
    assert why == want and ok == [0] * n


def test_on_a_stream_behind_the_kernel_that_produces_the_inputs(D, torch):
    name, count = "ML-DSA-44", DISTINCT
    ref = keys(name, count)
    pks, msgs, sigs = tiled(name, count, 136)
    assert pks == ref["pk"]
    sz = M.sizes(name)
    masked = bytes(b ^ 0x3C for b in b"".join(ref["xi"]))
    src = _put(torch, [masked], 0)[0]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xi_dev = torch.bitwise_xor(src, 0x3C)                              # the seeds exist only once this kernel has run on s
        bpk, ppk = _out(torch, count * sz["pk"])
        bsk, psk = _out(torch, count * sz["sk"])
        sc = Scratch(torch, D, name, count, "keygen")
        D.keygen_dev(name, count, xi_dev.data_ptr(), ppk, psk, sc.ptr, sc.bytes, d_fail=sc.flag.data_ptr(), stream=s.cuda_stream)
        bm, pm = _put(torch, msgs)
        bs, ps = _put(torch, sigs)
        bok, pok = _out(torch, count)
        bwhy, pwhy = _out(torch, count)
        sc2 = Scratch(torch, D, name, count, "verify")
        D.verify_dev(name, count, ppk, pm, 136, ps, pok, sc2.ptr, sc2.bytes, d_why=pwhy, d_fail=sc2.flag.data_ptr(), stream=s.cuda_stream)     # reads the pk the call before it writes
    s.synchronize()
    assert _take(torch, bpk, count * sz["pk"], sz["pk"], "pk") == ref["pk"]
    assert _take(torch, bsk, count * sz["sk"], sz["sk"], "sk") == ref["sk"]
    assert [b[0] for b in _take(torch, bok, count, 1, "ok")] == [1] * count
    assert [b[0] for b in _take(torch, bwhy, count, 1, "why")] == [0] * count
    sc.check("stream", cleared=True)
    sc2.check("stream", cleared=False)
    del bm, bs


@pytest.mark.parametrize("name", NAMES)
def test_host_forms_equal_the_device_forms(D, torch, name):
    ref = keys(name, DISTINCT)
    assert D.keygen_internal(name, ref["xi"]) == list(zip(ref["pk"], ref["sk"]))
    pks, msgs, sigs = tiled(name, 4, 200)
    lay = layout(name)
    sigs = [sigs[0], flip(sigs[1], lay["z"] + 5, 2), sigs[2], with_hint(name, sigs[3], bytes([1, 1]) + bytes(len(sigs[3]) - lay["hint"] - 2))]
    want = [why_of(name, p, m, s) for p, m, s in zip(pks, msgs, sigs)]
    assert want[0] == 0 and want[2] == 0 and want[1] != 0 and want[3] & HINT
    dev = dev_verify(torch, D, name, pks, msgs, sigs)
    assert D.verify_internal(name, pks, msgs, sigs, why=True) == [(w == 0, w) for w in want] == [(bool(o), w) for o, w in zip(*dev)]
    assert D.verify_internal(name, pks, msgs, sigs) == [w == 0 for w in want]
    pks1, msgs1, sigs1 = tiled(name, 3, 135, one_key=True)
    assert D.verify_internal(name, pks1[0], msgs1, sigs1) == [True] * 3
    assert D.verify_internal(name, pks1[0], [mu_of(pks1[0], m) for m in msgs1], sigs1, msg_kind=MU) == [True] * 3
    pairs = D.keygen(name, 2)                                              # fresh randomness, so only consistency is checked
    assert pairs[0] != pairs[1]
    for pk, sk in pairs:
        assert sk[:32] == pk[:32] and sk[64:128] == M.H(pk, 64)
        assert D.verify(name, pk, b"message", M.sign(sk, b"message", b"", bytes(32), name))


@pytest.mark.parametrize("name", NAMES)
def test_algorithm_3_with_a_context(D, name):
    ref = keys(name, DISTINCT)
    pk, sk = ref["pk"][0], ref["sk"][0]
    msg, ctx = b"the message of algorithm three", b"a context string"
    sig = M.sign(sk, msg, ctx, bytes(range(32)), name)
    assert M.verify(pk, msg, sig, ctx, name)
    assert D.verify(name, pk, msg, sig, ctx=ctx) is True
    for m2, c2 in ((msg, b""), (msg, b"a context strinh"), (msg + b"!", ctx)):
        assert D.verify(name, pk, m2, sig, ctx=c2) == M.verify(pk, m2, sig, c2, name) is False
    assert D.verify(name, pk, msg, sig, ctx=bytes(256)) is False


@pytest.mark.parametrize("name", NAMES)
def test_expand_a_writes_the_images_of_the_two_step_form(D, torch, name):
    """verification leaves its workspace as it is, and the header states its layout (tr | mu | why words | hint masks | images of A_hat | ..., each
    section rounded up to 256 bytes): the images ExpandA wrote there directly equal image_from(sample_ntt(rho)) of the public stages"""
    import numpy as np
    import tools_amd
    F = tools_amd.fips204
    k, l = M.PARAMS[name][:2]
    count = DISTINCT
    pks, msgs, sigs = tiled(name, count, 136)
    sz = M.sizes(name)
    (bp, pp), (bm, pm), (bs, ps) = _put(torch, pks), _put(torch, msgs), _put(torch, sigs)
    bok, pok = _out(torch, count)
    sc = Scratch(torch, D, name, count, "verify")
    D.verify_dev(name, count, pp, pm, 136, ps, pok, sc.ptr, sc.bytes)
    torch.cuda.synchronize()

    def up(n):
        return (n + 255) // 256 * 256
    at = (sc.ptr - sc.ws.data_ptr()) + up(64 * count) + up(64 * count) + up(4 * count) + up(32 * k * count)
    got = sc.ws[at:at + count * k * l * 1024].cpu().numpy().view(np.uint32).reshape(count, k, l, 256)
    rhos = np.frombuffer(b"".join(p[:32] for p in pks), np.uint8).reshape(count, 32)
    want = F.image_from_fips204(F.sample_ntt(rhos, k=k, l=l))
    assert (got == want).all()
    del bp, bm, bs, bok
