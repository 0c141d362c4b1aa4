"""SLH-DSA on the MI355X at the smallest batch in which one array that a single kernel addresses passes 2^32 bytes: the signatures of 256f (49 856
bytes each) read by Verify in both hash families and written by signing, at 86 152 instances; the chain ends of 192s in KeyGen (512 leaves of 51 chains
of 24 bytes per instance), at 6 857, in both families; and the chain ends of SHAKE-192s signing (7 layers of them), at 983.  An index computed in 32
bits anywhere below the entry points would wrap there; the largest batch that checks bytes elsewhere in the suite is 513 instances.

Instance i is instance i mod 3 of a short period of the model's.  3 divides neither the batch, 64 nor 256, and 2^32 bytes is not a whole number of
periods of the array, so an instance read or written at a wrapped index does not meet bytes equal to its own.  Inputs and expected outputs are tiled
on the device from the period; every byte of every instance is compared there, and the guard bytes and the workspace are checked there too: nothing of
the batch's size is copied to the host.  Each test frees what it allocated.

The three model KeyGens of 192s that the KeyGen tests compare with (K.keys(name, 3)) cost about 2.5 s per family on the CPU, once per process."""
import random

import pytest

from tests.helpers import slhdsa_edge_cases as E
from tests.helpers import slhdsa_sign_cases as S
from tests.helpers.mlkem_gpu import _out, _put_dev, _take_dev
from tests.helpers.slhdsa_gpu import Scratch, dev_verify_rows, release, rows, same_rows, tile
from tests.helpers.slhdsa_sign_gpu import SignScratch

pytestmark = pytest.mark.gpu

FAMS = sorted(E.FAMILIES)
PERIOD = 3
SIG_256F, ENDS_192S = 49856, 512 * 51 * 24
VERIFY_COUNT, KEYGEN_COUNT, SIGN_COUNT = 86152, 6857, 983


@pytest.fixture(scope="module")
def libs():
    import tools_amd
    return {"SHAKE": tools_amd.slhdsa, "SHA2": tools_amd.slhdsa_sha2}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def crossing(count, per_instance, period=PERIOD):
    """`count` is the smallest batch at which an array of `per_instance` bytes per instance reaches 2^32 bytes, plus the smallest addend >= 3 that
    leaves it divisible by neither the period, 64 nor 256; and 2^32 is not a whole number of periods of the array.  Returns the instance that holds
    byte 2^32 - 1 and byte 2^32."""
    least = -(-2 ** 32 // per_instance)
    assert per_instance * least >= 2 ** 32 > per_instance * (least - 1)
    ragged = [c for c in range(least + 3, least + 300) if c % period and c % 64 and c % 256]
    assert count == ragged[0]
    assert (2 ** 32) % (per_instance * period) != 0 and (2 ** 32) % per_instance != 0
    straddles = 2 ** 32 // per_instance
    assert straddles * per_instance < 2 ** 32 < (straddles + 1) * per_instance and straddles == least - 1
    return straddles


def pad256(b):
    return (b + 255) // 256 * 256


def room(torch, need, rest):
    free, _ = torch.cuda.mem_get_info()
    if free < need + rest + 2 ** 30:
        pytest.skip(f"{free} bytes of device memory are free; the test needs its workspace of {need} bytes, {rest} bytes of inputs and outputs, and {2 ** 30}")


@pytest.mark.parametrize("tag", FAMS)
def test_verify_with_the_signatures_at_4_gib(libs, torch, tag):
    """k_vf_fors, k_vf_wots and k_vf_xmss form c * sig_len: the fixture's three (pk, M, SIG) of 256f tiled, with instance 0, the last and the one whose
    signature holds byte 2^32 tampered (the model rejects each) and every other accepted"""
    fam, D = E.FAMILIES[tag], libs[tag]
    name, count = fam.name("256f"), VERIFY_COUNT
    sz, s = fam.M.sizes(name), fam.M.PARAMS[name]
    assert sz["sig"] == SIG_256F
    straddles = crossing(count, SIG_256F)
    need = D.workspace_bytes(name, count, "verify")
    ln = fam.M.wots_len(name)[2]
    assert need == sum(pad256(count * b) for b in (64, s.k * s.n, 32, ln * s.n))       # digest, FORS roots, node, chain ends: the library's sections
    room(torch, need, count * (SIG_256F + sz["pk"] + fam.K.MSG_LEN + 2 + 16))
    triples = fam.K.signed(name)
    assert len(triples) == PERIOD and all(fam.K.expect(name, *t) for t in triples)
    reg = fam.M.regions(name)
    hits = {0: reg["R"][0] + 1, straddles: reg["wots"][s.d - 1][1] - 1, count - 1: SIG_256F - 1}      # R, the last chain value's last byte, the top node's
    for i, pos in hits.items():
        pk, msg, sig = triples[i % PERIOD]
        assert fam.K.expect(name, pk, msg, E.flip(sig, pos, i % 8)) is False
    try:
        sigs = tile(torch, rows(torch, [t[2] for t in triples]), count)
        for i, pos in hits.items():
            sigs[i, pos] ^= 1 << (i % 8)
        want = torch.ones(count, dtype=torch.uint8, device="cuda")
        want[list(hits)] = 0
        ok = dev_verify_rows(torch, D, name, tile(torch, rows(torch, [t[0] for t in triples]), count), tile(torch, rows(torch, [t[1] for t in triples]), count), sigs)
        ne = (ok != want).nonzero().flatten()
        assert ne.numel() == 0, (name, int(ne.numel()), "instances differ; the first:", ne[:8].tolist(), "straddling:", straddles)
    finally:
        sigs = want = ok = ne = None
        release(torch)


@pytest.mark.parametrize("tag", FAMS)
def test_keygen_with_the_chain_ends_at_4_gib(libs, torch, tag):
    """k_kg_chains writes and k_kg_leaf reads 512 * 51 chain ends per instance of 192s (NW = 3 / NQ = 6)"""
    fam, D = E.FAMILIES[tag], libs[tag]
    name, count = fam.name("192s"), KEYGEN_COUNT
    sz, s = fam.M.sizes(name), fam.M.PARAMS[name]
    assert (1 << s.hp) * fam.M.wots_len(name)[2] * s.n == ENDS_192S
    crossing(count, ENDS_192S)
    need = D.workspace_bytes(name, count, "keygen")
    assert need == pad256(count * ENDS_192S) + pad256(count * (1 << s.hp) * s.n)        # chain ends, leaves: the library's sections
    room(torch, need, count * (sz["pk"] + sz["sk"] + 3 * s.n))
    ref = fam.K.keys(name, PERIOD)
    assert len(set(ref["pk"])) == PERIOD
    try:
        seeds = [_put_dev(torch, tile(torch, rows(torch, ref[k]), count), 0) for k in ("sk_seed", "sk_prf", "pk_seed")]
        bpk, ppk = _out(torch, count * sz["pk"], 0)
        bsk, psk = _out(torch, count * sz["sk"], 0)
        sc = Scratch(torch, D, name, count, "keygen")
        torch.cuda.synchronize()
        D.keygen_dev(name, count, seeds[0][1], seeds[1][1], seeds[2][1], ppk, psk, sc.ptr, sc.bytes)
        pk = _take_dev(torch, bpk, count * sz["pk"], sz["pk"], "pk", 0)
        sk = _take_dev(torch, bsk, count * sz["sk"], sz["sk"], "sk", 0)
        same_rows(torch, pk, rows(torch, ref["pk"]), (name, "pk"))
        same_rows(torch, sk, rows(torch, ref["sk"]), (name, "sk"))
        sc.check((name, count, "keygen"), cleared=True)
    finally:
        seeds = bpk = bsk = sc = pk = sk = None
        release(torch)


def sign_rows(torch, D, name, count, period):
    """sign_dev over `count` instances, instance i the (sk, M, addrnd) of period[i mod 3], a key per instance; the guards and the workspace are checked on
    the device; returns the signatures as a (count, size) device tensor and what keeps it alive"""
    size = S.M.sizes(name)["sig"]
    bk, pk = _put_dev(torch, tile(torch, rows(torch, [p[0] for p in period]), count), 0)
    bm, pm = _put_dev(torch, tile(torch, rows(torch, [p[1] for p in period]), count), 0)
    br, pr = _put_dev(torch, tile(torch, rows(torch, [p[2] for p in period]), count), 0)
    bs, ps = _out(torch, count * size, 0)
    sc = SignScratch(torch, D, name, count)
    torch.cuda.synchronize()
    D.sign_dev(name, count, pk, pm, len(period[0][1]), pr, ps, sc.ptr, sc.bytes)
    sig = _take_dev(torch, bs, count * size, size, (name, count, "sig"), 0)
    sc.check((name, count, "sign"))
    del bk, bm, br
    return sig, bs


def sign_sections(s, ln, count):
    """the workspace sections of psf_slhdsa_sign.hip in order, in bytes: digest, FORS subtree roots (a > 9), FORS roots, layer messages, chain ends, leaves"""
    leaves = 1 << s.hp
    return [count * 64, count * (s.k << (s.a - 9)) * s.n if s.a > 9 else 0, count * s.k * s.n, count * s.d * 32, count * s.d * leaves * ln * s.n, count * s.d * leaves * s.n]


def test_sign_with_the_chain_ends_at_4_gib(libs, torch):
    """k_sg_chains writes and k_sg_leaf reads d = 7 layers of chain ends per instance of SHAKE-192s.  The period is three (sk, M, addrnd) over the two
    keys of the fixture; every instance is compared on the device with instance i mod 3, and the model checks by parts instances 0, 1, 2, the last three
    and the one whose chain ends hold byte 2^32: no model signature of an s set is made"""
    fam, D = E.SHAKE, libs["SHAKE"]
    name, count = fam.name("192s"), SIGN_COUNT
    s, sz, ln = fam.M.PARAMS[name], fam.M.sizes(name), fam.M.wots_len(name)[2]
    straddles = crossing(count, s.d * ENDS_192S)
    need = D.sign_workspace_bytes(name, count)
    secs = sign_sections(s, ln, count)
    assert need == sum(pad256(b) for b in secs) and secs[4] == count * s.d * ENDS_192S == max(secs)
    room(torch, need, count * (sz["sig"] + sz["sk"] + fam.K.MSG_LEN + s.n))
    ks = fam.K.keys(name, 2)
    rng = random.Random(983)
    period = [(ks["sk"][j % 2], rng.randbytes(fam.K.MSG_LEN), rng.randbytes(s.n)) for j in range(PERIOD)]
    try:
        sig, keep = sign_rows(torch, D, name, count, period)
        same_rows(torch, sig, sig[:PERIOD].clone(), (name, "every instance against instance i mod 3"))
        for i in sorted({0, 1, 2, straddles, count - 3, count - 2, count - 1}):
            sk, msg, rnd = period[i % PERIOD]
            assert S.exact_by_parts(name, sk, msg, rnd, bytes(sig[i].cpu().numpy())) is None, (name, i)
    finally:
        sig = keep = None
        release(torch)


def test_sign_with_the_signatures_at_4_gib(libs, torch):
    """k_sg_prf_msg, k_sg_fors, k_sg_tree and k_sg_wots write at c * sig_len: SHAKE-256f, the hedged fixture tiled, bytes equal to the model's; the
    workspace is about 51 GB"""
    fam, D = E.SHAKE, libs["SHAKE"]
    name, count = fam.name("256f"), VERIFY_COUNT
    s, sz, ln = fam.M.PARAMS[name], fam.M.sizes(name), fam.M.wots_len(name)[2]
    crossing(count, SIG_256F)
    need = D.sign_workspace_bytes(name, count)
    assert sz["sig"] == SIG_256F and need == sum(pad256(b) for b in sign_sections(s, ln, count))
    room(torch, need, count * (SIG_256F + sz["sk"] + fam.K.MSG_LEN + s.n) + PERIOD * 2048 * SIG_256F * 2)
    t = S.hedged(name)
    assert len(t) == PERIOD
    try:
        sig, keep = sign_rows(torch, D, name, count, [r[:3] for r in t])
        same_rows(torch, sig, rows(torch, [r[3] for r in t]), (name, "sig"))
    finally:
        sig = keep = None
        release(torch)
