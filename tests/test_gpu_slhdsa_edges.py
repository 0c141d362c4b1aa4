"""SLH-DSA on the MI355X, both hash families (psf_slhdsa.hip and psf_slhdsa_sign.hip for SHAKE: KeyGen, Sign, Verify; psf_slhdsa_sha2.hip for SHA-2:
KeyGen, Verify), where the rest of the suite does not look, against the pure-Python models byte for byte and over every instance.

Alignment.  The units read and write by bytes (load_words, load_be, Cat3Reader, store_words), which the compiler may merge into wide accesses;
tests/test_gpu_slhdsa*.py put every buffer one byte past a 16-byte boundary ("all1").  Here every buffer sits at 0, 4 and 8, and the inputs and the
outputs at different alignments.

Strides.  Keys and messages at a pitch above their size, one that is and one that is not a multiple of 8, from aligned base pointers so that the pitch
alone decides; each alone and combined, every padded case twice with different bytes in the gaps; the deterministic variant too, whose opt_rand is
PK.seed read out of the padded keys.

Workgroup edges.  The per-instance kernels run 256 lanes per workgroup: 255, 256, 257 and 513 instances.

Positions and values.  The tables of tests/helpers/slhdsa_edge_cases.py, pinned to the models by tests/test_slhdsa_edge_cases_cpu.py: digests with
idx_leaf, the top bit of idx_tree and the FORS indices at their edges; signatures, a public key and secret keys of all 0x00 / 0xFF; a flipped bit in
every byte of a signature of every parameter set.

Every call keeps the checks of the harness (tests/helpers/slhdsa_gpu.py, slhdsa_sha2_gpu.py, slhdsa_sign_gpu.py): guard bytes around every output,
nothing written outside the workspace, the workspace all zero after KeyGen and after signing."""
import pytest

from tests.helpers import slhdsa_edge_cases as E
from tests.helpers import slhdsa_gpu as G
from tests.helpers import slhdsa_sha2_gpu as G2
from tests.helpers import slhdsa_sign_cases as S
from tests.helpers.slhdsa_gpu import dev_verify_rows, offsets, release, rows
from tests.helpers.slhdsa_sign_gpu import dev_sign

pytestmark = pytest.mark.gpu

FAMS = sorted(E.FAMILIES)
PATTERNS = {"all0": offsets(0, 0), "all4": offsets(4, 4), "all8": offsets(8, 8), "in0_out1": offsets(0, 1), "in1_out0": offsets(1, 0)}
SHAPES = [("128f", 67), ("192f", 3), ("256f", 3)]
STRIDE_SHAPES = [("128f", 67), ("256f", 3)]
PADS = [(k, m) for k in (0, 5, 8) for m in (0, 3, 8) if k or m]
GAPS = (0xC3, 0x11)
SETS = [(tag, short) for tag in FAMS for short in E.SHORT]


@pytest.fixture(scope="module")
def libs():
    import tools_amd
    return {"SHAKE": tools_amd.slhdsa, "SHA2": tools_amd.slhdsa_sha2}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def harness(tag):
    return G if tag == "SHAKE" else G2


def differing(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


def expected(fam, name, pks, msgs, sigs):
    return [int(fam.K.expect(name, p, m, s)) for p, m, s in zip(pks, msgs, sigs)]


def tampered(fam, name, count, at):
    """the tiled fixture with instance at[i] flipped in the i-th of four regions: R, the last FORS secret value, the last layer's WOTS part, the first
    layer's path; (pks, msgs, sigs, want) with `want` the model's verdicts"""
    pks, msgs, sigs = fam.K.tiled(name, count)
    pos = dict(fam.K.region_positions(name))
    s = fam.M.PARAMS[name]
    where = [pos["R"], pos[f"fors_sk{s.k - 1}"], pos[f"wots{s.d - 1}"], pos["auth0"]]
    hit = sorted({i for i in at if i < count})
    for t, i in enumerate(hit):
        sigs[i] = E.flip(sigs[i], where[t % 4], i % 8)
    want = expected(fam, name, pks, msgs, sigs)
    assert want == [0 if i in hit else 1 for i in range(count)]
    return pks, msgs, sigs, want


# ---- alignment -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("short,count", SHAPES)
@pytest.mark.parametrize("tag", FAMS)
def test_keygen_sign_and_verify_equal_the_model_at_every_alignment(libs, torch, tag, short, count, pattern):
    """KeyGen against the model's keys; on SHAKE the hedged fixture signed again, byte for byte; Verify of the device's signatures and the fixture's
    with one tampered instance, a key per instance and one key for all; then the message lengths around H_msg's block edge and the empty message"""
    fam, D, H, offs = E.FAMILIES[tag], libs[tag], harness(tag), PATTERNS[pattern]
    name = fam.name(short)
    what = (name, count, pattern)
    ref = fam.K.keys(name, 67)
    pk, sk = H.dev_keygen(torch, D, name, *[ref[k][:count] for k in ("sk_seed", "sk_prf", "pk_seed")], offs=offs)
    assert pk == ref["pk"][:count], (what, differing(pk, ref["pk"]))
    assert sk == ref["sk"][:count], (what, differing(sk, ref["sk"]))
    pks, msgs, sigs, want = tampered(fam, name, count, [1])
    if tag == "SHAKE":
        t = S.hedged(name)
        inst = [t[i % len(t)] for i in range(count)]
        got = dev_sign(torch, D, name, [r[0] for r in inst], [r[1] for r in inst], [r[2] for r in inst], offs=offs)
        assert got == [r[3] for r in inst] == fam.K.tiled(name, count)[2], (what, differing(got, [r[3] for r in inst]))
        assert H.dev_verify(torch, D, name, pks, msgs, got, offs=offs) == [1] * count, (what, "the device's own signatures")
        sk0, m0, r0, s0 = t[0]
        got = dev_sign(torch, D, name, sk0, [m0] * count, [r0] * count, offs=offs)
        assert got == [s0] * count, (what, "sk_stride = 0", differing(got, [s0] * count))
    ok = H.dev_verify(torch, D, name, pks, msgs, sigs, offs=offs)
    assert ok == want, (what, "a key per instance", differing(ok, want))
    one = [sigs[0] if i != 1 else E.flip(sigs[0], len(sigs[0]) - 1, 7) for i in range(count)]
    want1 = expected(fam, name, [pks[0]] * count, [msgs[0]] * count, one)
    assert want1 == [1 if i != 1 else 0 for i in range(count)]
    assert H.dev_verify(torch, D, name, pks[0], [msgs[0]] * count, one, offs=offs) == want1, (what, "pk_stride = 0")
    if name in fam.K.EDGE_SETS:
        first_sk = E.first_key(fam, name)[1]
        for ln, (pk1, msg, sig) in fam.K.edge_signed(name).items():
            assert len(msg) == ln and fam.K.expect(name, pk1, msg, sig)
            batch = [sig, E.flip(sig, 0), sig]
            assert H.dev_verify(torch, D, name, [pk1] * 3, [msg] * 3, batch, offs=offs) == [1, 0, 1], (what, ln)
            assert H.dev_verify(torch, D, name, pk1, [msg] * 3, batch, offs=offs) == [1, 0, 1], (what, ln, "pk_stride = 0")
            if tag == "SHAKE":
                assert dev_sign(torch, D, name, [first_sk] * 2, [msg] * 2, offs=offs) == [sig] * 2, (what, ln, "deterministic")


# ---- strides -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_pad,msg_pad", PADS)
@pytest.mark.parametrize("short,count", STRIDE_SHAPES)
@pytest.mark.parametrize("tag", FAMS)
def test_verify_with_keys_and_messages_at_a_padded_stride(libs, torch, tag, short, count, key_pad, msg_pad):
    """pk_stride = 2n + 5 or 2n + 8, msg_stride = len + 3 or len + 8, alone and combined; keys and messages differ from instance to instance, so a
    kernel that forms c * pk_stride or c * msg_stride with the packed size reads another instance's bytes or the gap"""
    fam, D, H = E.FAMILIES[tag], libs[tag], harness(tag)
    name = fam.name(short)
    sz = fam.M.sizes(name)
    pks, msgs, sigs, want = tampered(fam, name, count, [1, count - 1])
    assert len(set(pks)) == len(set(msgs)) == 3
    assert H.dev_verify(torch, D, name, pks, msgs, sigs, offs=0) == want, (name, "packed")
    pk_stride = sz["pk"] + key_pad if key_pad else None
    msg_stride = fam.K.MSG_LEN + msg_pad if msg_pad else None
    for gap in GAPS:
        ok = H.dev_verify(torch, D, name, pks, msgs, sigs, offs=0, pk_stride=pk_stride, msg_stride=msg_stride, gap=gap)
        assert ok == want, (name, count, key_pad, msg_pad, hex(gap), differing(ok, want))
    if msg_pad:                                                           # one key for all (pk_stride = 0) with the messages at a pitch
        one = expected(fam, name, [pks[0]] * count, msgs, sigs)
        assert one[0] == 1 and not any(one[1:3])
        assert H.dev_verify(torch, D, name, pks[0], msgs, sigs, offs=0, msg_stride=msg_stride) == one, (name, count, msg_pad, "pk_stride = 0")


@pytest.mark.parametrize("key_pad,msg_pad", PADS)
@pytest.mark.parametrize("short,count", STRIDE_SHAPES)
def test_sign_with_keys_and_messages_at_a_padded_stride(libs, torch, short, count, key_pad, msg_pad):
    """sk_stride = 4n + 5 or 4n + 8, msg_stride = len + 3 or len + 8.  Hedged: addrnd is packed whatever sk_stride is, and the bytes are the fixture's.
    Deterministic (d_addrnd NULL): opt_rand is PK.seed inside the key, so its pitch is sk_stride; the bytes are those of the packed run, of which the
    first three instances and the last are checked against the model by parts."""
    fam, D = E.SHAKE, libs["SHAKE"]
    name = fam.name(short)
    sz = fam.M.sizes(name)
    t = S.hedged(name)
    inst = [t[i % len(t)] for i in range(count)]
    sks, msgs, rnds, want = ([r[f] for r in inst] for f in range(4))
    sk_stride = sz["sk"] + key_pad if key_pad else None
    msg_stride = fam.K.MSG_LEN + msg_pad if msg_pad else None
    packed = dev_sign(torch, D, name, sks, msgs, offs=0)
    for i in sorted({0, 1, 2, count - 1}):
        assert S.exact_by_parts(name, sks[i], msgs[i], None, packed[i]) is None, (name, i, "deterministic, packed")
    for gap in GAPS:
        got = dev_sign(torch, D, name, sks, msgs, rnds, offs=0, sk_stride=sk_stride, msg_stride=msg_stride, gap=gap)
        assert got == want, (name, count, key_pad, msg_pad, hex(gap), "hedged", differing(got, want))
        got = dev_sign(torch, D, name, sks, msgs, offs=0, sk_stride=sk_stride, msg_stride=msg_stride, gap=gap)
        assert got == packed, (name, count, key_pad, msg_pad, hex(gap), "deterministic", differing(got, packed))
    if msg_pad:                                                           # one key for all (sk_stride = 0) with the messages at a pitch
        got = dev_sign(torch, D, name, sks[0], msgs, rnds, offs=0, msg_stride=msg_stride)
        assert got[0] == want[0] and got[3 % count] == want[0] and len(set(got)) == min(count, 3)
        assert [S.exact_by_parts(name, sks[0], msgs[i], rnds[i], got[i]) for i in (1, 2)] == [None, None]


# ---- workgroup edges -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [255, 256, 257, 513])
@pytest.mark.parametrize("tag", FAMS)
def test_verify_across_the_workgroups_of_the_per_instance_kernels(libs, torch, tag, count):
    """k_vf_digest, k_vf_fors_pk and k_vf_xmss (and their SHA-2 twins) take instance blockIdx.x * 256 + threadIdx.x: instances 0, 255, 256 and the
    last are tampered, each in another region, the rest are honest, so an instance that takes another's data or verdict shows"""
    fam, D, H = E.FAMILIES[tag], libs[tag], harness(tag)
    name = fam.name("128f")
    pks, msgs, sigs, want = tampered(fam, name, count, [0, 255, 256, count - 1])
    ok = H.dev_verify(torch, D, name, pks, msgs, sigs)
    assert ok == want, (name, count, differing(ok, want))
    hit = [i for i in range(count) if not want[i]]
    want1 = expected(fam, name, [pks[0]] * count, msgs, sigs)
    assert want1 == [1 if i % 3 == 0 and i not in hit else 0 for i in range(count)]        # under the first key: triple 0 alone verifies
    ok = H.dev_verify(torch, D, name, pks[0], msgs, sigs)
    assert ok == want1, (name, count, "pk_stride = 0", differing(ok, want1))
    # the same batch with instances 1 and 253 tampered instead: the edges of the workgroups are honest, and at 257 the one instance of the second is
    pks, msgs, sigs, want = tampered(fam, name, count, [1, 253])
    assert want[0] == want[255 % count] == want[count - 1] == 1
    ok = H.dev_verify(torch, D, name, pks, msgs, sigs)
    assert ok == want, (name, count, "honest edges", differing(ok, want))


@pytest.mark.parametrize("tag", FAMS)
def test_keygen_at_257_instances(libs, torch, tag):
    """instance i has seed triple i mod 67 of the model's 67: 67 divides neither 64 nor 256"""
    fam, D, H = E.FAMILIES[tag], libs[tag], harness(tag)
    name, count = fam.name("128f"), 257
    ref = fam.K.keys(name, 67)
    assert len(set(ref["pk"])) == 67
    pk, sk = H.dev_keygen(torch, D, name, *[[ref[k][i % 67] for i in range(count)] for k in ("sk_seed", "sk_prf", "pk_seed")])
    want_pk, want_sk = ([ref[k][i % 67] for i in range(count)] for k in ("pk", "sk"))
    assert pk == want_pk, (name, differing(pk, want_pk))
    assert sk == want_sk, (name, differing(sk, want_sk))


def test_sign_at_257_instances(libs, torch):
    """k_sg_prf_msg, k_sg_digest and k_sg_fors_pk at blockIdx.x = 1: instance i is hedged triple i mod 3, bytes equal to the fixture's"""
    name, count = E.SHAKE.name("128f"), 257
    t = S.hedged(name)
    inst = [t[i % 3] for i in range(count)]
    got = dev_sign(torch, libs["SHAKE"], name, [r[0] for r in inst], [r[1] for r in inst], [r[2] for r in inst])
    assert got == [r[3] for r in inst], (name, differing(got, [r[3] for r in inst]))


# ---- chosen digests ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("short", E.CHOSEN_SETS)
@pytest.mark.parametrize("tag", FAMS)
def test_digest_fields_at_their_edges(libs, torch, tag, short):
    """idx_leaf = 0 and 2^h' - 1, the top bit of idx_tree clear and set (bit 63 on 256f: the shift by 64 in layer_tree), FORS indices 0 and 2^a - 1:
    the three signatures of the table in one batch with an honest ordinary instance and a tampered one, and on SHAKE signed again"""
    fam, D, H = E.FAMILIES[tag], libs[tag], harness(tag)
    cases = [E.chosen(fam, short, case) for case in E.CASES]
    name = cases[0][0]
    pk0, m0, s0 = fam.K.signed(name)[1]
    last = cases[2]
    batch = [(pk0, m0, s0)] + [(c[1], c[3], c[5]) for c in cases] + [(last[1], last[3], E.flip(last[5], len(s0) - 1, 0)), (pk0, cases[0][3], cases[0][5])]
    want = expected(fam, name, *zip(*batch))
    assert want == [1, 1, 1, 1, 0, 0]
    ok = H.dev_verify(torch, D, name, *[list(x) for x in zip(*batch)])
    assert ok == want, (name, differing(ok, want))
    if tag == "SHAKE":
        got = dev_sign(torch, D, name, [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases])
        assert got == [c[5] for c in cases], (name, differing(got, [c[5] for c in cases]))


# ---- degenerate bytes ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,short", SETS)
def test_signatures_and_a_key_of_all_zero_and_all_ones_among_honest_instances(libs, torch, tag, short):
    fam, D, H = E.FAMILIES[tag], libs[tag], harness(tag)
    name = fam.name(short)
    pks, msgs, sigs = (list(x) for x in fam.K.tiled(name, 7))
    for at, (_, pk, msg, sig) in zip((1, 3, 4), E.degenerate_verify(fam, short)):
        pks[at], msgs[at], sigs[at] = pk, msg, sig
    want = expected(fam, name, pks, msgs, sigs)
    assert want == [1, 0, 1, 0, 0, 1, 1]
    ok = H.dev_verify(torch, D, name, pks, msgs, sigs)
    assert ok == want, (name, differing(ok, want))


def test_signing_under_secret_keys_of_all_zero_and_all_ones(libs, torch):
    """the expected bytes are the model's whole signatures (tests/helpers/slhdsa_edge_cases.py says why not exact_by_parts); the honest instances
    beside them are the fixture's (hedged) or checked by parts (deterministic)"""
    fam, D = E.SHAKE, libs["SHAKE"]
    name = fam.name(E.DEGENERATE_SIGN_SET)
    (_, sk_a, m_a, r_a, sig_a), (_, sk_b, m_b, r_b, sig_b) = E.degenerate_sign()
    t = S.hedged(name)
    assert r_a is not None and r_b is None
    got = dev_sign(torch, D, name, [t[0][0], sk_a, t[1][0]], [t[0][1], m_a, t[1][1]], [t[0][2], r_a, t[1][2]])
    assert got == [t[0][3], sig_a, t[1][3]], differing(got, [t[0][3], sig_a, t[1][3]])
    got = dev_sign(torch, D, name, [t[0][0], sk_b, t[1][0]], [t[0][1], m_b, t[1][1]])
    assert got[1] == sig_b
    assert [S.exact_by_parts(name, t[i][0], t[i][1], None, g) for i, g in ((0, got[0]), (1, got[2]))] == [None, None]


# ---- a flipped bit in every byte -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,short", SETS)
def test_a_flipped_bit_in_every_byte_of_a_signature(libs, torch, tag, short):
    """One batch per parameter set: the first fixture signature repeated on the device, instance j with bit b mod 8 of byte b flipped, b running over
    every byte of the signature, and the untouched signature at every 61st position (E.flips: 7 987 instances on 128s, 50 687 and 2.5 GB on 256f); one
    verify_dev call under one key, and the whole ok vector compared on the device.  The CPU test has the model's verdict at the ends of every region
    (128f) or at 16 spread positions; that every other flipped instance is rejected rests on second-preimage resistance: every byte of a signature
    enters a hash whose output the verifier carries up to the comparison with PK.root, so a kernel that accepts one of them did not read that byte."""
    fam, D = E.FAMILIES[tag], libs[tag]
    name = fam.name(short)
    t = E.flips(fam, name)
    count, size = t["count"], len(t["sig"])
    need = D.workspace_bytes(name, count, "verify") + count * size + 2048 * size * 10
    free, _ = torch.cuda.mem_get_info()
    if free < need + 2 ** 30:
        pytest.skip(f"{free} bytes of device memory are free; the test needs {need} and {2 ** 30}")
    try:
        batch = rows(torch, [t["sig"]]).repeat(count, 1)
        assert batch.is_contiguous() and batch.shape == (count, size)
        touched = torch.from_numpy(t["byte"] >= 0).cuda().nonzero().flatten()
        cols = torch.from_numpy(t["byte"]).cuda()[touched]
        batch[touched, cols] ^= torch.from_numpy(t["bit"]).cuda()[touched]            # the diagonal
        row, flipped = rows(torch, [t["sig"]]), torch.from_numpy(1 - t["want"].astype("int64")).cuda()
        for lo in range(0, count, 2048):                                      # one byte per flipped instance, no other; a slab at a time
            assert bool(((batch[lo:lo + 2048] != row).sum(dim=1) == flipped[lo:lo + 2048]).all().item()), (name, lo)
        ok = dev_verify_rows(torch, D, name, rows(torch, [t["pk"]]), rows(torch, [t["msg"]]).repeat(count, 1), batch)
        ne = (ok != torch.from_numpy(t["want"]).cuda()).nonzero().flatten()
        bad = [(j, int(t["byte"][j]), E.region_of(fam, name, int(t["byte"][j])) if t["byte"][j] >= 0 else "untouched") for j in ne[:8].tolist()]
        assert not bad, (name, int(ne.numel()), "instances differ; the first (instance, byte, region):", bad)
    finally:
        batch = ok = ne = touched = cols = None
        release(torch)
