"""SLH-DSA signing for the SHA-2 sets on the MI355X (psf_slhdsa_sha2_sign.hip) where tests/test_gpu_slhdsa_sha2_sign.py does not look, against the
pure-Python model byte for byte and over every instance: what tests/test_gpu_slhdsa_edges.py and tests/test_gpu_slhdsa_large.py ask of the SHAKE signer.

Alignment.  The unit reads and writes by bytes (load_be, Cat2Reader, Cat3Reader, store_be), which the compiler may merge into wide accesses; here every
buffer sits at offsets 0, 4 and 8 from a 16-byte boundary.

Strides.  Keys and messages at a pitch above their size, one that is and one that is not a multiple of 8, from aligned base pointers so that the pitch
alone decides; each alone and combined, every padded case twice with different bytes in the gaps; the deterministic variant too, whose opt_rand is
PK.seed read out of the padded keys, while addrnd stays packed whatever sk_stride is.

Workgroup edges.  The per-instance kernels run 256 lanes per workgroup, and the packed tree kernel takes 64 trees of 128f per workgroup: 255, 256, 257
and 513 instances under 3 keys.

Positions and values.  The searched inputs of tests/helpers/slhdsa_edge_cases.py (idx_leaf 0 and 2^h' - 1, the top bit of idx_tree clear and set, FORS
indices 0 and 2^a - 1), and secret keys of all 0x00 / 0xFF.

Size.  One call whose signatures pass 2^32 bytes: 86 152 instances of 256f.

Every call keeps the checks of the harness (tests/helpers/slhdsa_sha2_sign_gpu.py): guard bytes around the signatures, nothing written outside the
workspace, the workspace all zero after signing."""
import pytest

from tests.helpers import slhdsa_edge_cases as E
from tests.helpers import slhdsa_sha2_cases as K
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers import slhdsa_sha2_sign_cases as S
from tests.helpers.mlkem_gpu import _out, _put_dev, _take_dev
from tests.helpers.slhdsa_gpu import release, rows, same_rows, tile
from tests.helpers.slhdsa_sha2_sign_gpu import SignScratch, dev_sign
from tests.test_gpu_slhdsa_large import PERIOD, SIG_256F, VERIFY_COUNT, crossing, pad256, room, sign_sections

pytestmark = pytest.mark.gpu

SHAPES = [(K.F128, 67), (K.F256, 3)]
PADS = [(k, m) for k in (0, 5, 8) for m in (0, 3, 8) if k or m]
GAPS = (0xC3, 0x11)


@pytest.fixture(scope="module")
def D():
    import tools_amd
    return tools_amd.slhdsa_sha2


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def differing(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


def tiled(name, count):
    """instance i is hedged triple i mod 3: (sks, msgs, addrnds, SIGs)"""
    t = S.hedged(name)
    inst = [t[i % len(t)] for i in range(count)]
    return tuple([r[f] for r in inst] for f in range(4))


@pytest.mark.parametrize("off", [0, 4, 8])
@pytest.mark.parametrize("name,count", SHAPES)
def test_signatures_equal_the_model_at_every_alignment(D, torch, name, count, off):
    sks, msgs, rnds, want = tiled(name, count)
    got = dev_sign(torch, D, name, sks, msgs, rnds, offs=off)
    assert got == want == K.tiled(name, count)[2], (name, count, off, differing(got, want))
    got = dev_sign(torch, D, name, sks[0], [msgs[0]] * count, [rnds[0]] * count, offs=off)
    assert got == [want[0]] * count, (name, count, off, "sk_stride = 0", differing(got, [want[0]] * count))
    sk, msg, sig = S.edge_inputs(name)[0]
    assert dev_sign(torch, D, name, [sk] * 2, [msg] * 2, offs=off) == [sig] * 2, (name, off, "deterministic")


@pytest.mark.parametrize("key_pad,msg_pad", PADS)
@pytest.mark.parametrize("name,count", SHAPES)
def test_sign_with_keys_and_messages_at_a_padded_stride(D, torch, name, count, key_pad, msg_pad):
    """sk_stride = 4n + 5 or 4n + 8, msg_stride = len + 3 or len + 8.  Hedged: addrnd is packed whatever sk_stride is, and the bytes are the fixture's.
    Deterministic (d_addrnd NULL): opt_rand is PK.seed inside the key, so its pitch is sk_stride; the bytes are those of the packed run, of which the
    first three instances and the last are checked against the model by parts."""
    sz = M.sizes(name)
    sks, msgs, rnds, want = tiled(name, count)
    sk_stride = sz["sk"] + key_pad if key_pad else None
    msg_stride = K.MSG_LEN + msg_pad if msg_pad else None
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


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_sign_across_the_workgroups(D, torch, count):
    """k_sg_prf_msg, k_sg_digest and k_sg_fors_pk take instance blockIdx.x * 256 + threadIdx.x, and k_sg_tree 64 trees of 22 per instance to a workgroup:
    instance i is hedged triple i mod 3, so neighbouring instances differ in key, message and addrnd, and the bytes are the fixture's"""
    name = K.F128
    sks, msgs, rnds, want = tiled(name, count)
    assert len(set(sks)) == 3
    got = dev_sign(torch, D, name, sks, msgs, rnds)
    assert got == want, (name, count, differing(got, want))


@pytest.mark.parametrize("short", E.CHOSEN_SETS)
def test_digest_fields_at_their_edges(D, torch, short):
    """idx_leaf = 0 and 2^h' - 1, the top bit of idx_tree clear and set (bit 63 on 256f: the shift by 64 in layer_tree), FORS indices 0 and 2^a - 1: the
    three searched (M, addrnd) in one batch between two ordinary instances, every one checked by parts"""
    cases = [E.chosen_inputs(E.SHA2, short, case) for case in E.CASES]
    name = cases[0][0]
    t = S.hedged(name)
    batch = [t[1][:3]] + [(c[2], c[3], c[4]) for c in cases] + [t[2][:3]]
    s = M.PARAMS[name]
    seen = [E.fields(E.SHA2, name, *b)[2:] for b in batch[1:4]]
    assert seen[0][1] == 0 and seen[1][1] == (1 << s.hp) - 1 and seen[2][2][s.k - 1] == (1 << s.a) - 1
    got = dev_sign(torch, D, name, *[list(x) for x in zip(*batch)])
    assert got[0] == t[1][3] and got[4] == t[2][3], name
    assert [S.exact_by_parts(name, *b, g) for b, g in zip(batch, got)] == [None] * 5, name


def test_signing_under_secret_keys_of_all_zero_and_all_ones(D, torch):
    """the expected bytes are the model's whole signatures (S.degenerate_sign says why not exact_by_parts); the honest instances beside them are the
    fixture's (hedged) or checked by parts (deterministic)"""
    name = K.F128
    (_, sk_a, m_a, r_a, sig_a), (_, sk_b, m_b, r_b, sig_b) = S.degenerate_sign()
    t = S.hedged(name)
    assert r_a is not None and r_b is None
    got = dev_sign(torch, D, name, [t[0][0], sk_a, t[1][0]], [t[0][1], m_a, t[1][1]], [t[0][2], r_a, t[1][2]])
    assert got == [t[0][3], sig_a, t[1][3]], differing(got, [t[0][3], sig_a, t[1][3]])
    got = dev_sign(torch, D, name, [t[0][0], sk_b, t[1][0]], [t[0][1], m_b, t[1][1]])
    assert got[1] == sig_b
    assert [S.exact_by_parts(name, t[i][0], t[i][1], None, g) for i, g in ((0, got[0]), (1, got[2]))] == [None, None]


def sign_rows(torch, D, name, count, period):
    """sign_dev over `count` instances, instance i the (sk, M, addrnd) of period[i mod 3], a key per instance; the guards and the workspace are checked on
    the device; returns the signatures as a (count, size) device tensor and what keeps it alive"""
    size = M.sizes(name)["sig"]
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


def test_sign_with_the_signatures_at_4_gib(D, torch):
    """k_sg_prf_msg, k_sg_fors, k_sg_fors_top, k_sg_tree and k_sg_wots write at c * sig_len: SHA2-256f at the smallest ragged batch whose signatures pass
    2^32 bytes, the hedged fixture tiled with period 3, every byte compared on the device with the model's; the workspace is about 51 GB"""
    name, count = K.F256, VERIFY_COUNT
    s, sz, ln = M.PARAMS[name], M.sizes(name), M.wots_len(name)[2]
    crossing(count, SIG_256F)
    need = D.sign_workspace_bytes(name, count)
    assert sz["sig"] == SIG_256F and need == sum(pad256(b) for b in sign_sections(s, ln, count))
    room(torch, need, count * (SIG_256F + sz["sk"] + K.MSG_LEN + s.n) + PERIOD * 2048 * SIG_256F * 2)
    t = S.hedged(name)
    assert len(t) == PERIOD
    try:
        sig, keep = sign_rows(torch, D, name, count, [r[:3] for r in t])
        same_rows(torch, sig, rows(torch, [r[3] for r in t]), (name, "sig"))
    finally:
        sig = keep = None
        release(torch)
