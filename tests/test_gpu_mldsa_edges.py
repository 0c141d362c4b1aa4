"""ML-DSA on the MI355X at the inputs where psf_mldsa*.hip takes another path, against the pure-Python model, byte for byte over every instance.

Alignment.  The units branch on pointer alignment in kc::PtrReader (k_tr's 8-byte loads of pk, mu given to k_sign_seed), CatReader::le64 (tr || M' in
k_mu and k_sign_seed, with the seam at byte 64), put_words (8-byte stores of rho, K and tr into pk and sk) and, per lane, in k_verify_tail when mu is
given.  tests/test_gpu_mldsa.py puts every buffer one byte past a 16-byte boundary, which takes the byte-wise branch of them all; here KeyGen, Sign and
Verify run with every buffer at 0, 4 and 8, and with mixes in which one input of a reader is aligned and the other is not.

Strides.  Keys and messages at a pitch above their size, with a pitch that is and one that is not a multiple of 8, on the device forms and on the host
forms (whose repacking nothing else runs); every case twice with different bytes in the gaps.

Positions and values.  The tables of tests/helpers/mldsa_edge_cases.py (pinned to the model by tests/test_mldsa_edge_cases_cpu.py): a flipped bit in
every byte of a signature, the norm bound at every position, signatures and a key of all 0x00 / 0xFF, secret keys with fields KeyGen never writes, and
the signing instance in which ||c t0||_inf >= gamma2 fires.

Every call keeps the checks of the harness (tests/helpers/mldsa_gpu.py, tests/helpers/mldsa_sign_gpu.py): guard bytes around every output, nothing
written outside the workspace, the workspace zero after KeyGen and after signing, d_live against d_rounds after every round, the flag unchanged."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests.helpers import mldsa_edge_cases as E
from tests.helpers import mldsa_model as M
from tests.helpers.mldsa_gpu import NAMES, dev_keygen, dev_verify, keys, mu_of, offsets, pitched
from tests.helpers.mldsa_sign_gpu import MU, batch, dev_sign, reference

pytestmark = pytest.mark.gpu

SHAPES = [("ML-DSA-44", 67), ("ML-DSA-65", 3), ("ML-DSA-87", 3)]
MSG_LENS = (72, 136, 71)                                                  # tr || M' is 64 bytes longer: whole words on the two sides of a block edge, and not whole words
PATTERNS = {
    "all0": offsets(0, 0),
    "all4": offsets(4, 4),
    "all8": offsets(8, 8),
    "in0_out1": offsets(0, 1),
    "in1_out0": offsets(1, 0),
    "sk0_msg1": offsets(0, 0, in_msg=1),                                 # CatReader: the key (tr) aligned, the message not
    "sk1_msg0": offsets(0, 0, in_sk=1, in_pk=1),                         # ... and the reverse; k_tr reads pk by bytes
    "mu0": offsets(0, 0),                                                # mu given at an aligned pointer, Verify and Sign
}
DISTINCT = 3


@pytest.fixture(scope="module")
def D():
    import tools_amd
    return tools_amd.mldsa


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def differing(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]][:8]


@functools.lru_cache(maxsize=None)
def signing(name, msg_len, one_key):
    """DISTINCT instances (pk, sk, M', rnd, sigma, attempts) of the restated signer under DISTINCT keys, or all under the first"""
    ks = keys(name, DISTINCT)
    rng = random.Random(4409 * NAMES.index(name) + 17 * msg_len + one_key)
    out = []
    for i in range(DISTINCT):
        j = 0 if one_key else i
        msg, rnd = rng.randbytes(msg_len), rng.randbytes(32)
        out.append((ks["pk"][j], ks["sk"][j], msg, rnd) + reference(name, ks["sk"][j], msg, rnd, False))
    return out


def tiled(name, count, msg_len, one_key):
    """`count` instances, instance i is instance i mod DISTINCT of signing(): (pks, sks, msgs, rnds, sigs, attempts)"""
    t = signing(name, msg_len, one_key)
    return tuple([t[i % DISTINCT][f] for i in range(count)] for f in range(6))


def sign_then_verify(torch, D, name, count, msg_len, one_key, what, as_mu=False, **kw):
    """Sign on the device, compare every signature and attempt count with the model, then verify the device's own signatures there; `kw`: offs, strides, gap"""
    pks, sks, msgs, rnds, want, attempts = tiled(name, count, msg_len, one_key)
    kind = 0
    if as_mu:                                                             # the same instances with mu = H(tr || M', 64) given: the same signatures
        msgs, kind = [mu_of(p, m) for p, m in zip(pks, msgs)], MU
    skw = {k: v for k, v in kw.items() if k != "pk_stride"}
    vkw = {k: v for k, v in kw.items() if k != "sk_stride"}
    sigs, rounds, trail = dev_sign(torch, D, name, sks[0] if one_key else sks, msgs, rnds, msg_kind=kind, **skw)
    assert rounds == attempts, (what, differing(rounds, attempts))
    assert sigs == want, (what, differing(sigs, want))
    assert trail[-1] == 0 and len(trail) == max(attempts)
    ok, why = dev_verify(torch, D, name, pks[0] if one_key else pks, msgs, sigs, msg_kind=kind, **vkw)
    assert (ok, why) == ([1] * count, [0] * count), (what, differing(why, [0] * count))


# ---- alignment ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("name,count", SHAPES)
def test_keygen_sign_and_verify_equal_the_model_at_every_alignment(D, torch, name, count, pattern):
    offs = PATTERNS[pattern]
    ref = keys(name, count)
    pk, sk, _ = dev_keygen(torch, D, name, ref["xi"], flag=0, offs=offs)
    assert pk == ref["pk"], (name, count, pattern, differing(pk, ref["pk"]))
    assert sk == ref["sk"], (name, count, pattern, differing(sk, ref["sk"]))
    for one_key in (False, True):
        if pattern == "mu0":
            sign_then_verify(torch, D, name, count, 136, one_key, (name, count, pattern, one_key), as_mu=True, offs=offs)
            continue
        for msg_len in MSG_LENS:
            sign_then_verify(torch, D, name, count, msg_len, one_key, (name, count, pattern, msg_len, one_key), offs=offs)


# ---- strides -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("msg_pad", [0, 3, 8])
@pytest.mark.parametrize("key_pad", [0, 5, 8])
@pytest.mark.parametrize("name,count", [("ML-DSA-44", 67), ("ML-DSA-87", 3)])
def test_keys_and_messages_at_a_padded_stride(D, torch, name, count, key_pad, msg_pad):
    """base pointers aligned, so that the stride alone decides the fast paths; the results are those of the packed run (key_pad = msg_pad = 0) and the
    model's, whatever lies in the gaps"""
    sz, msg_len = M.sizes(name), 72
    for gap in (0xC3, 0x11) if key_pad or msg_pad else (0xC3,):
        kw = dict(offs=0, gap=gap, msg_stride=msg_len + msg_pad if msg_pad else None)
        sign_then_verify(torch, D, name, count, msg_len, False, (name, key_pad, msg_pad, gap), pk_stride=sz["pk"] + key_pad if key_pad else None,
                         sk_stride=sz["sk"] + key_pad if key_pad else None, **kw)
        if msg_pad:
            sign_then_verify(torch, D, name, count, msg_len, True, (name, "one key", msg_pad, gap), **kw)


def test_mu_given_at_a_stride_of_68_has_aligned_and_unaligned_lanes_in_a_wave(D, torch):
    name, count = "ML-DSA-44", 67
    for gap in (0xC3, 0x11):
        for one_key in (False, True):
            sign_then_verify(torch, D, name, count, 136, one_key, (name, "mu at 68", one_key, gap), as_mu=True, offs=0, msg_stride=68, gap=gap)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("name,count", [("ML-DSA-44", 67), ("ML-DSA-87", 3)])
def test_host_forms_repack_padded_host_arrays(D, torch, name, count):
    """psf_mldsa_verify and psf_mldsa_sign through ctypes with keys and messages at padded strides in host memory"""
    sz, msg_len = M.sizes(name), 71
    pks, sks, msgs, rnds, want, attempts = tiled(name, count, msg_len, False)
    L = D._lib()
    rnd = np.frombuffer(b"".join(rnds), np.uint8).copy()
    sigs_in = np.frombuffer(b"".join(want), np.uint8).copy()
    for key_pad, msg_pad in ((5, 3), (8, 8), (5, 0), (0, 3)):
        for gap in (0xC3, 0x11):
            what = (name, key_pad, msg_pad, gap)
            pk = np.frombuffer(pitched(pks, sz["pk"] + key_pad, gap) if key_pad else b"".join(pks), np.uint8).copy()
            sk = np.frombuffer(pitched(sks, sz["sk"] + key_pad, gap) if key_pad else b"".join(sks), np.uint8).copy()
            msg = np.frombuffer(pitched(msgs, msg_len + msg_pad, gap ^ 0x5F) if msg_pad else b"".join(msgs), np.uint8).copy()
            sig, rd = np.full((count, sz["sig"]), 0xEE, np.uint8), np.full(count, 77, np.uint32)
            rc = L.psf_mldsa_sign(0, D.PARAM[name], count, _vp(sk), sz["sk"] + key_pad, _vp(msg), msg_len, msg_len + msg_pad, 0, _vp(rnd), _vp(sig), 400, _vp(rd))
            assert rc == 0, what
            assert [int(r) for r in rd] == attempts, (what, differing([int(r) for r in rd], attempts))
            assert [bytes(s) for s in sig] == want, (what, differing([bytes(s) for s in sig], want))
            ok, why = np.full(count, 9, np.uint8), np.full(count, 9, np.uint8)
            rc = L.psf_mldsa_verify(0, D.PARAM[name], count, _vp(pk), sz["pk"] + key_pad, _vp(msg), msg_len, msg_len + msg_pad, 0, _vp(sigs_in), _vp(ok), _vp(why))
            assert rc == 0 and ok.tolist() == [1] * count and why.tolist() == [0] * count, (what, ok.tolist(), why.tolist())
    # one key for all with padded messages, and an instance that must fail: the message of its neighbour
    pks, sks, msgs, rnds, want, attempts = tiled(name, count, msg_len, True)
    moved = [msgs[1]] + list(msgs[1:])
    msg = np.frombuffer(pitched(moved, msg_len + 3, 0x77), np.uint8).copy()
    pk, sigs_in = np.frombuffer(pks[0], np.uint8).copy(), np.frombuffer(b"".join(want), np.uint8).copy()
    ok, why = np.full(count, 9, np.uint8), np.full(count, 9, np.uint8)
    assert L.psf_mldsa_verify(0, D.PARAM[name], count, _vp(pk), 0, _vp(msg), msg_len, msg_len + 3, 0, _vp(sigs_in), _vp(ok), _vp(why)) == 0
    assert ok.tolist() == [0] + [1] * (count - 1) and why.tolist() == [M.HASH] + [0] * (count - 1)


# ---- positions and values ----------------------------------------------------------------------------------------------------------------------------

def _verify_table(torch, D, name, pk, msg, sigs, want, off, one_key):
    n = len(sigs)
    ok, why = dev_verify(torch, D, name, pk if one_key else [pk] * n, [msg] * n, sigs, offs=off)
    assert why == want, (name, off, one_key, [(i, why[i], want[i]) for i in differing(why, want)])
    assert ok == [1 if w == 0 else 0 for w in want]


@pytest.mark.parametrize("one_key", [False, True], ids=["key_per_instance", "one_key"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_a_flipped_bit_in_every_byte_of_a_signature(D, torch, name, off, one_key):
    pk, msg, sigs, want = E.every_sig_byte(name)
    _verify_table(torch, D, name, pk, msg, sigs, want, off, one_key)


@pytest.mark.parametrize("one_key", [False, True], ids=["key_per_instance", "one_key"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_the_norm_bound_at_every_position(D, torch, name, off, one_key):
    pk, msg, sigs, want, _ = E.every_z_position(name)
    _verify_table(torch, D, name, pk, msg, sigs, want, off, one_key)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_signatures_and_a_key_of_all_zero_and_all_one_bits(D, torch, name, off):
    inst, want = E.extreme(name)
    ok, why = dev_verify(torch, D, name, [p for p, _, _ in inst], [m for _, m, _ in inst], [s for _, _, s in inst], offs=off)
    assert why == want and ok == [0] * len(inst), (name, off, why, want)
    mus = [mu_of(p, m) for p, m, _ in inst]                               # mu given: the same verdicts
    assert dev_verify(torch, D, name, [p for p, _, _ in inst], mus, [s for _, _, s in inst], msg_kind=MU, offs=off)[1] == want


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_secret_keys_with_fields_keygen_never_writes(D, torch, name, off):
    inst = E.odd_sk(name)
    want = [reference(name, sk, mu, rnd, True) for sk, mu, rnd in inst]
    sks, mus = [sk for sk, _, _ in inst], [mu for _, mu, _ in inst]
    sigs, rounds, _ = dev_sign(torch, D, name, sks, mus, None, msg_kind=MU, offs=off)                  # rnd = 0: d_rnd = NULL
    assert rounds == [w[1] for w in want], (name, off, differing(rounds, [w[1] for w in want]))
    assert sigs == [w[0] for w in want], (name, off, differing(sigs, [w[0] for w in want]))
    for n in range(3):                                                    # each key as the one key for all
        part = slice(6 * n, 6 * n + 6)
        sigs, rounds, _ = dev_sign(torch, D, name, sks[6 * n], mus[part], [bytes(32)] * 6, msg_kind=MU, offs=off)
        assert (sigs, rounds) == ([w[0] for w in want[part]], [w[1] for w in want[part]]), (name, off, n)


# ---- the c t0 case -----------------------------------------------------------------------------------------------------------------------------------

def test_the_instance_in_which_c_t0_fires(D, torch):
    name = E.CT0_NAME
    sk, mu, rnd = E.ct0_instance()
    sig, attempts, fired = E.ct0_trace()
    assert 4 in fired and sig is not None
    # alone
    for off in (0, 1):
        assert dev_sign(torch, D, name, [sk], [mu], [rnd], msg_kind=MU, offs=off)[:2] == ([sig], [attempts]), off
    got = dev_sign(torch, D, name, [sk], [mu], [rnd], msg_kind=MU, with_rounds=False, with_fail=False)          # d_rounds = d_fail = NULL
    assert got[0] == [sig] and got[1] is None and len(got[2]) == attempts
    # inside a batch of 65 with the searched cases: a key per instance, the case at the edge of the first wave and in the second
    trio = E.ct0_instances()
    rest = list(zip(*batch(name, False)))                                  # 40 instances, the searched cases of mldsa_sign_cases among them
    inst = (rest + rest)[:65]
    inst[10], inst[30], inst[63], inst[64] = trio[0], trio[2], trio[1], trio[1]
    want = [reference(name, s, m, r, True) for s, m, r in inst]
    sigs, rounds, _ = dev_sign(torch, D, name, [s for s, _, _ in inst], [m for _, m, _ in inst], [r for _, _, r in inst], msg_kind=MU)
    assert rounds == [w[1] for w in want], differing(rounds, [w[1] for w in want])
    assert sigs == [w[0] for w in want], differing(sigs, [w[0] for w in want])
    assert sigs[63] == sigs[64] == sig and rounds[63] == attempts
    # one key for all
    want = [reference(name, s, m, r, True) for s, m, r in trio]
    sigs, rounds, _ = dev_sign(torch, D, name, sk, [m for _, m, _ in trio], [r for _, _, r in trio], msg_kind=MU, offs=0)
    assert (sigs, rounds) == ([w[0] for w in want], [w[1] for w in want]) and sigs[1] == sig
