"""The tables of tests/helpers/slhdsa_edge_cases.py against the pure-Python models, for both hash families: no GPU test of the SLH-DSA edge suite
carries an expected value that is not tied to the model here.  Alone this module takes about 75 s, of which about 50 s are the shared fixture's model
signatures of the s sets (5 to 10 s each), which the other SLH-DSA modules make too; its own work is about 25 s."""
import numpy as np
import pytest

from tests.helpers import slhdsa_edge_cases as E
from tests.helpers import slhdsa_model as SM
from tests.helpers import slhdsa_sha2_model as S2
from tests.helpers import slhdsa_sign_cases as S

FAMS = sorted(E.FAMILIES)
SETS = [(tag, short) for tag in FAMS for short in E.SHORT]


@pytest.mark.parametrize("tag", FAMS)
def test_the_recorded_counters_are_the_first_the_search_finds(tag):
    fam = E.FAMILIES[tag]
    assert sorted(k for k in E.COUNTERS if k[0] == tag) == sorted((tag, short, case) for short in E.CHOSEN_SETS for case in E.CASES)
    for short in E.CHOSEN_SETS:
        for case in E.CASES:
            assert E.search(fam, fam.name(short), case) == E.COUNTERS[tag, short, case], (tag, short, case)


@pytest.mark.parametrize("tag", FAMS)
def test_the_chosen_signatures_have_their_digest_fields_and_the_model_accepts_them(tag):
    fam = E.FAMILIES[tag]
    seen = 0
    for name, pk, sk, msg, addrnd, sig in E.all_chosen(fam):
        s = fam.M.PARAMS[name]
        n = s.n
        case = E.CASES[seen % 3]
        seen += 1
        assert (pk, sk) == E.first_key(fam, name) and len(msg) == fam.K.MSG_LEN and len(addrnd) == n
        r, md, idx_tree, idx_leaf, fors = E.fields(fam, name, sk, msg, addrnd)
        assert sig[:n] == r and len(sig) == fam.M.sizes(name)["sig"]
        # the fields again from the signature and the public key, as a verifier gets them
        assert fam.M.split_digest(name, fam.h_msg(name, sig[:n], pk[:n], pk[n:], msg)) == (md, idx_tree, idx_leaf)
        tree_bits = s.h - s.hp
        assert tree_bits == (64 if n == 32 else 63) and idx_tree < 1 << tree_bits and len(fors) == s.k
        if case == "leaf_0_tree_top_clear":
            assert idx_leaf == 0 and idx_tree >> (tree_bits - 1) == 0
        elif case == "leaf_max_tree_top_set":
            assert idx_leaf == (1 << s.hp) - 1 and idx_tree >> (tree_bits - 1) == 1
            assert n != 32 or idx_tree >= 1 << 63
        else:
            assert fors[s.k - 1] == (1 << s.a) - 1
            assert n == 32 or fors[0] == 0
            assert n != 32 or (s.k * s.a + 7) // 8 == 40 and (s.k * s.a - 1) // 8 == 39         # the last index ends inside byte 39 of md
        assert fam.K.expect(name, pk, msg, sig) is True
        assert fam.K.expect(name, pk, msg, E.flip(sig, len(sig) - 1, 7)) is False
        if tag == "SHAKE":
            assert S.exact_by_parts(name, sk, msg, addrnd, sig) is None
    assert seen == 6


@pytest.mark.parametrize("tag,short", SETS)
def test_the_model_rejects_the_degenerate_signatures_and_key(tag, short):
    fam = E.FAMILIES[tag]
    name = fam.name(short)
    cases = E.degenerate_verify(fam, short)
    assert [c[0] for c in cases] == ["sig 0x00", "sig 0xFF", "pk 0x00"]
    sz = fam.M.sizes(name)
    assert set(cases[0][3]) == {0} and set(cases[1][3]) == {255} and set(cases[2][1]) == {0}
    assert all(len(c[1]) == sz["pk"] and len(c[3]) == sz["sig"] for c in cases)
    assert fam.K.expect(name, cases[0][1], cases[0][2], cases[2][3]) is True          # the honest signature under its own key
    assert [fam.K.expect(name, pk, msg, sig) for _, pk, msg, sig in cases] == [False] * 3


def test_the_signatures_under_degenerate_secret_keys_are_the_models():
    name = E.SHAKE.name(E.DEGENERATE_SIGN_SET)
    n = SM.PARAMS[name].n
    cases = E.degenerate_sign()
    assert [(c[0], set(c[1]), c[3] is None) for c in cases] == [("sk 0x00", {0}, False), ("sk 0xFF", {255}, True)]
    sch = S2.Scheme(SM.PARAMS[name], S2.Shake)
    for what, sk, msg, addrnd, sig in cases:
        assert len(sk) == 4 * n and sig == SM.sign_internal(name, msg, sk, addrnd)
        assert sig[:n] == SM.prf_msg(name, sk[n:2 * n], sk[2 * n:3 * n] if addrnd is None else addrnd, msg)
        # PK.root in the key is not the hypertree's root: the signature leads to the true root, which is why exact_by_parts does not serve here
        true_root = SM.keygen_internal(name, sk[:n], sk[n:2 * n], sk[2 * n:3 * n])[1][n:]
        assert true_root != sk[3 * n:] and sch.root_from_sig(msg, sig, sk[2 * n:]) == true_root
        assert S.exact_by_parts(name, sk, msg, addrnd, sig) == "verify"


@pytest.mark.parametrize("tag,short", SETS)
def test_the_flip_table_covers_every_byte_and_the_model_gives_its_verdicts(tag, short):
    """The model's verdict at the first and the last byte of every region on 128f and at 16 spread positions on the other sets, and at two untouched
    instances.  The verdict 0 at every other flipped instance rests on second-preimage resistance: each byte of a signature enters a hash whose output
    the verifier carries up to the comparison with PK.root."""
    fam = E.FAMILIES[tag]
    name = fam.name(short)
    t = E.flips(fam, name)
    size = fam.M.sizes(name)["sig"]
    assert (t["pk"], t["msg"], t["sig"]) == fam.K.signed(name)[0] and len(t["sig"]) == size
    count = t["count"]
    assert len(t["byte"]) == len(t["bit"]) == len(t["want"]) == count == size + (size + E.EVERY - 2) // (E.EVERY - 1)
    touched = t["byte"] >= 0
    assert np.array_equal(t["byte"][touched], np.arange(size))                         # every byte once, in order: none left out
    assert np.array_equal(np.nonzero(~touched)[0], np.arange(0, count, E.EVERY))       # the untouched signature at every 61st position
    assert np.array_equal(t["bit"][touched], 1 << (np.arange(size) % 8)) and not t["bit"][~touched].any()
    assert np.array_equal(t["want"], (~touched).astype(np.uint8))
    pins = E.pinned_instances(fam, name)
    s = fam.M.PARAMS[name]
    assert len(pins) >= 18 and (short != "128f" or len(pins) == 2 + 2 * (1 + 2 * s.k + 2 * s.d))
    for j in pins:
        sig = E.flipped_instance(t, j)
        assert (sig == t["sig"]) == (j % E.EVERY == 0)
        assert int(fam.K.expect(name, t["pk"], t["msg"], sig)) == int(t["want"][j]), (name, j, int(t["byte"][j]))
    regions = {E.region_of(fam, name, int(t["byte"][j])) for j in pins[2:]}
    assert short != "128f" or len(regions) == 1 + 2 * s.k + 2 * s.d


@pytest.mark.parametrize("tag", FAMS)
def test_the_fixtures_reach_both_extreme_digits_in_both_parts_and_both_leaf_parities(tag):
    cov = E.coverage(E.FAMILIES[tag])
    assert {0, 15} <= cov["msg"] and {0, 15} <= cov["csum"] and cov["leaf"] == {0, 1}
