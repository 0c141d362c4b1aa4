"""The case tables of tests/helpers/mldsa_edge_cases.py against the model, without a GPU: the rule that predicts `why` for a flipped bit in every byte
of a signature (proved with M.verify_why at every byte of c~, every hint byte, both ends of every polynomial of z and every 16th byte of z), the
positions and values of the norm-bound table, the extreme signatures and key, the secret keys with eta-fields that KeyGen never writes (the restated
signer equals the model's sign_internal on them, within 64 attempts), and the searched instance in which ||c t0||_inf >= gamma2 fires."""
import pytest

from tests.helpers import mldsa_edge_cases as E
from tests.helpers import mldsa_model as M
from tests.helpers import mldsa_sign_cases as K
from tests.helpers import mldsa_sign_model as S
from tests.helpers.mldsa_gpu import layout, with_z_coefficient

NAMES = sorted(M.PARAMS)
HINT, NORM, HASH = M.HINT, M.NORM, M.HASH


@pytest.mark.parametrize("name", NAMES)
def test_rule_of_a_flipped_bit_in_every_byte_of_a_signature(name):
    pk, msg, sigs, want = E.every_sig_byte(name)
    size, lay = M.sizes(name)["sig"], layout(name)
    assert len(sigs) == len(want) == size + 1 and M.verify_why(pk, msg, sigs[0], name) == want[0] == 0
    for b in range(size):
        diff = [i for i in range(size) if sigs[1 + b][i] != sigs[0][i]]
        assert diff == [b] and sigs[1 + b][b] ^ sigs[0][b] == 1 << (b % 8), b
        assert want[1 + b] & HASH and (want[1 + b] & NORM == 0 or lay["z"] <= b < lay["hint"]) and (want[1 + b] & HINT == 0 or b >= lay["hint"]), b
    proof = E.proof_positions(name)
    assert set(range(lay["z"])) <= set(proof) and set(range(lay["hint"], size)) <= set(proof)
    zs = [b for b in proof if lay["z"] <= b < lay["hint"]]
    assert max(b - a for a, b in zip(zs, zs[1:])) <= 16 and zs[0] == lay["z"] and zs[-1] == lay["hint"] - 1
    for b in proof:
        assert M.verify_why(pk, msg, sigs[1 + b], name) == want[1 + b], (name, b)
    assert HINT | HASH in want and HASH in want[1 + lay["hint"]:]
    # NORM: one flipped bit takes an honest coefficient over the bound only from a window of about beta values, so the table may hold no such byte.
    # Those it holds are all run, and the rule's NORM branch is proved on both sides of the bound from coefficients set next to it.
    l, g1, beta = M.PARAMS[name][1], M.PARAMS[name][5], M.PARAMS[name][7]
    for b in range(lay["z"], lay["hint"]):
        if want[1 + b] & NORM:
            assert M.verify_why(pk, msg, sigs[1 + b], name) == NORM | HASH and M.inf_norm(M.sig_decode(sigs[1 + b], name)[1]) >= g1 - beta
    bits = lay["zb"] // 32
    for poly, index in ((0, 0), (l - 1, 255), (l // 2, 101)):
        pos, bit = lay["z"] + lay["zb"] * poly + bits * index // 8, bits * index % 8              # the lowest bit of the field
        for start, after, why in ((g1 - beta - 1, g1 - beta, NORM | HASH), (g1 - beta, g1 - beta - 1, HASH)):
            new, w = E.flipped(name, with_z_coefficient(name, sigs[0], poly, index, start), pos, bit)
            assert E.z_field(name, new, poly, index) == after == M.sig_decode(new, name)[1][poly][index]
            assert w == why == M.verify_why(pk, msg, new, name), (name, poly, index, start)


@pytest.mark.parametrize("name", NAMES)
def test_norm_bound_at_every_position(name):
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    pk, msg, sigs, want, where = E.every_z_position(name)
    polys = range(l) if name == "ML-DSA-44" else (0, l - 1)
    edge = {(p, i) for (p, i, v), w in zip(where, want) if abs(v) == g1 - beta}
    inside = [(p, i) for p, i, v in where if abs(v) == g1 - beta - 1]
    if name == "ML-DSA-44":
        assert edge == {(p, i) for p in polys for i in range(256)}
    else:
        assert edge == {(p, 8 * g + e) for p in polys for g in range(32) for e in (0, 7)}
    assert sorted((p, i // 8) for p, i in inside) == [(p, g) for p in polys for g in range(32)] and len({i % 8 for p, i in inside}) == 8
    assert {v > 0 for p, i, v in where} == {True, False} and len(where) == len(edge) + len(inside)
    _, _, honest = E.honest(name)
    for n, ((p, i, v), s, w) in enumerate(zip(where, sigs, want)):
        z = M.sig_decode(s, name)[1]
        assert z[p][i] == v == E.z_field(name, s, p, i) and s[:cb] == honest[:cb] and s[layout(name)["hint"]:] == honest[layout(name)["hint"]:]
        assert (M.inf_norm(z) >= g1 - beta) == bool(w & NORM) == (abs(v) == g1 - beta) and w & HASH, (name, n)
        if n % 37 == 0 or n >= len(where) - 3:
            assert M.verify_why(pk, msg, s, name) == w, (name, n)


@pytest.mark.parametrize("name", NAMES)
def test_extreme_signatures_and_key(name):
    k, l, eta, tau, cb, g1, g2, beta, omega = M.PARAMS[name]
    inst, want = E.extreme(name)
    assert want == [NORM | HASH, NORM | HINT | HASH, NORM | HASH, NORM | HASH, HASH], want
    zs = [M.sig_decode(s, name)[1] for _, _, s in inst]
    for z, v in ((zs[0], g1), (zs[1], -(g1 - 1)), (zs[2], g1), (zs[3], -(g1 - 1))):
        assert all(x == v for p in z for x in p)
    assert all(x << M.D == M.Q - 1 for p in M.pk_decode(inst[4][0], k)[1] for x in p)
    assert inst[4][0][:32] == inst[0][0][:32] and M.hint_bit_unpack(inst[0][2][layout(name)["hint"]:], k, omega) is not None


@pytest.mark.parametrize("name", NAMES)
def test_secret_keys_with_fields_keygen_never_writes(name):
    k, l, eta = M.PARAMS[name][:3]
    low = eta - (2 ** M.bitlen(2 * eta) - 1)
    assert low == {2: -5, 4: -11}[eta]
    ks = E.odd_keys(name)
    dec = [M.sk_decode(sk, name) for sk in ks]
    assert dec[0][3][0][:8] == [low] * 8 and min(dec[0][3][0][8:]) >= -eta and all(min(p) >= -eta for p in dec[0][3][1:] + dec[0][4])
    assert dec[1][4][k - 1][-8:] == [low] * 8 and min(dec[1][4][k - 1][:-8]) >= -eta and all(min(p) >= -eta for p in dec[1][3] + dec[1][4][:-1])
    assert all(x == low for p in dec[2][3] + dec[2][4] for x in p)
    assert dec[0][5] == dec[1][5] == dec[2][5] and dec[0][:3] == dec[2][:3]
    inst = E.odd_sk(name)
    assert len(inst) == 18 and [sk for sk, _, _ in inst] == [ks[n // 6] for n in range(18)] and len({mu for _, mu, _ in inst}) == 18
    for sk, mu, rnd in inst:
        sig, attempts, fired = S.sign_trace(sk, name, mu=mu, rnd=rnd, max_attempts=E.MAX_ATTEMPTS)
        assert sig is not None and 1 <= attempts <= E.MAX_ATTEMPTS
        assert sig == M.sign_internal(sk, b"", rnd, name, mu=mu)


def test_the_instance_in_which_c_t0_fires():
    E.check()
    sk, mu, rnd = E.ct0_instance()
    rho, Kk, tr, s1, s2, t0 = M.sk_decode(sk, E.CT0_NAME)
    ref = M.sk_decode(M.keygen_internal(E.CT0_XI, E.CT0_NAME)[1], E.CT0_NAME)
    assert all(set(t0[r]) == {4096, -4095} for r in E.CT0_ROWS) and t0[2:] == ref[5][2:] and (rho, Kk, tr, s1, s2) == ref[:5]
    sig, attempts, fired = E.ct0_trace()
    assert sig == M.sign_internal(sk, b"", rnd, E.CT0_NAME, mu=mu) and attempts == len(fired) == 16
    assert len(E.ct0_instances()) == 3 and E.ct0_instances()[1] == (sk, mu, rnd) and len({m for _, m, _ in E.ct0_instances()}) == 3
    assert "no instance exercises" not in K.__doc__
