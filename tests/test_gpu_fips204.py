"""The stages of ML-DSA on the MI355X (tools_amd/fips204.py, psf_sample_*_fips204*, psf_ntt_image_from_fips204*) against the pure-Python model: the three
rejection samplers byte for byte (counts 1, 3 and 67, so that a wave holds lanes that finish in different blocks: the searched seeds of
tests/helpers/mldsa_cases.py are among them), and the NTT-domain interop through the library's own products at (8380417, 256).  Outputs sit between
guard words; the sampler flag stays as it was."""
import random

import numpy as np
import pytest

from tests.helpers import mldsa_cases as K
from tests.helpers import mldsa_model as M

pytestmark = pytest.mark.gpu
Q, N = M.Q, 256
GUARD, FILL = 64, 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def F():
    import tools_amd
    return tools_amd.fips204


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _seeds(torch, rows, off=1):
    """the rows packed on the device, the first byte `off` bytes past a 16-byte boundary"""
    data = np.frombuffer(b"".join(rows), dtype=np.uint8)
    buf = torch.zeros((16 + data.size + off,), dtype=torch.uint8, device="cuda")
    buf[off:off + data.size] = torch.from_numpy(data.copy())
    return buf, buf.data_ptr() + off


def _words(torch, n):
    """n 64-bit output words between guard words, and a flag that starts at 4"""
    buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.int64, device="cuda")
    flag = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    return buf, buf.data_ptr() + 8 * GUARD, flag


def _taken(torch, buf, n, flag):
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + n:] == FILL).all(), "wrote outside the output"
    assert int(flag.item()) == 4, "the sampler flag changed"
    return host[GUARD:GUARD + n].reshape(-1, N).tolist()


@pytest.mark.parametrize("count", [1, 3, 67])
def test_sample_ntt_raw_form(F, torch, count):
    rng = random.Random(100 + count)
    seeds = [rng.randbytes(34) for _ in range(count)]
    for at, s in zip((0, 40), K.NTT_REJECTS_FIRST_AND_LAST):               # both in the first wave of the batch of 67
        if at < count:
            seeds[at] = s
    bs, ps = _seeds(torch, seeds)
    buf, po, flag = _words(torch, count * N)
    F.sample_ntt_dev(po, count, ps, d_fail=flag.data_ptr())
    assert _taken(torch, buf, count * N, flag) == [M.rej_ntt_poly(s) for s in seeds]
    assert F.sample_ntt(np.frombuffer(b"".join(seeds), np.uint8).reshape(count, 34)).tolist() == [M.rej_ntt_poly(s) for s in seeds]


@pytest.mark.parametrize("count", [1, 3, 67])
@pytest.mark.parametrize("k,l", [(4, 4), (6, 5), (8, 7)])
def test_sample_ntt_matrix_form(F, torch, k, l, count):
    rng = random.Random(200 + 10 * k + count)
    rhos = [rng.randbytes(32) for _ in range(count)]
    stride = 45                                                            # seeds apart from each other, at odd addresses
    bs, ps = _seeds(torch, [r + bytes(stride - 32) for r in rhos])
    buf, po, flag = _words(torch, count * k * l * N)
    F.sample_ntt_dev(po, count, ps, k=k, l=l, seed_stride=stride, d_fail=flag.data_ptr())
    want = [p for r in rhos for row in M.expand_a(r, k, l) for p in row]
    assert _taken(torch, buf, count * k * l * N, flag) == want


@pytest.mark.parametrize("count", [1, 3, 67])
@pytest.mark.parametrize("eta", [2, 4])
def test_sample_bounded(F, torch, eta, count):
    rng = random.Random(300 + eta + count)
    seeds = [rng.randbytes(64) for _ in range(count)]
    special = (K.BOUNDED2_ONE_BLOCK, K.BOUNDED2_TWO_BLOCKS) if eta == 2 else (K.BOUNDED4_THREE_BLOCKS, K.BOUNDED4_TWO_BLOCKS)
    for at, s in zip((0, 20), special):
        if at < count:
            seeds[at] = s
    bs, ps = _seeds(torch, seeds)
    for first, per in ((0, 3), (5, 1), (65533, 3)):
        buf, po, flag = _words(torch, count * per * N)
        F.sample_bounded_dev(po, count, ps, eta, first_nonce=first, per_seed=per, d_fail=flag.data_ptr())
        want = [M.rej_bounded_poly(s + (first + t).to_bytes(2, "little"), eta) for s in seeds for t in range(per)]
        assert _taken(torch, buf, count * per * N, flag) == want, (eta, count, first, per)
    got = F.sample_bounded(np.frombuffer(b"".join(seeds), np.uint8).reshape(count, 64), eta, first_nonce=0, per_seed=2)
    assert got.reshape(-1, N).tolist() == [M.rej_bounded_poly(s + bytes([t, 0]), eta) for s in seeds for t in range(2)]


@pytest.mark.parametrize("count", [1, 3, 67])
@pytest.mark.parametrize("tau,length", [(39, 32), (49, 48), (60, 64)])
def test_sample_in_ball(F, torch, tau, length, count):
    rng = random.Random(400 + tau + count)
    cts = [rng.randbytes(length) for _ in range(count)]
    stride = length + 3
    bs, ps = _seeds(torch, [c + bytes(3) for c in cts])
    buf, po, flag = _words(torch, count * N)
    F.sample_in_ball_dev(po, count, ps, tau, length, ctilde_stride=stride, d_fail=flag.data_ptr())
    want = [M.sample_in_ball(c, tau) for c in cts]
    assert all(sum(1 for v in p if v) == tau and set(p) <= {-1, 0, 1} for p in want)
    assert _taken(torch, buf, count * N, flag) == want
    assert F.sample_in_ball(np.frombuffer(b"".join(cts), np.uint8).reshape(count, length), tau).tolist() == want


def test_image_from_multiplies_like_the_model(F, torch):
    """poly_mul_hat_dev over from(NTT(f)) equals the model's negacyclic f b; with b = 1 it returns f"""
    import tools_amd
    rng = random.Random(500)
    count = 5
    f = [[rng.randrange(Q) for _ in range(N)] for _ in range(count)]
    b = [[rng.randrange(-(1 << 19), 1 << 19) for _ in range(N)] for _ in range(count - 1)] + [[1] + [0] * 255]
    fhat = np.array([M.ntt(p) for p in f], dtype=np.uint64)
    fhat[1] += np.uint64(Q) * np.uint64(12345)                             # any 64-bit value, read mod q
    d_fhat = torch.from_numpy(fhat.view(np.int64)).cuda()
    d_hat = torch.full((count * N + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    F.image_from_fips204_dev(d_hat.data_ptr() + 4 * GUARD, count, d_fhat.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_hat[:GUARD] == 0x5A5A5A5A).all().item()) and bool((d_hat[GUARD + count * N:] == 0x5A5A5A5A).all().item())
    d_b = torch.tensor(b, dtype=torch.int64, device="cuda")
    d_out = torch.zeros((count, N), dtype=torch.int64, device="cuda")
    tools_amd.gadget.poly_mul_hat_dev(d_hat.data_ptr() + 4 * GUARD, N, d_b.data_ptr(), d_out.data_ptr(), Q, N, count)
    torch.cuda.synchronize()
    got = d_out.cpu().tolist()
    assert got == [M.schoolbook(p, [x % Q for x in c]) for p, c in zip(f, b)]
    assert got[-1] == f[-1]
    host = F.image_from_fips204(fhat)
    assert (host == d_hat[GUARD:GUARD + count * N].cpu().numpy().view(np.uint32).reshape(count, N)).all()
    assert sorted(int(v) for v in host[0]) == sorted(M.ntt(f[0]))          # a permutation of the residues


@pytest.mark.parametrize("k,l", [(4, 4), (6, 5), (8, 7)])
def test_sampled_matrix_as_operand_of_the_matrix_product(F, torch, k, l):
    """from(sample_ntt(rho)) as A of matpoly_mul_hat_dev with rows = k and inner = l equals the model's A_hat o s_hat transformed back"""
    import tools_amd
    rng = random.Random(600 + k)
    count = 3
    rhos = [rng.randbytes(32) for _ in range(count)]
    s = [[[rng.randrange(-4, 5) for _ in range(N)] for _ in range(l)] for _ in range(count)]
    bs, ps = _seeds(torch, rhos)
    d_a = torch.zeros((count * k * l * N,), dtype=torch.int64, device="cuda")
    F.sample_ntt_dev(d_a.data_ptr(), count, ps, k=k, l=l)
    d_hat = torch.zeros((count * k * l * N,), dtype=torch.int32, device="cuda")
    F.image_from_fips204_dev(d_hat.data_ptr(), count * k * l, d_a.data_ptr())
    d_s = torch.tensor(s, dtype=torch.int64, device="cuda")
    d_c = torch.zeros((count, k, N), dtype=torch.int64, device="cuda")
    tools_amd.rq.matpoly_mul_hat_dev(d_hat.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), Q, N, count, k, l, 1, hat_stride=k * l * N)
    torch.cuda.synchronize()
    want = [[M.ntt_inv(p) for p in M.mat_vec_hat(M.expand_a(r, k, l), [M.ntt(x) for x in sv])] for r, sv in zip(rhos, s)]
    assert d_c.cpu().tolist() == want
