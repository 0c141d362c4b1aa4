"""check_domain on the device, decided as the reference decides it -- exact rationals (mp_perturbation.rs:396-402, gpv.rs:219-224, gpv_ring.rs:274-283) --
through the three ways a caller reaches k_check_domain: X_check_domain, the d_ok of X_f_a_dev and the PSF_ERR_DOMAIN status of the host X_f_a, for
PSFPerturbation (m = 121: less than one stride of the kernel; m = 537: three strides, a ragged last one), PSFGPV and PSFGPVRing.

Every expected value is a Python int / Fraction (tests/helpers/domain_cases.py); the CPU oracle is compared as well (GPU == oracle on every row), never used as
the expectation.  A device handle exists only for s r sqrt(m) < 2^23 (psfp_create: the int8 digit planes of the Z_q products), i.e. for bounds below 2^46:
  * what the kernel can get wrong there is covered here -- the rows on the bound in both directions, norms beyond 2^53, 2^64 and 2^128 (limb carries, the
    wrap of a 128-bit sum, -2^63), the largest bound a handle can have, a zero bound, other lengths, rows mixed in calls of at least 70;
  * bounds of 60-75 and 120-127 bits and B >= 2^128 cannot be installed in a device handle -- asserted below -- and are covered on the CPU: the limbs the
    kernel is handed (psf::domain_bound_exact) and the oracle's decision, tests/test_check_domain_exact_cpu.py."""
import math

import numpy as np
import pytest

from tests.helpers import domain_cases as dc

pytestmark = pytest.mark.gpu
KINDS = ["psfp-121", "psfp-537", "gpv", "ring"]


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Maker:
    """handles of one kind that share one public key (generated once): check_domain needs none, f_a needs A"""

    def __init__(self, T, oracle, kind):
        self.T, self.O, self.kind = T, oracle, kind
        self.r = 3.0 if kind.startswith("psfp") else 1.0
        self.n = {"psfp-121": 8, "psfp-537": 32, "gpv": 6, "ring": 8}[kind]
        h = self.device(200.0 if kind.startswith("psfp") else 25.0, self.r, key=False)      # (wide enough for Sigma_2 to be positive definite: A does not depend on s)
        if kind.startswith("psfp"):
            self.key = (h.trap_gen(seed=3)[0],)
            self.m = h.m
        elif kind == "gpv":
            A, (bt, gt) = h.trap_gen(seed=3)
            self.key = (A, bt, gt)
            self.m = h.m
        else:
            a, (r, e) = h.trap_gen(seed=3)
            self.key = (a, r, e)
            self.m = h.d
        h.close()

    def device(self, s, r, key=True):
        T = self.T
        if self.kind == "psfp-121":
            h = T.PSFPerturbation(T.GadgetParameters.init_default(8, 128), r, s)
        elif self.kind == "psfp-537":
            h = T.PSFPerturbation(T.GadgetParameters.init_default(32, 256), r, s)
        elif self.kind == "gpv":
            h = T.PSFGPV(T.GadgetParameters.init_default(6, 128), s)
        else:
            h = T.PSFGPVRing(T.GadgetParametersRing.init_default(8, 257), s, 1.005)
        if key:
            h.load_key(*self.key)
        return h

    def oracle(self, s, r):
        O = self.O
        if self.kind == "psfp-121":
            return O.PSFPerturbation(O.gadget_params_default(8, 128), r, s, with_L=False)
        if self.kind == "psfp-537":
            return O.PSFPerturbation(O.gadget_params_default(32, 256), r, s, with_L=False)
        if self.kind == "gpv":
            return O.PSFGPV(O.gadget_params_default(6, 128), s)
        return O.PSFGPVRing(O.gadget_params_ring_default(8, 257), s, 1.005)

    def shape(self, rows):
        """rows as the type's domain elements: B x m, or B x (k+2) x n polynomials"""
        return rows.reshape(rows.shape[0], -1, 8) if self.kind == "ring" else rows


_makers = {}


@pytest.fixture
def maker(T, oracle, request):
    kind = request.param
    if kind not in _makers:
        _makers[kind] = Maker(T, oracle, kind)
    return _makers[kind]


def all_paths(mk, torch, h, orc, rows, exp, what, singles):
    """rows: B x m int64; exp: the exact decisions.  check_domain in one call and row by row (`singles`), f_a_dev's d_ok, host f_a's status, the oracle."""
    from tools_amd._ffi import ERR_DOMAIN, PsfError
    B, m = rows.shape
    dom = mk.shape(rows)
    got = h.check_domain(dom)
    assert (got == exp).all(), f"{what}: check_domain rows {np.nonzero(got != exp)[0].tolist()[:8]} differ from the exact decision"
    assert (orc.check_domain(rows) == got).all(), f"{what}: GPU != oracle"
    for i in singles:
        assert bool(h.check_domain(dom[i])) == bool(exp[i]), f"{what}: single row {i}"
    # f_a_dev: d_ok
    d_e = torch.from_numpy(rows).cuda()
    d_u = torch.zeros((B, mk.n), dtype=torch.int64, device="cuda")
    d_ok = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    h.f_a_dev(d_e.data_ptr(), d_u.data_ptr(), d_ok.data_ptr(), B)
    torch.cuda.synchronize()
    ok = d_ok.cpu().numpy().astype(bool)
    assert (d_ok.cpu().numpy() <= 1).all() and (ok == exp).all(), f"{what}: f_a_dev d_ok rows {np.nonzero(ok != exp)[0].tolist()[:8]}"
    one = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    for i in singles:
        h.f_a_dev(d_e[i:i + 1].data_ptr(), d_u.data_ptr(), one.data_ptr(), 1)
        torch.cuda.synchronize()
        assert int(one.item()) == int(exp[i]), f"{what}: f_a_dev single row {i}"
    # host f_a: PSF_ERR_DOMAIN iff a row is outside
    h.f_a(mk.shape(rows[exp]))
    with pytest.raises(PsfError) as err:
        h.f_a(dom)
    assert err.value.status == ERR_DOMAIN
    for i in singles:
        if exp[i]:
            h.f_a(dom[i])
        else:
            with pytest.raises(PsfError) as err:
                h.f_a(dom[i])
            assert err.value.status == ERR_DOMAIN, f"{what}: f_a single row {i}"


@pytest.mark.parametrize("maker", KINDS, indirect=True)
def test_on_the_bound_in_both_directions(maker, torch):
    """at least 20 (K, s) of each kind per type: s where the rounded bound ((s*s)*m)*(r*r) admits floor(B) + 1, and s where it refuses floor(B);
    norms floor(B) - 34 ... floor(B) + 36 in one call of 71 rows, floor(B) + {-1, 0, 1, 2} as single rows too"""
    mk = maker
    m = mk.m
    rs = (3.0, 3.3, math.log2(6)) if mk.kind == "psfp-121" else (mk.r,)
    for r in rs:
        acc, rej = dc.on_the_bound_pairs(m, r, count=-(-20 // len(rs)))
        assert len(acc) * len(rs) >= 20 and len(rej) * len(rs) >= 20
        for s in acc + rej:
            h, orc = mk.device(s, r), mk.oracle(s, r)
            fb = dc.floor_bound(s, r, m)
            norms = dc.window_norms(fb)
            rows = dc.rows_array([dc.row_with_norm(N, m, salt=i) for i, N in enumerate(norms)])
            exp = dc.expected(norms, fb)
            all_paths(mk, torch, h, orc, rows, exp, f"{mk.kind} r={r!r} s={s!r}", [norms.index(fb + d) for d in (-1, 0, 1, 2)])
            h.close()


@pytest.mark.parametrize("maker", KINDS, indirect=True)
def test_norms_beyond_2_to_53_2_to_64_and_2_to_128_are_rejected(maker, torch):
    """B < 2^128 (every device handle): rows of norm 2^53 + 1 ... 2^128 + floor(B) ... m 2^126 are outside, mixed with the rows around the bound in one call.
    A 128-bit sum wraps 2^128 + floor(B) into the accepted range; a carry lost between limbs turns 2^64 into 0."""
    mk = maker
    s = 25.0
    h, orc = mk.device(s, mk.r), mk.oracle(s, mk.r)
    fb = dc.floor_bound(s, mk.r, mk.m)
    rows, exp, norms = dc.mixed_batch(fb, mk.m)
    huge = [i for i, N in enumerate(norms) if N >= 1 << 53]
    assert len(huge) >= 15 and not exp[huge].any()
    all_paths(mk, torch, h, orc, rows, exp, f"{mk.kind} s=25", huge + [norms.index(fb + d) for d in (-1, 0, 1, 2)])
    h.close()


@pytest.mark.parametrize("maker", KINDS, indirect=True)
def test_the_largest_bound_a_device_handle_can_have(maker, torch):
    """s r sqrt(m) just below 2^23: a 46-bit bound, the window around it and the carry / huge norms"""
    mk = maker
    s = math.nextafter(8388606.5 / (mk.r * math.sqrt(mk.m)), 0.0) * (1 - 2.0**-30)
    h, orc = mk.device(s, mk.r), mk.oracle(s, mk.r)
    fb = dc.floor_bound(s, mk.r, mk.m)
    assert fb.bit_length() == 46
    rows, exp, norms = dc.mixed_batch(fb, mk.m)
    all_paths(mk, torch, h, orc, rows, exp, f"{mk.kind} s={s!r}", [norms.index(fb + d) for d in (-1, 0, 1, 2)])
    h.close()


@pytest.mark.parametrize("maker", KINDS, indirect=True)
def test_larger_bounds_cannot_be_installed_on_the_device(maker):
    """bounds of 60-75 bits, 120-127 bits and >= 2^128: psfp_create refuses the handle (PSF_ERR_UNSUPPORTED), so no device decision exists to be wrong;
    tests/test_check_domain_exact_cpu.py decides these rows on the oracle and checks the limbs the kernel would be handed"""
    from tools_amd._ffi import ERR_UNSUPPORTED, PsfError
    for s in (2.0**30 + 0.37, 2.0**58, 2.0**62):
        with pytest.raises(PsfError) as err:
            maker.device(s, maker.r, key=False)
        assert err.value.status == ERR_UNSUPPORTED


@pytest.mark.parametrize("maker", KINDS, indirect=True)
def test_other_lengths_and_a_zero_bound(maker, torch):
    from tools_amd._ffi import ERR_DOMAIN, PsfError, lib
    import ctypes as C
    mk, m = maker, maker.m
    h = mk.device(25.0, mk.r)
    fn = {"psfp-121": "psfp_check_domain", "psfp-537": "psfp_check_domain", "gpv": "psfgpv_check_domain", "ring": "psfring_check_domain"}[mk.kind]
    for ln in (m - 1, m + 1, 1):
        rows = np.zeros((72, ln), dtype=np.int64)
        ok = np.full(72, 7, dtype=np.uint8)
        assert getattr(lib(), fn)(h._h, C.c_size_t(72), rows.ctypes.data_as(C.c_void_p), C.c_size_t(ln), ok.ctypes.data_as(C.c_void_p)) == 0
        assert not ok.any()
    assert h.check_domain(mk.shape(np.zeros((72, m), dtype=np.int64))).all()
    h.close()
    s = 2.0**-8                                       # s^2 m r^2 < 1: floor(B) = 0, the zero vector is the whole domain
    assert dc.floor_bound(s, mk.r, m) == 0
    h, orc = mk.device(s, mk.r), mk.oracle(s, mk.r)
    rows = np.zeros((72, m), dtype=np.int64)
    exp = np.ones(72, dtype=bool)
    for b in range(0, 72, 3):
        rows[b, (b * 7) % m] = 1 if b % 2 else -1
        exp[b] = False
    rows[69, m - 1], exp[69] = -2**63, False
    all_paths(mk, torch, h, orc, rows, exp, f"{mk.kind} zero bound", [0, 1, 69])
    h.close()
