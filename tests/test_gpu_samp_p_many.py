"""samp_p_dev_many: `count` independent samp_p_dev calls in one submission (include/psf_mi355x.h).  The nearest-plane types run the batches on two lanes of one
handle (two sets of per-batch buffers on two streams); PSFPerturbation runs them in order.  Whatever the schedule, the bytes are those of the loop of single
samp_p_dev calls, the call is ordered on the caller's stream, and last_status reports a sampler failure of any batch."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


def _torch():
    import torch
    return torch


def make(kind, oracle=None, seed=None):
    """the small keys of tests/test_gpu_np_forms.py (at least three 64-row blocks, a short top block)"""
    import tools_amd as T
    if kind == "gpv":
        n, q, s = 14, 2**9, 70.0
        psf = T.PSFGPV(T.GadgetParameters.init_default(n, q), s)
        A, (bt, gt) = psf.trap_gen(21 if seed is None else seed)
        d = psf.m
        orc = None
        if oracle is not None:
            orc = oracle.PSFGPV(oracle.gadget_params_default(n, q), s)
            assert orc.load_key(A, bt, gt) == 0
    else:
        n, q = 16, 3329
        s = ((2 * 2 * 1.005 * math.sqrt(n) + 1) * 2) * 4
        psf = T.PSFGPVRing(T.GadgetParametersRing.init_default(n, q), s, 1.005)
        psf.trap_gen(22 if seed is None else seed)
        d = psf.d
        orc = None
        if oracle is not None:
            a, r, e, bt, gt = psf.export_key()
            orc = oracle.PSFGPVRing(oracle.gadget_params_ring_default(n, q), s, 1.005)
            orc.load_key(a, r, e, gso_t=gt)
    return psf, orc, n, d


def targets(psf, rows, n, seed=9, stream=None):
    torch = _torch()
    u = torch.empty((rows, n), dtype=torch.int64, device="cuda")
    psf.uniform_targets_dev(u.data_ptr(), rows, seed=seed, first_index=0, stream=stream)
    return u


def loop(psf, u, B, d, seeds, firsts, stream=None):
    """the reference result: one samp_p_dev call per batch"""
    torch = _torch()
    e = torch.full((len(seeds) * B, d), -7, dtype=torch.int64, device="cuda")
    for i, (sd, fi) in enumerate(zip(seeds, firsts)):
        psf.samp_p_dev(u[i * B].data_ptr(), e[i * B].data_ptr(), B, seed=sd, first_index=fi, stream=stream)
    torch.cuda.synchronize()
    assert psf.last_status() == 0
    return e.cpu().numpy()


def many(psf, u, B, d, seeds, firsts, stream=None):
    torch = _torch()
    e = torch.full((len(seeds) * B, d), -7, dtype=torch.int64, device="cuda")
    psf.samp_p_dev_many(u.data_ptr(), e.data_ptr(), B, seeds, firsts, stream=stream)
    torch.cuda.synchronize()
    assert psf.last_status() == 0
    return e.cpu().numpy()


def seeds_firsts(count, base=40):
    return [base + 3 * i for i in range(count)], [777 * i + 3 for i in range(count)]


@pytest.mark.parametrize("kind,B,walk", [("gpv", 5, -1), ("gpv", 150, -1), ("gpv", 200, 0), ("gpv", 1000, 0),
                                         ("ring", 5, -1), ("ring", 150, -1), ("ring", 200, 0), ("ring", 1000, 0)])
def test_many_equals_the_loop_of_single_calls_and_the_oracle(oracle, kind, B, walk):
    psf, orc, n, d = make(kind, oracle)
    psf._debug_set_walk(walk)
    u = targets(psf, 5 * B, n)
    u_host = u.cpu().numpy().astype(np.uint64)
    for count in (1, 2, 3, 5):
        seeds, firsts = seeds_firsts(count)
        ref = loop(psf, u, B, d, seeds, firsts)
        got = many(psf, u, B, d, seeds, firsts)
        assert (got == ref).all(), (kind, B, count)
        form = psf.nearest_plane_form()
        assert form[0] == (1 if walk == -1 else 0), form
        assert form[3] == 0                                   # no walk was re-run on an idle device
        for i in sorted({0, count - 1}):                     # first and last row of two batches against the oracle
            for r in (0, B - 1):
                row = np.asarray(orc.samp_p(seeds[i], u_host[i * B + r:i * B + r + 1], first_index=firsts[i] + r)).reshape(-1, d)      # (the ring oracle: k+2 polynomials)
                assert (got[i * B + r] == row[0]).all(), (count, i, r)
    psf.close()


def test_two_pass_walk_and_generic_recombination(T, oracle):
    """the large-modulus key of test_gpu_gpv_parity.py::test_large_modulus (two passes: e1 and its centres are per lane) and the keys of
    test_recombination_in_64_bit_integers_when_the_digit_planes_do_not_fit (the 64-bit recombination, decided at load_key or on the device per batch)"""
    seeds, firsts = seeds_firsts(3, base=11)
    n, q, s = 3, 2**45, 60.0
    psf = T.PSFGPV(T.GadgetParameters.init_default(n, q), s)
    assert psf.two_pass
    psf.trap_gen(9)
    u = targets(psf, 3 * 5, n, seed=3)
    assert (many(psf, u, 5, psf.m, seeds, firsts) == loop(psf, u, 5, psf.m, seeds, firsts)).all()
    psf.close()

    n, q, s = 6, 128, 40.0
    gp = T.GadgetParameters.init_default(n, q)
    base = T.PSFGPV(gp, s)
    A, (bt, gt) = base.trap_gen(5)
    bt2 = bt.copy()
    bt2[-1] = bt[-1] + 40000 * bt[-2]
    big = T.PSFGPV(gp, s)
    big.load_key(A, bt2, oracle.gso_rows(bt2))
    wide = T.PSFGPV(gp, 400000.0)
    wide.load_key(A, bt, gt)
    for psf in (big, wide):
        u = targets(psf, 3 * 7, n, seed=2)
        ref = loop(psf, u, 7, psf.m, seeds, firsts)
        got = many(psf, u, 7, psf.m, seeds, firsts)
        assert (got == ref).all()
        assert psf.nearest_plane_stats()[1] == 1
        A_o = A.astype(object)
        assert ((A_o @ got.astype(object).T).T % q == u.cpu().numpy().astype(object)).all()
    for psf in (base, big, wide):
        psf.close()


@pytest.mark.parametrize("kind,B,walk", [("gpv", 150, -1), ("ring", 200, 0)])
def test_ordered_on_a_non_default_stream(kind, B, walk):
    """targets, the many-call and f_a over every row enqueued on one side stream without a host synchronisation between them"""
    torch = _torch()
    psf, _, n, d = make(kind)
    psf._debug_set_walk(walk)
    count = 4
    seeds, firsts = seeds_firsts(count)
    rows = count * B
    u = torch.empty((rows, n), dtype=torch.int64, device="cuda")
    e = torch.full((rows, d), -7, dtype=torch.int64, device="cuda")
    u2 = torch.full((rows, n), -1, dtype=torch.int64, device="cuda")
    ok = torch.zeros(rows, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    st = side.cuda_stream
    psf.uniform_targets_dev(u.data_ptr(), rows, seed=9, first_index=0, stream=st)
    psf.samp_p_dev_many(u.data_ptr(), e.data_ptr(), B, seeds, firsts, stream=st)
    psf.f_a_dev(e.data_ptr(), u2.data_ptr(), ok.data_ptr(), rows, stream=st)
    side.synchronize()
    assert psf.last_status() == 0
    assert bool((ok == 1).all())
    assert torch.equal(u2, u)
    again = many(psf, u, B, d, seeds, firsts)
    assert (e.cpu().numpy() == again).all()
    psf.close()


@pytest.mark.parametrize("kind,B,walk", [("gpv", 150, -1), ("ring", 200, 0)])
def test_interleaved_with_single_and_asynchronous_calls(kind, B, walk):
    torch = _torch()
    psf, _, n, d = make(kind)
    psf._debug_set_walk(walk)
    seeds, firsts = seeds_firsts(3)
    u = targets(psf, 5 * B, n)
    single = [loop(psf, u[3 * B:], B, d, [70], [5]), loop(psf, u[4 * B:], B, d, [71], [9])]
    batches = loop(psf, u, B, d, seeds, firsts)
    ea = torch.full((B, d), -7, dtype=torch.int64, device="cuda")
    eb = torch.full((3 * B, d), -7, dtype=torch.int64, device="cuda")
    ec = torch.full((B, d), -7, dtype=torch.int64, device="cuda")
    psf.samp_p_dev(u[3 * B].data_ptr(), ea.data_ptr(), B, seed=70, first_index=5)
    psf.samp_p_dev_many(u.data_ptr(), eb.data_ptr(), B, seeds, firsts)
    psf.samp_p_dev(u[4 * B].data_ptr(), ec.data_ptr(), B, seed=71, first_index=9)
    torch.cuda.synchronize()
    assert psf.last_status() == 0
    assert (ea.cpu().numpy() == single[0]).all() and (eb.cpu().numpy() == batches).all() and (ec.cpu().numpy() == single[1]).all()
    # an asynchronous host-pointer call in flight, then a many-call: the many-call drains it first
    u_host = u[3 * B:4 * B].cpu().numpy().astype(np.uint64)
    out = np.full((B, psf.K, psf.n) if kind == "ring" else (B, d), -7, dtype=np.int64)      # (the ring type's rows: k+2 polynomials)
    psf.samp_p_async(u_host, out, seed=70, first_index=5)
    eb.fill_(-7)
    psf.samp_p_dev_many(u.data_ptr(), eb.data_ptr(), B, seeds, firsts)
    psf.wait()
    torch.cuda.synchronize()
    assert psf.last_status() == 0
    assert (out.reshape(B, d) == single[0]).all() and (eb.cpu().numpy() == batches).all()
    psf.close()


def test_two_handles_on_two_streams():
    """two handles with the same key, each a many-call of four one-launch walks on its own stream at once: the walks of both handles' lanes take turns (WalkTurn)"""
    torch = _torch()
    B, count = 150, 4
    hs = [make("gpv")[0] for _ in range(2)]
    n, d = 14, hs[0].m
    seeds, firsts = seeds_firsts(count)
    u = targets(hs[0], count * B, n)
    refs = [loop(h, u, B, d, [s + 100 * j for s in seeds], firsts) for j, h in enumerate(hs)]
    outs = [torch.full((count * B, d), -7, dtype=torch.int64, device="cuda") for _ in hs]
    streams = [torch.cuda.Stream() for _ in hs]
    torch.cuda.synchronize()
    for j, h in enumerate(hs):
        h.samp_p_dev_many(u.data_ptr(), outs[j].data_ptr(), B, [s + 100 * j for s in seeds], firsts, stream=streams[j].cuda_stream)
    torch.cuda.synchronize()
    for j, h in enumerate(hs):
        assert h.last_status() == 0
        assert h.nearest_plane_form()[0] == 1
        assert (outs[j].cpu().numpy() == refs[j]).all()
        h.close()


def test_status_of_the_call(T):
    import ctypes as C
    from tools_amd._ffi import lib, ERR_PARAM, ERR_NO_KEY
    torch = _torch()
    psf, _, n, d = make("gpv")
    B = 5
    u = targets(psf, 2 * B, n)
    e = torch.full((2 * B, d), -7, dtype=torch.int64, device="cuda")
    sd = (C.c_uint64 * 2)(1, 2)
    fi = (C.c_uint64 * 2)(0, 5)
    f = lib().psfgpv_samp_p_dev_many
    assert f(psf._h, C.c_size_t(0), None, None, C.c_size_t(B), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == 0
    assert f(psf._h, C.c_size_t(2), sd, fi, C.c_size_t(0), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == 0
    assert f(psf._h, C.c_size_t(2), None, fi, C.c_size_t(B), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == ERR_PARAM
    assert f(psf._h, C.c_size_t(2), sd, None, C.c_size_t(B), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == ERR_PARAM
    assert f(psf._h, C.c_size_t(2), sd, fi, C.c_size_t(B), None, C.c_void_p(e.data_ptr()), None) == ERR_PARAM
    torch.cuda.synchronize()
    assert bool((e == -7).all())                                # nothing was enqueued
    fresh = T.PSFGPV(T.GadgetParameters.init_default(14, 2**9), 70.0)
    assert lib().psfgpv_samp_p_dev_many(fresh._h, C.c_size_t(2), sd, fi, C.c_size_t(B), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == ERR_NO_KEY
    ring = T.PSFGPVRing(T.GadgetParametersRing.init_default(16, 3329), 40.0, 1.005)
    assert lib().psfring_samp_p_dev_many(ring._h, C.c_size_t(2), sd, fi, C.c_size_t(B), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == ERR_NO_KEY
    pp = T.PSFPerturbation(T.GadgetParameters.init_default(8, 64), 3.0, 25.0)
    assert lib().psfp_samp_p_dev_many(pp._h, C.c_size_t(2), sd, fi, C.c_size_t(B), C.c_void_p(u.data_ptr()), C.c_void_p(e.data_ptr()), None) == ERR_NO_KEY
    with pytest.raises(T.PsfError):
        psf.samp_p_dev_many(u.data_ptr(), e.data_ptr(), B, [1, 2], [0])      # seeds and first indices of different lengths
    for h in (psf, fresh, ring, pp):
        h.close()


GIVE_UP = r'''
import sys, json
sys.path.insert(0, %r)
import torch
import tools_amd as T
psf = T.PSFGPV(T.GadgetParameters.init_default(14, 2**9), 70.0)
psf.trap_gen(21)
B, count = 150, 3
u = torch.empty((count * B, 14), dtype=torch.int64, device="cuda")
e = torch.empty((count * B, psf.m), dtype=torch.int64, device="cuda")
psf.uniform_targets_dev(u.data_ptr(), count * B, seed=9)
psf.samp_p_dev_many(u.data_ptr(), e.data_ptr(), B, [1, 2, 3], [0, 500, 1000])
torch.cuda.synchronize()
print(json.dumps({"status": int(psf.last_status())}))
''' % ROOT


def test_a_wait_that_gives_up_in_a_many_call_reports_a_sampler_failure():
    """experiments build, PSF_NP_WALK=3 with PSF_NP_WALK_SPINS=1: the software give-up of test_gpu_np_forms.py::test_a_wait_that_gives_up_reports_a_sampler_failure,
    here inside a many-call: last_status reports it (status 9)"""
    import json
    from tests.conftest import exp_env
    env = exp_env(PSF_NP_WALK="3", PSF_NP_WALK_SPINS="1")
    r = subprocess.run([sys.executable, "-c", GIVE_UP], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["status"] == 9


@pytest.mark.parametrize("n,q,r,s,B", [(8, 64, 3.0, 25.0, 6), (64, 128, 6.0, 100.0, 17), (64, 128, 6.0, 100.0, 64)])
def test_psfp_many_equals_the_loop(T, n, q, r, s, B):
    psf = T.PSFPerturbation(T.GadgetParameters.init_default(n, q), r, s)
    psf.trap_gen(seed=1)
    u = targets(psf, 3 * B, n, seed=7)
    seeds, firsts = seeds_firsts(3, base=42)
    ref = loop(psf, u, B, psf.m, seeds, firsts)
    got = many(psf, u, B, psf.m, seeds, firsts)
    assert (got == ref).all()
    assert psf.check_domain(got).all()
    assert (psf.f_a(got) == u.cpu().numpy().astype(np.uint64)).all()
    psf.close()


def test_full_size_c4_shape():
    """bench.py's c4 shape (PSFGPVRing n = 256, q = 3329, 4096 preimages, key seed 3, targets of seed 7): two batches, the rows of the loop, every row in the domain"""
    import ctypes as C
    import tools_amd as T
    from tools_amd._ffi import lib, check
    n, q, B = 256, 3329, 4096
    s = ((2 * 2 * 1.005 * math.sqrt(n) + 1) * 2) * 4
    psf = T.PSFGPVRing(T.GadgetParametersRing.init_default(n, q), s, 1.005)
    check(lib().psfring_trap_gen(psf._h, C.c_uint64(3)), "trap_gen")
    d = psf.d
    u = targets(psf, 2 * B, n, seed=7)
    seeds, firsts = [1000, 1001], [0, B]
    ref = loop(psf, u, B, d, seeds, firsts)
    got = many(psf, u, B, d, seeds, firsts)
    assert (got == ref).all()
    assert psf.check_domain(got.reshape(2 * B, psf.K, n)).all()
    psf.close()
