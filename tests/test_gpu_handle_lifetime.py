"""A handle owns its device memory, pinned buffers, streams and events, and gives all of them back when it is closed.

One cycle = create, trap_gen, every call form that allocates lazily (the small-call buffer and the compact copies, growing batch buffers, both slots of the
host-pointer transport, lane 1 and the lane streams of a many-call, f_a / check_domain / samp_d, timing events), close().  Tiny keys, at most 130 preimages.
  1. the rows of the first and of the last cycle are bit-identical, and A e = u / check_domain hold: a handle on recycled memory behaves as a fresh one;
  2. after a warm-up cycle (the runtime's own pools exist), N = 6 further cycles leave free device memory no more than F / 2 below where it was, F being what
     ONE live handle holds after all the calls: a cycle that leaks a twelfth of a handle fails, one that leaks nothing has F / 2 to spare against other users
     of the card.  A gross-leak check (a lost flag array is below the allocator's granularity); tests/cpp/owned_check.cpp and test_release_sites_cpu.py hold
     the fine grain;
  3. close() with two asynchronous calls in flight and no wait() returns, and the callers' buffers are complete: the transport is joined before anything
     its calls read is released (psfp_destroy, psfgpv_destroy)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CYCLES = 6
B_MANY = 40                                                   # three batches of a many-call: 120 preimages


def _perturbation(T, structured=False):
    return T.PSFPerturbation(T.GadgetParameters.init_default(8, 64), 3.0, 25.0, structured=structured), 8, 64


CONFIGS = {
    "perturbation": lambda T: _perturbation(T),
    "perturbation-structured": lambda T: _perturbation(T, True),
    "gpv": lambda T: (T.PSFGPV(T.GadgetParameters.init_default(14, 2**9), 70.0), 14, 2**9),
    "gpv-two-pass": lambda T: (T.PSFGPV(T.GadgetParameters.init_default(3, 2**45), 60.0), 3, 2**45),
    "ring": lambda T: (T.PSFGPVRing(T.GadgetParametersRing.init_default(16, 3329), ((2 * 2 * 1.005 * math.sqrt(16) + 1) * 2) * 4, 1.005), 16, 3329),
}


@pytest.fixture(scope="module")
def T():
    import tools_amd
    return tools_amd


def _free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


class _Work:
    """What the cycles of one configuration share: targets on the host, targets and rows on the device (allocated once, before the first reading)."""

    def __init__(self, T, oracle, torch, name):
        self.T, self.torch, self.make = T, torch, CONFIGS[name]
        h, self.n, self.q = self.make(T)
        self.row = (h.K, h.n) if isinstance(h, T.PSFGPVRing) else (h.m,)
        h.close()
        self.u = oracle.uniform_targets(21, 130, self.n, self.q)
        dev = torch.device("cuda", 0)
        self.d_u = torch.from_numpy(oracle.uniform_targets(22, 3 * B_MANY, self.n, self.q).astype(np.int64)).to(dev)
        self.d_e = torch.zeros((3 * B_MANY,) + self.row, dtype=torch.int64, device=dev)
        self.u_many = self.d_u.cpu().numpy().astype(np.uint64)

    def cycle(self, live=None):
        """One handle from create to close(); `live()` runs while it still holds everything.  Returns the rows of every call, in order."""
        T, torch = self.T, self.torch
        h, _, _ = self.make(T)
        h.trap_gen(seed=3)
        u = self.u
        got = [h.samp_p(u[:1], seed=40)]                                       # the small-call buffer, the compact copies
        got.append(h.samp_p(u[:70], seed=41, first_index=7))                   # the batch buffers ...
        got.append(h.samp_p(u, seed=42, first_index=9))                        # ... grow
        outs = [np.full((B,) + self.row, -7, dtype=np.int64) for B in (70, 130)]
        h.samp_p_async(u[:70], outs[0], seed=41, first_index=7)                # both transport slots
        h.samp_p_async(u, outs[1], seed=42, first_index=9)
        h.wait()
        got += outs
        h.samp_p_dev_many(self.d_u.data_ptr(), self.d_e.data_ptr(), B_MANY, [50, 51, 52], [0, 100, 200], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()                                               # lane 1 and the lane streams (nearest-plane types)
        got.append(self.d_e.cpu().numpy().copy())
        got.append(h.f_a(got[2]))
        got.append(np.asarray(h.check_domain(got[2])))
        got.append(h.samp_d(seed=60, B=5))
        if isinstance(h, T.PSFPerturbation):
            h.enable_timing(True)
            got.append(h.samp_p(u[:70], seed=41, first_index=7))
            assert h.get_timing()
            h.enable_timing(False)
        if live:
            live()
        h.close()
        return got

    def check(self, got):
        assert (got[3] == got[1]).all() and (got[4] == got[2]).all(), "asynchronous rows differ from the synchronous ones"
        assert (got[6] == self.u).all(), "A e != u"
        assert got[7].all(), "preimage outside the domain"
        h, _, _ = self.make(self.T)                                            # (a verifier's view of the many-call: same key, f_a only)
        h.trap_gen(seed=3)
        assert (h.f_a(got[5]) == self.u_many).all(), "A e != u (many-call)"
        h.close()
        if len(got) > 9:
            assert (got[9] == got[1]).all(), "timing changed the rows"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_cycles_return_the_same_rows_and_the_device_memory(T, oracle, name):
    import torch
    w = _Work(T, oracle, torch, name)
    first = w.cycle()                                                           # warm-up: the runtime's pools, the code objects, torch's context
    w.check(first)
    before = _free_bytes(torch)
    held = []
    last = w.cycle(live=lambda: held.append(before - _free_bytes(torch)))      # F: what one live handle holds after all its calls
    for _ in range(N_CYCLES - 1):
        last = w.cycle()
    after = _free_bytes(torch)
    F, drop = held[0], before - after
    print(f"HANDLE_LIFETIME {name}: F = {F} bytes held by one live handle, free memory {drop} bytes lower after {N_CYCLES} cycles")
    assert len(first) == len(last)
    for i, (a, b) in enumerate(zip(first, last)):
        assert a.shape == b.shape and (a == b).all(), f"call {i} of the last cycle differs from the first cycle's"
    w.check(last)
    assert drop <= F / 2, (name, F, drop)


@pytest.mark.parametrize("name", ["perturbation", "gpv"])
def test_close_with_asynchronous_calls_in_flight_completes_their_rows(T, oracle, name):
    h, n, q = CONFIGS[name](T)
    h.trap_gen(seed=3)
    u = oracle.uniform_targets(23, 130, n, q)
    want = [h.samp_p(u[:70], seed=71, first_index=5), h.samp_p(u, seed=72, first_index=6)]
    outs = [np.full((B, h.m), -7, dtype=np.int64) for B in (70, 130)]
    h.samp_p_async(u[:70], outs[0], seed=71, first_index=5)
    h.samp_p_async(u, outs[1], seed=72, first_index=6)
    h.close()                                                                   # no wait(): destroy joins both slots' workers first
    assert (outs[0] == want[0]).all() and (outs[1] == want[1]).all()
