"""Every launch form of PSFPerturbation::samp_p at the full-size key, against the oracle.

plan_samp_p / plan_zq (tools_amd/csrc/psfp.hip) choose per call, from the batch size B and the key's shape, a product form, a normals layout, a rounding kernel, a Z_q
form, a gadget walk and a recombination.  The choices switch on m and B together (h->mL < 16384, n B, K_pad), so small keys do not reproduce what the C3 shape
(n = 512, q = 2^30, m = 30 801) runs.  This module asks the handle which plan it would take (psfp_query_plan) for every B from 1 to 4352, takes both sides of every
B where a field of the plan changes, adds a fixed list that does not depend on the planner, and checks every such size:

  1. the executed plan (psfp_get_last_plan) equals the queried plan;
  2. every row: f_a(e) == u and check_domain(e) on the device, last_status() == 0;
  3. every row, bit for bit: the batch equals the same rows computed 16 at a time (first_index + 16 j);
  4. a sample of 8 ... 11 rows per size (row 0, B - 1, B // 2, both sides of the last multiple of 16, 64, 128 and 256 below B, filled up to 8) against the oracle from
     scratch: oracle.normals, the centres through oracle.centres_rows over ALL 2048-row blocks of the exported factor (each block exported once per test and every
     sampled row pushed through it before the next), then samp_p_from_x; for B <= 256 also the staged d, x, p, v, z of samp_p_stages, so a failure names its stage.

STALE DATA MUST NOT PASS.  Device buffers are reused between calls, and a kernel that skips the stores of a ragged tile leaves the previous call's values, which are
right by accident if that call computed the same rows at the same positions.  The rule of this module: NO COMPARED CALL DIRECTLY FOLLOWS A CALL THAT LEFT THE SAME VALUES
AT THE SAME POSITIONS.  Every size has its own seed (1000 + B) and first_index; the 16-row reference calls of a size run first (consecutive ones differ in first_index,
so in every value); then one call of B preimages with ANOTHER seed, checked by item 2 only; then the compared batch.  The staged call of a size up to 256 preimages is
again preceded by a call with a third seed.  Every output tensor is filled with a sentinel before the call that writes it.

ORDER ON THE HANDLE.  The list runs ascending on a fresh handle (buffers grow with the batch: ensure_batch), then descending on the same handle (buffers of the largest
batch: other leading dimensions and split caps).  The passes must agree bit for bit; the first is the one compared with the oracle.  After the ascending pass the compact
key copies exist, so the descending pass must report tail == 1 and recombine == R_SMALL2 at one and two preimages.  syn.form == SMALL32 is asserted in the ASCENDING
pass, at one preimage, where the compared batch waits for the copies: plan_zq gives SMALL32 to one preimage only (small_max), and only while its ceil(m / 2048) splits fit
the handle's split cap -- FOUND BY THIS SWEEP: at C3 a handle that has served more than 4096 preimages has a cap of 15 against 16 splits and plans MFMA for one preimage
(no launch reads the field then: behind the fused tail no syndrome stage runs; the rows are the oracle's either way).  The first call of one and of two preimages on
the fresh handle runs without the copies (SMALL, R_SMALL, tail 0) and is recorded as well.  The copies are packed in the
background and the query changes nothing on the handle: a handle learns that they are complete in a call of at most four preimages, so the test asks the query, makes
such a call with a seed of its own and asks again, a bounded number of times.

THINNING.  Fields that do not name a kernel (ncg, syn.splits, gq_p, rsplits, ...) step often over 1 ... 4352.  For such a field with more than eight steps the list
keeps its first, its last and every fourth step.  one_launch, product, tail, round, syn.form, gadget and recombine are never thinned; `round` alone alternates at every
multiple of 64 from 1024 on (ROUND_TAB_ROW), which is most of the list.

COVERAGE is asserted at the end of the C3 leg: every enumerator of product (BIG with both super-tiles), round, syn.form, gadget and recombine that these keys can reach
(UNREACHABLE names the others and why), and tail 0 / 1.

The tests of a leg share one key and one handle and run in file order; each stays far from the 600 s ceiling of tests/conftest.py.

Measured on an MI355X (profiles/plan_sweep_run1.log; MEASURED below): C3 214 sizes (445 625 rows a pass) in 125 s, 75 s of them the oracle, the slowest single test
19.5 s; C3' 31 sizes in 14 s (oracle 10 s); the small factor 88 sizes in 11 s (oracle 9 s, every row); the module 162 s.
"""
import os
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizes per leg, wall time per leg and the oracle's share (seconds), from profiles/plan_sweep_run1.log
MEASURED = {      # one MI355X, one run; seconds of wall time
    "C3": dict(sizes=214, rows=445625, leg=124.9, oracle=74.5, key_and_list=11.6, slowest_test=19.5),
    "C3'": dict(sizes=31, rows=28961, leg=13.9, oracle=10.0),
    "small factor": dict(sizes=88, rows=130665, leg=10.9, oracle=9.4),
    "whole module": 162.5,
}

B_MAX = 4352
EDGES = (4, 16, 20, 32, 64, 96, 128, 192, 256, 320, 448, 960, 1024, 1088, 1472, 1536, 1728, 2048, 4096)      # both sides of each: B and B + 1
RAGGED = (100, 150, 333, 1000, 1100, 1500, 1601, 1801, 2177, 3201, 4160, 4224)
NEVER_THINNED = ("one_launch", "product", "tail", "round", "syn.form", "gadget", "recombine")
SENTINEL = 0x5555555555555555
PARTS = 4                      # tests per pass of the C3 leg
STAGES = ("d", "x", "p", "v", "z", "e")

# enumerators no leg of this module can reach, and why
UNREACHABLE = {
    "gadget": {"G_LOCKSTEP": "taken only when the handle has no queue tables (PSF_GADGET_QUEUE=0 of the experiments build)"},
    "round": {"ROUND_LEAN": "the table screen exists for every parameter set with a 16-bit rounding sampler; the fp32 screen is an experiments arm (PSF_ROUND=lean)",
              "ROUND_WAVE": "the round-2 kernel: the experiments arm PSF_ROUND=wave, or a rounding sampler that is not 16-bit"},
    "one_launch": {1: "needs m <= 256 and n <= 64; covered by test_fused_one_launch_call_gives_the_oracles_rows"},
}


# ---- which sizes -------------------------------------------------------------------------------------------------------------------------------------------------
def fixed_sizes(b_max=B_MAX):
    """The sizes that do not depend on the planner: a broken query cannot empty the sweep."""
    s = {1, 2}                                                     # the fused tail's sizes
    for e in EDGES:
        s.update((e, e + 1))
    s.update(RAGGED)
    return sorted(b for b in s if b <= b_max)


def plan_steps(query, b_max=B_MAX):
    """[(B, names of the fields that differ between the plans of B and B + 1)] for B = 1 ... b_max - 1."""
    steps = []
    prev = query(1)
    for B in range(1, b_max):
        nxt = query(B + 1)
        changed = tuple(k for k in prev if prev[k] != nxt[k])
        if changed:
            steps.append((B, changed))
        prev = nxt
    return steps


def derive_sizes(query, b_max=B_MAX, only=None):
    """Both sides of every B where the plan changes (`only`: where one of these fields changes), thinned as the module docstring says, plus the fixed list
    (`only`: plus nothing -- the caller adds its own)."""
    steps = plan_steps(query, b_max)
    per_field = {}
    for B, changed in steps:
        for f in changed:
            per_field.setdefault(f, []).append(B)
    kept_of = {}
    for f, at in per_field.items():
        if f in NEVER_THINNED or len(at) <= 8:
            kept_of[f] = set(at)
        else:
            kept_of[f] = {b for i, b in enumerate(at) if i % 4 == 0 or i == len(at) - 1}
    sizes = set()
    for B, changed in steps:
        fields = [f for f in changed if only is None or f in only]
        if any(B in kept_of[f] for f in fields):
            sizes.update((B, B + 1))
    if only is None:
        sizes.update(fixed_sizes(b_max))
    return sorted(sizes)


def sample_rows(B):
    """8 ... 11 rows of a batch of B (all of them below 8): row 0, B - 1, B // 2, both sides of the last multiple of 16, 64, 128, 256 below B; filled up from a
    generator seeded with B."""
    rows = {0, B - 1, B // 2}
    for g in (16, 64, 128, 256):
        t = (B - 1) // g * g
        if t > 0:
            rows.update((t - 1, t))
    rng = np.random.RandomState(B)
    while len(rows) < min(8, B):
        rows.add(int(rng.randint(B)))
    assert len(rows) <= 16
    return sorted(rows)


def seeds_of(B):
    """(seed of the targets, seed of samp_p, first_index) of a size: its own in every size; odd sizes sit above 2^33."""
    return 7000 + B, 1000 + B, 7919 * B + 5 + (2**33 if B & 1 else 0)


# ---- comparison helpers (plain arrays: tests/test_gpu_plan_sweep.py::test_helpers_* run them without a GPU) ------------------------------------------------------------
def assert_rows_equal(got, want, B, what, row0=0):
    """got == want bit for bit, both [rows][coordinates] (numpy arrays or torch tensors); the message names the size, the first differing row and coordinate."""
    assert tuple(got.shape) == tuple(want.shape), f"{what} at {B} preimages: shapes {tuple(got.shape)} and {tuple(want.shape)}"
    ne = got != want
    if not bool(ne.any()):
        return
    def where(mask):                 # numpy: a tuple of index arrays; torch: a tensor [count][1]
        nz = mask.nonzero()
        return nz[0] if isinstance(nz, tuple) else nz.flatten()
    bad = where(ne.any(1))
    r = int(bad[0])
    c = int(where(ne[r])[0])
    raise AssertionError(f"{what} at {B} preimages: {len(bad)} of {got.shape[0]} rows differ, first row {row0 + r} coordinate {c}: {int(got[r][c])} against {int(want[r][c])}")


def assert_sample_matches_oracle(B, rows, got, want):
    """got, want: {stage: [len(rows)][...]} of the sampled rows of a size; the stages are compared in the order they are computed, so the message names the first
    stage that went wrong, with the size and the row OF THE BATCH.  Doubles are compared as bit patterns."""
    for stage in STAGES:
        if stage not in got:
            continue
        g, w = np.ascontiguousarray(got[stage]), np.ascontiguousarray(want[stage])
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert g.shape == w.shape, f"stage {stage} at {B} preimages: shapes {g.shape} and {w.shape}"
        ne = g != w
        if ne.any():
            i = int(ne.any(1).nonzero()[0][0])
            c = int(ne[i].nonzero()[0][0])
            raise AssertionError(f"stage {stage} at {B} preimages differs from the oracle: row {rows[i]} coordinate {c}: {got[stage][i][c]!r} against {want[stage][i][c]!r} "
                                 f"({int(ne.any(1).sum())} of {len(rows)} sampled rows)")


# ---- CPU tests of the helpers: the comparisons fail when they must, and say where -----------------------------------------------------------------------------------------
def _fake_sample(B, m=40, n=6, w=12):
    rows = sample_rows(B)
    rng = np.random.RandomState(3)
    R = len(rows)
    return rows, dict(d=rng.randn(R, m), x=rng.randn(R, m), p=rng.randint(-50, 50, (R, m)), v=rng.randint(0, 99, (R, n)).astype(np.uint64),
                      z=rng.randint(-9, 9, (R, w)), e=rng.randint(-50, 50, (R, m)))


def test_helpers_one_perturbed_oracle_element_fails_and_names_size_row_and_stage():
    B = 1601
    rows, got = _fake_sample(B)
    want = {k: v.copy() for k, v in got.items()}
    assert_sample_matches_oracle(B, rows, got, want)
    i = rows.index(1600)
    for stage in STAGES:
        bad = {k: v.copy() for k, v in want.items()}
        if stage in ("d", "x"):
            bad[stage][i, 7] = np.nextafter(bad[stage][i, 7], np.inf)       # one unit in the last place
        else:
            bad[stage][i, 5] += 1
        with pytest.raises(AssertionError) as exc:
            assert_sample_matches_oracle(B, rows, got, bad)
        msg = str(exc.value)
        assert f"stage {stage} " in msg and "1601 preimages" in msg and "row 1600 " in msg, msg
    # -0.0 against 0.0: equal as numbers, different bits
    bad = {k: v.copy() for k, v in want.items()}
    got["x"][0, 0], bad["x"][0, 0] = 0.0, -0.0
    with pytest.raises(AssertionError, match="stage x at 1601 preimages"):
        assert_sample_matches_oracle(B, rows, got, bad)


def test_helpers_one_swapped_reference_row_fails_and_names_size_and_row():
    import torch
    B, m = 333, 50
    rng = np.random.RandomState(5)
    e = rng.randint(-99, 99, (B, m)).astype(np.int64)
    ref = e.copy()
    ref[[320, 321]] = ref[[321, 320]]                                      # two rows of the last 16-row reference call swapped
    for conv in (np.asarray, torch.from_numpy):
        assert_rows_equal(conv(e), conv(e.copy()), B, "the batch against its rows 16 at a time")
        with pytest.raises(AssertionError) as exc:
            assert_rows_equal(conv(e), conv(ref), B, "the batch against its rows 16 at a time")
        msg = str(exc.value)
        assert "333 preimages" in msg and "2 of 333 rows" in msg and "first row 320 " in msg, msg


def test_helpers_sizes_hold_the_fixed_list_and_both_sides_of_every_step():
    def plan(B):             # a planner in miniature: a form field with one step, a counter that steps every 16, a quiet field
        return {"product": "TASKS" if B <= 1472 else "BIG", "gadget": "G_ROW" if B <= 20 else "G_QUEUE", "ncg": (B + 15) // 16, "k32": 1}
    sizes = derive_sizes(plan)
    assert set(fixed_sizes()) <= set(sizes) and sizes[0] == 1 and sizes[-1] <= B_MAX
    for e in EDGES:
        assert e in sizes and e + 1 in sizes
    assert all(b in sizes for b in RAGGED)
    ncg_steps = [b for b in range(16, B_MAX, 16)]
    kept = [b for b in ncg_steps if b in sizes and b + 1 in sizes]
    assert ncg_steps[0] in kept and ncg_steps[-1] in kept and all(b in kept for b in ncg_steps[::4]) and len(kept) < len(ncg_steps) // 2      # first, last, every fourth
    assert derive_sizes(lambda B: {"product": "BIG"}) == fixed_sizes()       # a query that says nothing leaves the fixed list
    only = derive_sizes(plan, only=("gadget",))
    assert only == [20, 21]
    for B in (1, 2, 7, 8, 9, 100, 257, 1601, 4096, 4352):
        rows = sample_rows(B)
        assert min(8, B) <= len(rows) <= 16 and {0, B - 1, B // 2} <= set(rows) and all(0 <= r < B for r in rows)
    assert {4079, 4080, 4031, 4032, 3967, 3968, 3839, 3840} <= set(sample_rows(4096))
    assert len({seeds_of(B) for B in range(1, B_MAX + 1)}) == B_MAX


# ---- a leg: one key, one handle, the ascending pass, the descending pass, the oracle ----------------------------------------------------------------------------------------
class Leg:
    def __init__(self, oracle, n, q, r, s, key_seed, full_oracle=False, select=None):
        import torch
        import tools_amd as T
        self.torch, self.oracle = torch, oracle
        self.n, self.q, self.full_oracle = n, q, full_oracle
        self.dev = torch.device("cuda:0")
        self.psf = T.PSFPerturbation(T.GadgetParameters.init_default(n, q), r, s)
        if full_oracle:
            A, (R, Lp, _) = self.psf.trap_gen(key_seed)
            self.orc = oracle.PSFPerturbation(oracle.gadget_params_default(n, q), r, s)
            self.orc.load_key(A, R, Lp)
        else:
            self.psf.trap_gen(key_seed, export=False)
            A, R = self.psf.export_A_R()
            self.orc = oracle.PSFPerturbation(oracle.gadget_params_default(n, q), r, s, with_L=False)
            self.orc.load_key(A, R)
        self.m = self.psf.m
        t0 = time.time()
        self.sizes = select(self.psf.query_plan) if select else derive_sizes(self.psf.query_plan)      # the query changes nothing: the handle is still fresh
        self.t_query = time.time() - t0
        self.first = {}          # B -> the ascending pass's rows on the device, narrowed (checked to hold the values)
        self.sample = {}         # B -> dict(rows, u, got={stage: sampled rows})
        self.small_desc = {}     # B in (1, 2) -> the descending pass's rows
        self.plans = []          # the executed plans of the compared calls
        self.done_asc, self.done_desc = set(), set()
        self.oracle_s = 0.0

    def close(self):
        self.first.clear()
        self.psf.close()
        self.torch.cuda.empty_cache()

    def part(self, k, parts, descending=False):
        lo, hi = k * len(self.sizes) // parts, (k + 1) * len(self.sizes) // parts
        chunk = self.sizes[lo:hi]
        if descending:
            lo, hi = (parts - 1 - k) * len(self.sizes) // parts, (parts - k) * len(self.sizes) // parts
            chunk = self.sizes[lo:hi][::-1]
        return chunk

    # one device-pointer call into a tensor of sentinels, synchronised, its status checked
    def call(self, u, B, seed, first, out=None):
        e = self.torch.empty((B, self.m), dtype=self.torch.int64, device=self.dev) if out is None else out
        e.fill_(SENTINEL)
        self.psf.samp_p_dev(u.data_ptr(), e.data_ptr(), B, seed=seed, first_index=first)
        self.torch.cuda.synchronize()
        assert self.psf.last_status() == 0, f"sampler failure at {B} preimages"
        return e

    def targets(self, B):
        u = self.torch.empty((B, self.n), dtype=self.torch.int64, device=self.dev)
        self.psf.uniform_targets_dev(u.data_ptr(), B, seed=seeds_of(B)[0], first_index=0)
        self.torch.cuda.synchronize()
        return u

    def check_valid(self, u, e, B, what):      # item 2
        torch = self.torch
        u2 = torch.empty_like(u)
        ok = torch.zeros((B,), dtype=torch.uint8, device=self.dev)
        self.psf.f_a_dev(e.data_ptr(), u2.data_ptr(), ok.data_ptr(), B)
        torch.cuda.synchronize()
        assert_rows_equal(u2, u, B, f"f_a(e) against u, {what}")
        assert bool(ok.all().item()), f"check_domain fails at {B} preimages, {what}: rows {(ok == 0).nonzero().flatten().tolist()[:8]}"

    def ascending(self, B):
        torch, psf = self.torch, self.psf
        su, seed, first = seeds_of(B)
        u = self.targets(B)
        # the same rows 16 at a time, each call another first_index
        ref = torch.empty((B, self.m), dtype=torch.int64, device=self.dev)
        for j in range(0, B, 16):
            self.call(u[j:], min(16, B - j), seed, first + j, out=ref[j:j + min(16, B - j)])
            if j == 0:           # (a compared call as well: item 3 ties it to the batch, item 4 the batch to the oracle)
                self.plans.append(dict(psf.last_plan(), B=min(16, B)))
        # a batch of the same size with another seed: what the compared call finds in the buffers is not its own result
        q0 = psf.query_plan(B)                                   # (here B may exceed what the handle's buffers hold: the query derives what the call will)
        other = self.call(u, B, seed + 500000, first)
        assert psf.last_plan() == q0, f"executed and queried plan differ at {B} preimages (buffers growing): {psf.last_plan()} against {q0}"
        self.check_valid(u, other, B, "the call with another seed")
        del other
        if B <= 2:      # the first call of a size ran without the compact copies (recorded above); the compared batch runs with them, whatever the packers' timing
            self.wait_for_compact_copies()
        q = psf.query_plan(B)
        e = self.call(u, B, seed, first)
        ran = psf.last_plan()
        assert ran == q, f"executed and queried plan differ at {B} preimages: {ran} against {q}"                       # item 1
        if B <= 2:      # (plan_zq serves ONE preimage with the 32-bit copy of A: small_max)
            assert (ran["tail"], ran["recombine"]) == (1, "R_SMALL2") and (B == 2 or ran["syn.form"] == "SMALL32"), f"{B} preimages with the compact copies ran {ran}"
        self.plans.append(dict(ran, B=B))
        self.check_valid(u, e, B, "the compared batch")                                                                # item 2
        assert_rows_equal(e, ref, B, "the batch against its rows 16 at a time")                                        # item 3
        del ref
        keep = e.to(torch.int16)      # (the coordinates of these parameter sets fit 16 bits; checked, with 32 bits to fall back on)
        if not bool((keep.to(torch.int64) == e).all().item()):
            keep = e.to(torch.int32)
            assert bool((keep.to(torch.int64) == e).all().item())
        self.first[B] = keep
        rows = list(range(B)) if self.full_oracle else sample_rows(B)
        idx = torch.tensor(rows, device=self.dev)
        got = {"e": e[idx].cpu().numpy()}
        uh = u.cpu().numpy().astype(np.uint64)
        if B <= 256:      # the staged call (host pointers, the same plan), behind a call with a third seed
            self.call(u, B, seed + 700000, first)
            qs = psf.query_plan(B)
            st = psf.samp_p_stages(uh, seed=seed, first_index=first)
            assert psf.last_plan() == qs, f"executed and queried plan differ at {B} preimages (staged call)"
            assert_rows_equal(st["e"], e.cpu().numpy(), B, "the staged call against the batch")
            srows = sample_rows(B)
            got_st = {k: st[k][srows] for k in STAGES}
        else:
            srows, got_st = None, None
        self.sample[B] = dict(rows=rows, u=uh[rows], got=got, srows=srows, u_st=None if srows is None else uh[srows], got_st=got_st)
        self.done_asc.add(B)

    def wait_for_compact_copies(self):
        """Until the query reports the forms of the compact copies at one preimage.  The query does not touch the handle and the packers' event is polled by calls of
        at most four preimages only: each try is such a call, with a seed of its own."""
        u = self.targets(1)
        for attempt in range(40):
            q = self.psf.query_plan(1)
            if q["tail"] == 1 and q["recombine"] == "R_SMALL2":
                return
            self.call(u, 1, 900000 + attempt, 77 + attempt)
            time.sleep(0.05)
        raise AssertionError(f"the compact key copies never became usable: the plan of one preimage is still {self.psf.query_plan(1)}")

    def descending(self, B):
        psf = self.psf
        su, seed, first = seeds_of(B)
        assert B in self.done_asc, f"the ascending pass did not reach {B} preimages"
        if B <= 4 and not getattr(self, "compact_seen", False):
            self.wait_for_compact_copies()
            self.compact_seen = True
        u = self.targets(B)
        q = psf.query_plan(B)
        e = self.call(u, B, seed, first)
        ran = psf.last_plan()
        assert ran == q, f"executed and queried plan differ at {B} preimages (descending): {ran} against {q}"
        self.plans.append(dict(ran, B=B))
        if B <= 2:      # (syn.form is not asserted here: see ORDER ON THE HANDLE)
            assert (ran["tail"], ran["recombine"]) == (1, "R_SMALL2"), f"{B} preimages with the compact copies ran {ran}"
            self.small_desc[B] = e.cpu().numpy()
        self.check_valid(u, e, B, "the descending pass")
        assert_rows_equal(e, self.first.pop(B).to(self.torch.int64), B, "the descending pass against the ascending pass")
        self.done_desc.add(B)

    def oracle_rows(self, sizes):
        """Item 4 for these sizes: d, x, p, v, z, e of the sampled rows from the oracle alone, compared with the ascending pass (and, at one and two preimages, with the
        descending pass's fused launch)."""
        t0 = time.time()
        O, m = self.oracle, self.m
        from concurrent.futures import ThreadPoolExecutor
        jobs = []                # (B, batch row, u row, which comparison)
        for B in sizes:
            assert B in self.done_asc, f"the ascending pass did not reach {B} preimages"
            s = self.sample[B]
            su, seed, first = seeds_of(B)
            for i, r in enumerate(s["rows"]):
                if self.full_oracle and r not in sample_rows(B):
                    continue
                assert (O.uniform_targets(su, 1, self.n, self.q, first_index=r)[0] == s["u"][i]).all(), f"target row {r} at {B} preimages is not the oracle's"
            want = {}
            if self.full_oracle:
                want["e"] = self.orc.samp_p(seed, s["u"], first_index=first, nthreads=min(16, os.cpu_count() or 1))
                assert_sample_matches_oracle(B, s["rows"], s["got"], want)
                if s["srows"] is not None:
                    tr = [self.orc.samp_p_trace(seed, first + r, s["u_st"][i]) for i, r in enumerate(s["srows"])]
                    assert_sample_matches_oracle(B, s["srows"], s["got_st"], {k: np.array([t[k] for t in tr]) for k in STAGES})
            else:
                jobs += [(B, r, s["u"][i]) for i, r in enumerate(s["rows"])]
        if jobs:
            d = np.array([O.normals(seeds_of(B)[1], seeds_of(B)[2] + r, m) for B, r, _ in jobs])
            x = np.zeros((len(jobs), m))
            for row0 in range(0, m, 2048):                        # every row block of the factor, each exported once
                nr = min(2048, m - row0)
                x[:, row0:row0 + nr] = O.centres_rows(self.psf.export_sqrt_sigma2_rows(row0, nr), row0, nr, m, d)
            with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
                fx = list(pool.map(lambda a: self.orc.samp_p_from_x(seeds_of(a[1][0])[1], seeds_of(a[1][0])[2] + a[1][1], a[1][2], x[a[0]]), enumerate(jobs)))
            at = 0
            for B in sizes:
                s = self.sample[B]
                k = len(s["rows"])
                want = {key: np.array([f[key] for f in fx[at:at + k]]) for key in ("p", "v", "z", "e")}
                want["d"], want["x"] = d[at:at + k], x[at:at + k]
                at += k
                assert_sample_matches_oracle(B, s["rows"], s["got"], want)                    # e of the batch
                if s["srows"] is not None:                                                    # B <= 256: every stage (sample_rows(B) is what s["rows"] holds here)
                    assert s["srows"] == s["rows"]
                    assert_sample_matches_oracle(B, s["srows"], s["got_st"], want)
                if B in self.small_desc:                                                      # the fused tail, SMALL32 and R_SMALL2 of the descending pass
                    assert_sample_matches_oracle(B, s["rows"], {"e": self.small_desc[B][s["rows"]]}, want)
        if self.full_oracle:
            for B in sizes:
                if B in self.small_desc:
                    su, seed, first = seeds_of(B)
                    assert_sample_matches_oracle(B, list(range(B)), {"e": self.small_desc[B]}, {"e": self.orc.samp_p(seed, self.sample[B]["u"], first_index=first)})
        self.oracle_s += time.time() - t0


def assert_coverage(plans, want):
    """want: {field: values that must occur}; plus the pairs named below"""
    for field, values in want.items():
        seen = {p[field] for p in plans}
        assert set(values) <= seen, f"{field}: {sorted(map(str, set(values) - seen))} never ran (ran: {sorted(map(str, seen))})"


C3_COVERAGE = {
    "product": ("TASKS", "TILES32", "TILES64", "TILES96", "BIG"),
    "round": ("ROUND_TAB", "ROUND_TAB_ROW"),
    "syn.form": ("SMALL", "SMALL32", "MFMA"),
    "gadget": ("G_WAVE", "G_ROW", "G_QUAD", "G_QUEUE"),
    "recombine": ("R_SMALL", "R_SMALL2", "R_WG", "R_TILES"),
    "tail": (0, 1),
    "one_launch": (0,),
}


def _leg_fixture(make):
    @pytest.fixture(scope="class")
    def leg(self, oracle):
        lg = make(oracle)
        t0 = time.time()
        yield lg
        print(f"\n[plan sweep] {type(self).__name__}: {len(lg.sizes)} sizes, {sum(lg.sizes)} rows, leg {time.time() - t0:.1f} s, query {lg.t_query:.2f} s, "
              f"oracle {lg.oracle_s:.1f} s")
        lg.close()
    return leg


@pytest.mark.gpu
class TestC3:
    """n = 512, q = 2^30, r = 9, s = 512: m = 30 801, a 3.79 GB factor.  The full list."""
    leg = _leg_fixture(lambda oracle: Leg(oracle, 512, 2**30, 9.0, 512.0, key_seed=11))

    def test_the_derived_list_holds_the_fixed_list(self, leg):
        assert leg.m == 30801
        assert set(fixed_sizes()) <= set(leg.sizes), sorted(set(fixed_sizes()) - set(leg.sizes))
        assert len(leg.sizes) > len(fixed_sizes()), "the query found no step of the plan between 1 and 4352 preimages"
        print(f"\n[plan sweep] C3 sizes ({len(leg.sizes)}): {leg.sizes}")

    @pytest.mark.parametrize("k", range(PARTS))
    def test_ascending(self, leg, k):
        for B in leg.part(k, PARTS):
            leg.ascending(B)

    @pytest.mark.parametrize("k", range(PARTS))
    def test_descending_agrees_with_ascending(self, leg, k):
        for B in leg.part(k, PARTS, descending=True):
            leg.descending(B)

    @pytest.mark.parametrize("k", range(PARTS))
    def test_sampled_rows_match_the_oracle(self, leg, k):
        leg.oracle_rows(leg.part(k, PARTS))

    def test_every_reachable_form_ran(self, leg):
        assert leg.done_desc == set(leg.sizes)
        assert_coverage(leg.plans, C3_COVERAGE)
        big = {(p["GR"], p["GC"]) for p in leg.plans if p["product"] == "BIG"}
        assert {(8, 4), (16, 2)} <= big, big
        assert any(p["recombine"] == "R_TILES" and p["rc_big"] == 1 for p in leg.plans)
        assert all(p["syn.pow2"] == 1 for p in leg.plans if p["syn.form"] == "MFMA")
        import tools_amd.psf as P
        for field, names in UNREACHABLE.items():           # what the list above leaves out is exactly what UNREACHABLE explains
            every = set(P.PLAN_ENUMS[field]) if field in P.PLAN_ENUMS else {0, 1}
            assert every - set(C3_COVERAGE[field]) == set(names), field


def _c3prime_sizes(query):
    steps = derive_sizes(query, only=("syn.form", "syn.splits", "syn.fold128", "syn.pow2", "syn.wave_combine", "gadget", "k32", "gq_p"))
    return sorted(set(steps) | {1, 2, 100, 1601, 4096})


@pytest.mark.gpu
class TestC3Prime:
    """q = 1 073 741 789: pow2 == 0, the digit column, the reduction that is no mask.  The sizes where a syn.* field or the gadget form changes, and 100, 1601, 4096."""
    leg = _leg_fixture(lambda oracle: Leg(oracle, 512, 1073741789, 9.0, 512.0, key_seed=12, select=_c3prime_sizes))

    def test_ascending(self, leg):
        print(f"\n[plan sweep] C3' sizes ({len(leg.sizes)}): {leg.sizes}")
        assert {1, 2, 100, 1601, 4096} <= set(leg.sizes) and len(leg.sizes) > 5
        for B in leg.sizes:
            leg.ascending(B)

    def test_descending_agrees_with_ascending(self, leg):
        for B in leg.sizes[::-1]:
            leg.descending(B)

    def test_sampled_rows_match_the_oracle(self, leg):
        leg.oracle_rows(leg.sizes)
        mfma = [p for p in leg.plans if p["syn.form"] == "MFMA"]
        assert mfma and all(p["syn.pow2"] == 0 for p in mfma)
        assert_coverage(leg.plans, {"syn.form": ("SMALL", "SMALL32", "MFMA"), "gadget": ("G_WAVE", "G_ROW", "G_QUAD", "G_QUEUE"), "tail": (0, 1)})


@pytest.mark.gpu
class TestSmallFactor:
    """n = 64, q = 128 (m = 932, the shape of tests/test_gpu_single_call.py): h->mL < 16384 switches whole branches, and BIG above 2048 preimages meets ragged batches.
    The oracle is cheap here: item 4 covers EVERY row."""
    leg = _leg_fixture(lambda oracle: Leg(oracle, 64, 128, float(np.log2(64)), 100.0, key_seed=21, full_oracle=True))

    @pytest.mark.parametrize("k", range(2))
    def test_ascending(self, leg, k):
        if k == 0:
            assert leg.m == 932 and set(fixed_sizes()) <= set(leg.sizes)
            print(f"\n[plan sweep] small-factor sizes ({len(leg.sizes)}): {leg.sizes}")
        for B in leg.part(k, 2):
            leg.ascending(B)

    @pytest.mark.parametrize("k", range(2))
    def test_descending_agrees_with_ascending(self, leg, k):
        for B in leg.part(k, 2, descending=True):
            leg.descending(B)

    @pytest.mark.parametrize("k", range(2))
    def test_every_row_matches_the_oracle(self, leg, k):
        leg.oracle_rows(leg.part(k, 2))
        if k == 1:
            assert leg.done_desc == set(leg.sizes)
            assert_coverage(leg.plans, {"product": ("TASKS", "TILES32", "TILES64", "BIG"), "tail": (0, 1), "syn.form": ("SMALL32", "MFMA"), "recombine": ("R_SMALL2",)})
            assert any(p["product"] == "BIG" and p["B"] > 2048 and p["B"] % 16 for p in leg.plans)       # BIG with a ragged batch at a small factor
