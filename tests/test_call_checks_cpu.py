"""The argument checks and the workspace layout every bytes-in, bytes-out unit shares (tools_amd/csrc/psf_call_host.hpp) on the CPU: g++ compiles the
header, which has no HIP in it, into the stand-alone program tests/cpp/call_host_check.cpp.  The program reads cases from stdin and prints what span_of,
overlap, Layout::take and the check functions answer; the expected answers are computed here with Python's unbounded integers.  A second build with
-fsanitize=address,undefined runs the same cases; it is a program of its own, nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "call_host_check.cpp")
SIZE_MAX = 2 ** 64 - 1
OK, PARAM = 0, 1                                                         # PSF_OK, PSF_ERR_PARAM (include/psf_mi355x.h)
UNTOUCHED = 7                                                            # the span the program gives every buffer before the combined run


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host check of the shared argument checks"
    out = str(tmp / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module", params=["plain", "san"])
def run(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("call_host_check_" + request.param)
    extra = [] if request.param == "plain" else ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    prog = _build(tmp, "check", extra)

    def go(lines):
        out = subprocess.run([prog], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        got = out.stdout.split("\n")[:-1]
        assert len(got) == len(lines), (len(got), len(lines))
        return [[int(x) for x in g.split()] for g in got]

    return go


# ---- the models ------------------------------------------------------------------------------------------------------------------------------------
def span_model(base, count, length, stride):
    """(fits, span): stride 0 means one item."""
    if count == 0 or length == 0:
        return True, 0
    span = (count - 1) * stride + length
    return span <= SIZE_MAX and base + span <= SIZE_MAX, span


def overlap_model(a, na, b, nb):
    return na > 0 and nb > 0 and a < b + nb and b < a + na


def take_model(requests):
    ok, total, offs = True, 0, []
    for r in requests:
        end = total + (r + 255) // 256 * 256
        if end > SIZE_MAX:
            ok = False
            offs.append(0)
        else:
            offs.append(total)
            total = end
    return ok, total, offs


def check_model(count, dev, ws, ws_bytes, need_ok, need, bufs):
    """The codes of the four checks each on its own, of the whole sequence, and the spans the sequence leaves: bufs = (p, len, stride, out, ok_null)."""
    r_null = PARAM if any(p == 0 and not ok_null for p, _, _, _, ok_null in bufs) else OK
    spans = [span_model(p, count, ln, st) for p, ln, st, _, _ in bufs]
    r_spans = OK if all(f for f, _ in spans) else PARAM
    r_ws = PARAM if dev and (ws == 0 or ws % 256 != 0 or ws_bytes < need) else OK

    def overlaps(sp):
        for i, (p, _, _, out, _) in enumerate(bufs):
            if not out or p == 0:
                continue
            for j, (q, _, _, _, _) in enumerate(bufs):
                if j != i and q != 0 and overlap_model(p, sp[i], q, sp[j]):
                    return PARAM
            if dev and overlap_model(p, sp[i], ws, need):
                return PARAM
        return OK

    # check_spans stops at the first buffer that does not fit and leaves the later spans alone
    left, seen = [], []
    for f, s in spans:
        if not f:
            break
        seen.append(s)
    each_spans = seen + [UNTOUCHED] * (len(bufs) - len(seen))
    if r_spans != OK:
        each_spans[len(seen)] = None                                      # the span that did not fit: whatever span_of left there
    r_over = overlaps([s if s is not None else 0 for s in each_spans]) if r_spans == OK else None
    if r_null != OK:
        return r_null, r_spans, r_ws, r_over, PARAM, [UNTOUCHED] * len(bufs)
    left = each_spans
    whole = PARAM if (r_spans != OK or not need_ok or r_ws != OK or r_over != OK) else OK
    return r_null, r_spans, r_ws, r_over, whole, left


def check_line(count, dev, ws, ws_bytes, need_ok, need, bufs):
    return "check %d %d %d %d %d %d %d " % (count, dev, ws, ws_bytes, need_ok, need, len(bufs)) + " ".join("%d %d %d %d %d" % b for b in bufs)


def assert_check(run, case):
    got = run([check_line(*case)])[0]
    r_null, r_spans, r_ws, r_over, whole, left = check_model(*case)
    assert got[0:3] == [r_null, r_spans, r_ws], (case, got)
    if r_over is not None:
        assert got[3] == r_over, (case, got)
    assert got[4] == whole, (case, got)
    for g, w in zip(got[5:], left):
        assert w is None or g == w, (case, got, left)
    return got


# ---- span_of ---------------------------------------------------------------------------------------------------------------------------------------
def _span_cases():
    cases = []
    for count in (0, 1, 2, 5):
        for length in (0, 1, 32):
            for stride in (0, length, length + 3):
                cases.append((4096, count, length, stride))
    for length in (1, 32, 2 ** 32 + 1):
        for stride in (length, length + 3):
            most = (SIZE_MAX - length) // stride + 1                       # the largest count whose span fits at base 0
            assert span_model(0, most, length, stride)[0] and not span_model(0, most + 1, length, stride)[0]
            cases.append((0, most, length, stride))
            if most + 1 <= SIZE_MAX:                                       # one-byte items at stride 1: every count a size_t can hold fits
                cases.append((0, most + 1, length, stride))
        cases += [(0, SIZE_MAX, length, 0), (SIZE_MAX - length, SIZE_MAX, length, 0), (SIZE_MAX - length + 1, 2, length, 0)]
    for count, length, stride in ((1, 1, 1), (3, 32, 35), (2, 2 ** 32 + 1, 2 ** 32 + 1)):
        span = (count - 1) * stride + length
        cases += [(SIZE_MAX - span, count, length, stride), (SIZE_MAX - span + 1, count, length, stride)]      # the end at SIZE_MAX, and one byte more
    return cases


def test_span_of_at_every_edge(run):
    cases = _span_cases()
    got = run(["span %d %d %d %d" % c for c in cases])
    fits = 0
    for c, (g_ok, g_span) in zip(cases, got):
        ok, span = span_model(*c)
        assert g_ok == int(ok), (c, g_ok, g_span)
        if ok:
            assert g_span == span, (c, g_span, span)
            fits += 1
    assert 0 < fits < len(cases)


# ---- overlap ---------------------------------------------------------------------------------------------------------------------------------------
def test_overlap_adjacent_shared_and_empty(run):
    cases = [(100, 10, 110, 10), (110, 10, 100, 10),                      # adjacent, both ways
             (100, 11, 110, 10), (110, 10, 100, 11),                      # one shared byte
             (100, 20, 105, 0), (105, 0, 100, 20), (100, 0, 100, 0),      # a zero-length range inside another
             (100, 20, 105, 5), (100, 5, 100, 5), (100, 5, 200, 5),
             (SIZE_MAX - 15, 15, SIZE_MAX - 7, 7), (SIZE_MAX - 15, 8, SIZE_MAX - 7, 7)]
    got = run(["overlap %d %d %d %d" % c for c in cases])
    want = [int(overlap_model(*c)) for c in cases]
    assert [g[0] for g in got] == want
    assert want[:7] == [0, 0, 1, 1, 0, 0, 0]


# ---- Layout::take ----------------------------------------------------------------------------------------------------------------------------------
def test_layout_take_rounds_and_overflows(run):
    top = SIZE_MAX // 256 * 256                                            # SIZE_MAX rounded down to 256
    cases = [[0], [1], [256], [257], [0, 1, 256, 257, 0, 3],
             [top], [top - 256, 256], [top - 256, 1],                     # a total exactly at the top
             [top, 1], [top - 256, 257], [top + 1],                       # the first that overflows
             [2 ** 64], [2 ** 64 + 5], [2 ** 100, 1], [1, 2 ** 127, 1]]     # 128-bit requests above 2^64; a later section after a failed one
    got = run(["take " + " ".join(str(r) for r in c) for c in cases])
    for c, g in zip(cases, got):
        ok, total, offs = take_model(c)
        assert g == [int(ok), total] + offs, (c, g)
    assert [take_model(c)[0] for c in cases] == [True] * 8 + [False] * 7
    assert take_model([top])[1] == top and take_model([257])[1] == 512


# ---- the order of the checks -----------------------------------------------------------------------------------------------------------------------
WS, NEED = 0x10000, 1024


def test_checks_report_in_the_documented_order(run):
    """One call that violates the NULL, span, workspace and overlap rules at once, repaired one rule at a time: every check still reports its own
    violation, the whole sequence fails until the last one is repaired, and it returns before check_spans while a NULL is left."""
    count = 4
    null_in, huge, out_on_in = (0, 32, 32, 0, 0), (0x2000, 2 ** 63, 2 ** 63, 0, 0), (0x1008, 16, 16, 1, 0)
    ok_in, small = (0x1000, 32, 32, 0, 0), (0x2000, 64, 64, 0, 0)
    out_free = (0x4000, 16, 16, 1, 0)
    steps = [((count, 1, WS + 1, NEED - 1, 1, NEED, [null_in, huge, out_on_in]), [PARAM, PARAM, PARAM]),
             ((count, 1, WS + 1, NEED - 1, 1, NEED, [ok_in, huge, out_on_in]), [OK, PARAM, PARAM]),
             ((count, 1, WS + 1, NEED - 1, 1, NEED, [ok_in, small, out_on_in]), [OK, OK, PARAM]),
             ((count, 1, WS, NEED, 1, NEED, [ok_in, small, out_on_in]), [OK, OK, OK])]
    for case, first3 in steps:
        got = assert_check(run, case)
        assert got[0:3] == first3 and got[4] == PARAM, (case, got)
    assert assert_check(run, steps[0][0])[5:] == [UNTOUCHED] * 3           # NULL: returned before any span was computed
    assert assert_check(run, steps[1][0])[5] == 3 * 32 + 32                # span: the first buffer's was, the second stopped it
    assert assert_check(run, steps[3][0])[3] == PARAM                      # only the overlap is left
    got = assert_check(run, (count, 1, WS, NEED, 1, NEED, [ok_in, small, out_free]))
    assert got[:5] == [OK] * 5 and got[5:] == [128, 256, 64]
    # a workspace whose size does not fit size_t fails after the spans and before the workspace is looked at
    got = assert_check(run, (count, 1, WS, NEED, 0, NEED, [ok_in, small, out_free]))
    assert got[:5] == [OK, OK, OK, OK, PARAM] and got[5:] == [128, 256, 64]


def test_workspace_rules_hold_for_device_forms_only(run):
    bufs = [(0x1000, 32, 32, 0, 0), (0x4000, 16, 16, 1, 0)]
    for ws, ws_bytes in ((0, NEED), (WS + 8, NEED), (WS, NEED - 1)):
        assert assert_check(run, (2, 1, ws, ws_bytes, 1, NEED, bufs))[4] == PARAM
        assert assert_check(run, (2, 0, ws, ws_bytes, 1, NEED, bufs))[4] == OK
    # an output inside the workspace: refused in the device form, unseen in the host form
    inside = [(0x1000, 32, 32, 0, 0), (WS + 512, 16, 16, 1, 0)]
    assert assert_check(run, (2, 1, WS, NEED, 1, NEED, inside))[3:5] == [PARAM, PARAM]
    assert assert_check(run, (2, 0, WS, NEED, 1, NEED, inside))[3:5] == [OK, OK]
    # an input may lie in the workspace and inputs may overlap each other
    shared = [(WS, 32, 32, 0, 0), (WS + 8, 32, 32, 0, 0), (0x4000, 16, 16, 1, 0)]
    assert assert_check(run, (2, 1, WS, NEED, 1, NEED, shared))[4] == OK


def test_null_buffers_that_may_be_null_are_skipped(run):
    """ok_null: a NULL input (an empty message) and a NULL output (d_why) pass check_null and take no part in check_overlaps, whatever their length."""
    out = (0x4000, 16, 16, 1, 0)
    null_msg, null_why = (0, 0, 0, 0, 1), (0, 1, 1, 1, 1)
    got = assert_check(run, (3, 1, WS, NEED, 1, NEED, [null_msg, out, null_why]))
    assert got[:5] == [OK] * 5
    # a NULL output with a span that would cover every address still overlaps nothing
    wide_null = (0, 2 ** 40, 2 ** 40, 1, 1)
    assert assert_check(run, (3, 1, WS, NEED, 1, NEED, [wide_null, out, (0x100, 64, 0, 0, 0)]))[:5] == [OK] * 5
    # the same buffers without ok_null: the NULL is refused
    assert assert_check(run, (3, 1, WS, NEED, 1, NEED, [(0, 1, 1, 1, 0), out]))[0] == PARAM
    # stride 0: one item for all, so `count` does not stretch its span
    assert assert_check(run, (1000, 1, WS, NEED, 1, NEED, [(0x100, 64, 0, 0, 0), (0x140, 1, 1, 1, 0)]))[:5] == [OK] * 5
    assert assert_check(run, (1000, 1, WS, NEED, 1, NEED, [(0x100, 64, 64, 0, 0), (0x140, 1, 1, 1, 0)]))[3:5] == [PARAM, PARAM]
