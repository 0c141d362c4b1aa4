"""No-GPU checks of ML-DSA signing (psf_mldsa_sign_*, include/psf_mi355x.h): every symbol exported and mirrored; the workspace sizes; every argument
error in its stated order with fake pointers (all checked before the first HIP call, so the codes hold on any host) and the guard buffer unchanged;
the restated signer of tests/helpers/mldsa_sign_model.py against the model's sign_internal; the searched cases; and what signing adds to
tools_amd/csrc/psf_mldsa_core.hpp, compiled by g++ with -fsanitize=address,undefined as a program of its own (tests/cpp/mldsa_sign_host_check.cpp)
and compared with hashlib and the model.  The device results are compared with the model in tests/test_gpu_mldsa_sign.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import mldsa_model as M
from tests.helpers import mldsa_sign_cases as K
from tests.helpers import mldsa_sign_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PARAM, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 7, 8
SMAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
SYMBOLS = ("psf_mldsa_sign_workspace_bytes", "psf_mldsa_sign_begin_dev", "psf_mldsa_sign_round_dev", "psf_mldsa_sign_end_dev", "psf_mldsa_sign")
SIZES = {44: (1312, 2560, 2420), 65: (1952, 4032, 3309), 87: (2592, 4896, 4627)}
KL = {44: (4, 4), 65: (6, 5), 87: (8, 7)}
BYTES, MU = 0, 1
Q = M.Q


def _lib():
    from tools_amd import mldsa
    return mldsa._lib()


def _have_device():
    if not os.path.exists("/dev/kfd"):
        return False
    name, cus = C.create_string_buffer(64), C.c_int(0)
    return _lib().psf_device_info(0, name, 64, C.byref(cus)) == 0


def _ws(L, param, count, sk_stride):
    out = C.c_size_t(0)
    assert L.psf_mldsa_sign_workspace_bytes(param, count, sk_stride, C.byref(out)) == OK
    return out.value


def test_every_symbol_is_exported_and_mirrored():
    L = _lib()
    for fn in SYMBOLS:
        assert hasattr(L, fn), fn
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"])
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "psf_mi355x.hpp")).read()
    for fn in SYMBOLS:
        assert f"pub fn {fn}(" in ffi, fn
        assert fn + "(" in hpp, fn
    import tools_amd as T
    for name in ("sign_workspace_bytes", "sign_begin_dev", "sign_round_dev", "sign_end_dev", "sign_internal", "sign"):
        assert callable(getattr(T.mldsa, name)), name
    assert "Signing is not offered" not in open(os.path.join(ROOT, "include", "psf_mi355x.h")).read()
    assert "Signing is not offered" not in (T.mldsa.__doc__ or "")


def test_workspace_bytes_values_and_monotonicity():
    L = _lib()
    out = C.c_size_t(99)
    for param in (-1, 0, 2, 45):
        assert L.psf_mldsa_sign_workspace_bytes(param, 1, 0, C.byref(out)) == ERR_PARAM
    assert L.psf_mldsa_sign_workspace_bytes(65, 1, 0, None) == ERR_PARAM
    assert L.psf_mldsa_sign_workspace_bytes(65, 1, 1, C.byref(out)) == ERR_PARAM                 # a stride below the sk size
    assert L.psf_mldsa_sign_workspace_bytes(65, 1, SIZES[65][1] - 1, C.byref(out)) == ERR_PARAM
    assert L.psf_mldsa_sign_workspace_bytes(65, SMAX // 1024, 0, C.byref(out)) == ERR_PARAM       # does not fit size_t
    assert out.value == 99
    for param, (k, l) in KL.items():
        sk = SIZES[param][1]
        for stride in (0, sk, sk + 7):
            last = 0
            for count in (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 67, 255, 256, 259, 4096, 65536):
                w = _ws(L, param, count, stride)
                assert w % 256 == 0 and w >= last, (param, stride, count)
                last = w
            assert _ws(L, param, 0, stride) == 0
        assert _ws(L, param, 65536, sk) == _ws(L, param, 65536, sk + 7)
        # a slot's state: mu, rho'', kappa, the index; with a key per instance the images of A_hat, s1, s2, t0 too; the scratch: y, w, c, z, c t0
        state, images, scratch = 64 + 64 + 4 + 4, (k * l + l + 2 * k) * 1024, (2 * l + 2 * k + 1) * 2048
        assert _ws(L, param, 1, 0) == _ws(L, param, 1, sk)                                         # one instance has one key either way
        for count in (2, 65, 65536):
            shared, per_key = _ws(L, param, count, 0), _ws(L, param, count, sk)
            assert shared < per_key, (param, count)
            assert shared >= count * (state + scratch) + images
            assert per_key >= count * (state + scratch + images)
            assert per_key < count * (state + scratch + images + 256) + 64 * 256
    assert _ws(L, 87, 65536, SIZES[87][1]) > 1 << 32                                               # offsets past 32 bits


def _begin(L, param, msg_len=33, kind=BYTES, sk_stride=None, msg_stride=None):
    ss = SIZES.get(param, SIZES[44])[1] if sk_stride is None else sk_stride
    ms = msg_len if msg_stride is None else msg_stride
    return lambda c, sk, msg, rnd, live, w, wb: L.psf_mldsa_sign_begin_dev(0, param, c, sk, ss, msg, msg_len, ms, kind, rnd, w, wb, live, None, None)


def _round(L, param, sk_stride=None, active=None):
    ss = SIZES.get(param, SIZES[44])[1] if sk_stride is None else sk_stride
    return lambda c, sig, rounds, live, w, wb: L.psf_mldsa_sign_round_dev(0, param, c, ss, c if active is None else active, sig, rounds, w, wb, live, None, None)


def _host(L, param, msg_len=33, kind=BYTES, sk_stride=None, max_rounds=8):
    ss = SIZES.get(param, SIZES[44])[1] if sk_stride is None else sk_stride
    return lambda c, sk, msg, rnd, sig, rounds, w=None, wb=0: L.psf_mldsa_sign(0, param, c, sk, ss, msg, msg_len, msg_len, kind, rnd, sig, max_rounds, rounds)


@pytest.mark.parametrize("param", [44, 65, 87])
def test_argument_errors_in_order_and_nothing_written(param):
    L = _lib()
    count = 2
    pk_len, sk_len, sig_len = SIZES[param]
    wsb = _ws(L, param, count, sk_len)
    buf = np.full(wsb + (1 << 16), 7, dtype=np.uint8)
    WS = (buf.ctypes.data + 255) // 256 * 256
    P = (WS + wsb + 15) // 16 * 16
    msg_len = 33
    # name: (maker, byte lengths per instance (0: one item of 4 bytes), index of the first output, NULL allowed, device form)
    calls = {
        "begin": (lambda p: _begin(L, p, msg_len), (sk_len, msg_len, 32, 0), 3, {2}, True),
        "round": (lambda p: _round(L, p), (sig_len, 4, 0), 0, {1}, True),
        "host": (lambda p: _host(L, p, msg_len), (sk_len, msg_len, 32, sig_len, 4), 3, {2, 4}, False),
    }
    for name, (make, lens, n_in, may_null, dev) in calls.items():
        f = make(param)
        ptrs, at = [], P
        for ln in lens:
            ptrs.append(at)
            at += (count * ln if ln else 4) + 64
            at = (at + 15) // 16 * 16
        nul = [None] * len(ptrs)
        span = [count * ln if ln else 4 for ln in lens]

        def call(cnt, p, w=WS, wb=wsb, g=f):
            return g(cnt, *p, w, wb)
        # 1. unknown param first of all, even with count = 0 and NULL pointers
        for bad in (-1, 0, 2, 3, 45, 768):
            g = make(bad)
            assert call(count, ptrs, g=g) == ERR_PARAM, (name, bad)
            assert call(0, nul, w=None, wb=0, g=g) == ERR_PARAM, (name, bad)
        assert call(0, nul, w=None, wb=0) == OK, name
        # 2. a NULL data pointer, before the strides, the byte counts, the workspace and the overlaps
        for i in range(len(ptrs)):
            if i in may_null:
                continue
            p = list(ptrs)
            p[i] = None
            assert call(count, p) == ERR_PARAM, (name, i)
            assert call(SMAX // 16, p) == ERR_PARAM, (name, i)
            if dev:
                assert call(count, p, w=None) == ERR_PARAM, (name, i)
        # 4. a byte count that overflows size_t
        if name != "round":                                                   # round: active = count > the instances any workspace holds is the same class
            assert call(SMAX // 16, ptrs) == ERR_PARAM, name
            assert call(SMAX // max(lens) + 1, ptrs) == ERR_PARAM, name
        if dev:
            assert call(SMAX // (1 << 18), ptrs) == ERR_PARAM, name           # the buffers fit, the workspace does not
            # 5. the workspace: NULL, misaligned, too small
            assert call(count, ptrs, w=None) == ERR_PARAM, name
            for off in (1, 8, 64, 128):
                assert call(count, ptrs, w=WS + off) == ERR_PARAM, (name, off)
            assert call(count, ptrs, wb=wsb - 1) == ERR_PARAM, name
            assert call(count, ptrs, wb=0) == ERR_PARAM, name
            # ... d_live (and d_rounds) 4-byte aligned
            live_at = len(ptrs) - 1
            for off in (1, 2, 3):
                p = list(ptrs)
                p[live_at] += off
                assert call(count, p) == ERR_PARAM, (name, off)
            if name == "round":
                p = list(ptrs)
                p[1] += 2
                assert call(count, p) == ERR_PARAM, name
        # 6. an output that overlaps an input, another output, the workspace
        for o in range(n_in, len(ptrs)):
            for other in range(len(ptrs)):
                if other == o:
                    continue
                p = list(ptrs)
                p[o] = ptrs[other] + span[other] - 4                          # its first word is the other's last
                assert call(count, p) == ERR_PARAM, (name, o, other)
                p[o] = ptrs[other] - span[o] + 4
                assert call(count, p) == ERR_PARAM, (name, o, other)
            if dev:
                p = list(ptrs)
                p[o] = WS + wsb - 4
                assert call(count, p) == ERR_PARAM, (name, o)
                p[o] = WS - span[o] + 4
                assert call(count, p) == ERR_PARAM, (name, o)
        # a valid call (inputs may overlap each other; the optional pointers NULL) without a device is a HIP error
        if not _have_device():
            assert call(count, ptrs) == ERR_HIP, name
            for i in may_null:
                p = list(ptrs)
                p[i] = None
                assert call(count, p) == ERR_HIP, (name, i)
            if name != "round":
                p = list(ptrs)
                p[1] = p[0]
                assert call(count, p) == ERR_HIP, name
    # begin: msg_kind, then the strides and MSG_MU's length, each before the later classes
    ptrs, at = [], P
    for ln in (sk_len, 64, 32, 0):
        ptrs.append(at)
        at = (at + (count * ln if ln else 4) + 64 + 15) // 16 * 16
    for kind in (-1, 2, 7):
        assert _begin(L, param, 64, kind)(count, *ptrs, WS, wsb) == ERR_PARAM
        assert _begin(L, param, 64, kind)(0, None, None, None, None, None, 0) == ERR_PARAM
        assert _host(L, param, 64, kind)(0, None, None, None, None, None) == ERR_PARAM
    for stride in (1, sk_len - 1):
        assert _begin(L, param, 64, BYTES, sk_stride=stride)(count, *ptrs, WS, wsb) == ERR_PARAM
        assert _round(L, param, sk_stride=stride)(count, P, P + 16384, P + 32768, WS, wsb) == ERR_PARAM
        assert L.psf_mldsa_sign_end_dev(0, param, count, stride, WS, wsb, None) == ERR_PARAM
    assert _begin(L, param, 64, BYTES, msg_stride=63)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _begin(L, param, 64, BYTES, msg_stride=0)(count, *ptrs, WS, wsb) == ERR_PARAM
    for bad_len in (0, 32, 63, 65):
        assert _begin(L, param, bad_len, MU, msg_stride=128)(count, *ptrs, WS, wsb) == ERR_PARAM
    assert _begin(L, param, 64, MU, msg_stride=63)(SMAX // 16, *ptrs, None, 0) == ERR_PARAM      # the stride, before overflow and workspace
    p = list(ptrs)
    p[0] = None                                                              # a NULL pointer comes before a bad stride
    assert _begin(L, param, 64, BYTES, msg_stride=1)(count, *p, WS, wsb) == ERR_PARAM
    # round: active above count
    assert _round(L, param, active=count + 1)(count, P, P + 16384, P + 32768, WS, wsb) == ERR_PARAM
    # the host form: max_rounds in [1, 65536 / l]
    l = KL[param][1]
    hp = [P, P + 16384, P + 20000, P + 24000, P + 40000]
    for bad in (0, 65536 // l + 1, 1 << 31):
        assert _host(L, param, 64, MU, max_rounds=bad)(count, *hp) == ERR_PARAM
        assert _host(L, param, 64, MU, max_rounds=bad)(0, None, None, None, None, None) == ERR_PARAM
    # end: the workspace
    assert L.psf_mldsa_sign_end_dev(0, -1, count, 0, WS, wsb, None) == ERR_PARAM
    assert L.psf_mldsa_sign_end_dev(0, param, 0, 0, None, 0, None) == OK
    assert L.psf_mldsa_sign_end_dev(0, param, count, sk_len, None, wsb, None) == ERR_PARAM
    assert L.psf_mldsa_sign_end_dev(0, param, count, sk_len, WS + 64, wsb, None) == ERR_PARAM
    assert L.psf_mldsa_sign_end_dev(0, param, count, sk_len, WS, wsb - 1, None) == ERR_PARAM
    if not _have_device():
        assert L.psf_mldsa_sign_end_dev(0, param, count, 0, WS, _ws(L, param, count, 0), None) == ERR_HIP
    # more than 2^31 - 1 instances: unsupported, after every other check (a workspace of that size is only claimed, never touched)
    big = 1 << 31
    need = _ws(L, param, big, 0)
    far = [1 << 60, 1 << 61, (1 << 61) + (1 << 59), 1 << 62]
    assert _begin(L, param, 64, MU, sk_stride=0)(big, *far, 256, need) == ERR_UNSUPPORTED
    assert _begin(L, param, 64, MU, sk_stride=0)(big, *far, 256, need - 1) == ERR_PARAM
    assert _round(L, param, sk_stride=0)(big, far[0], far[1], far[3], 256, need) == ERR_UNSUPPORTED
    if not _have_device():
        # valid forms: one key for all, an empty message without a pointer, mu as the message, the deterministic variant, the last valid max_rounds
        assert _begin(L, param, 64, BYTES, sk_stride=0)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _begin(L, param, 64, BYTES, sk_stride=sk_len + 5, msg_stride=70)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _begin(L, param, 0, BYTES)(count, ptrs[0], None, None, ptrs[3], WS, wsb) == ERR_HIP
        assert _begin(L, param, 64, MU)(count, *ptrs, WS, wsb) == ERR_HIP
        assert _round(L, param, active=0)(count, P, None, P + 32768, WS, wsb) == ERR_HIP
        assert _host(L, param, 64, MU, max_rounds=65536 // l)(count, *hp) == ERR_HIP
        assert _host(L, param, 64, MU, sk_stride=0, max_rounds=1)(count, hp[0], hp[1], None, hp[3], None) == ERR_HIP
    assert (buf == 7).all()


def test_python_forms_without_a_device():
    import tools_amd as T
    D = T.mldsa
    for call in (lambda: D.sign_internal("ML-DSA-44", bytes(2560), [b"m", b"n"]), lambda: D.sign("ML-DSA-65", bytes(4032), b"msg", ctx=b"c"),
                 lambda: D.sign("ML-DSA-87", bytes(4896), b"msg", deterministic=True)):
        if _have_device():
            break                                                             # the calls would run: tests/test_gpu_mldsa_sign.py
        with pytest.raises(T.PsfError) as ei:
            call()
        assert ei.value.status == ERR_HIP
    with pytest.raises(ValueError):
        D.sign("ML-DSA-44", bytes(2560), b"msg", ctx=bytes(256))
    with pytest.raises(ValueError):
        D.sign_internal("ML-DSA-65", bytes(4031), [b"m"])
    with pytest.raises(ValueError):
        D.sign_internal("ML-DSA-65", bytes(4032), [b"m", b"mm"])


# ---- the restated signer and the cases --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.PARAMS))
def test_restated_signer_equals_the_model(name):
    rng = random.Random(97 + len(name) + int(name[-2:]))
    sk = M.keygen_internal(rng.randbytes(32), name)[1]
    for i in range(6):
        msg, rnd = rng.randbytes(1 + 40 * i), (bytes(32) if i % 2 else rng.randbytes(32))
        sig, attempts, fired = S.sign_trace(sk, name, m_prime=msg, rnd=rnd)
        assert sig == M.sign_internal(sk, msg, rnd, name)
        assert attempts == len(fired) and fired[-1] == 0 and all(fired[:-1])
        mu = rng.randbytes(64)
        assert S.sign_trace(sk, name, mu=mu, rnd=rnd)[0] == M.sign_internal(sk, b"", rnd, name, mu=mu)
    got = S.sign_batch(name, sk, [b"a", b"b"])
    assert [g[0] for g in got] == [M.sign_internal(sk, m, bytes(32), name) for m in (b"a", b"b")]
    assert S.sign_trace(sk, name, m_prime=b"a", max_attempts=got[0][1] - 1)[:2] == (None, 0)         # one attempt short: unsigned


def test_searched_cases_have_their_properties():
    K.check()
    for name in M.PARAMS:
        assert 1 <= len(K.case_instances(name)) <= 5


# ---- the core on the CPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mldsa_sign") / "mldsa_sign_host_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "mldsa_sign_host_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return go


def test_expand_mask_parse(run):
    """both gamma1, against BitUnpack of hashlib's stream: the nonce in both bytes, 576 and 640 bytes over five blocks"""
    rng = random.Random(51)
    lines, want = [], []
    for bits, g1 in ((18, 1 << 17), (20, 1 << 19)):
        for nonce in (0, 1, 255, 256, 0x1234, 65535):
            rho = rng.randbytes(64)
            lines.append(f"mask {bits} {(rho + nonce.to_bytes(2, 'little')).hex()}")
            want.append(" ".join(str(v) for v in M.bit_unpack(M.H(rho + nonce.to_bytes(2, "little"), 32 * bits), g1 - 1, g1)))
            assert M.expand_mask(rho, nonce, 1, g1)[0] == [int(v) for v in want[-1].split()]
    assert run(lines) == want


def _edges(g2):
    """residues at the edges of every interval of Decompose, and of the wrap at q - 1"""
    rs = {0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2}
    for i in range((Q - 1) // (2 * g2) + 1):
        for d in (-2, -1, 0, 1, 2):
            for c in (2 * g2 * i + d, 2 * g2 * i + g2 + d):
                if 0 <= c < Q:
                    rs.add(c)
    return sorted(rs)


def test_high_bits_low_bits_and_make_hint_at_every_edge(run):
    rng = random.Random(52)
    g2s = ((Q - 1) // 88, (Q - 1) // 32)
    rs = sorted(set(_edges(g2s[0])) | set(_edges(g2s[1])) | {rng.randrange(Q) for _ in range(500)})
    out = [int(v) for v in run(["bits " + " ".join(str(r) for r in rs)])[0].split()]
    want = []
    for r in rs:
        for g2 in g2s:
            want += [M.high_bits(r, g2), M.low_bits(r, g2)]
    assert out == want
    for high, g2 in enumerate(g2s):
        edges = _edges(g2)
        pairs = []
        for r in edges:
            for z in (0, 1, Q - 1, 2, Q - 2, g2, Q - g2, g2 - 1, Q - g2 + 1, rng.randrange(Q)):
                pairs.append((r, z))
        out = [int(v) for v in run([f"makehint {high} " + " ".join(f"{r} {z}" for r, z in pairs)])[0].split()]
        assert out == [M.make_hint(z, r, g2) for r, z in pairs]
        assert 0 < sum(out) < len(out)


def test_hint_bit_pack_against_hint_bit_unpack(run):
    rng = random.Random(53)
    lines, want = [], []
    for name, (k, l, eta, tau, cb, g1, g2, beta, omega) in M.PARAMS.items():
        for ones in (0, 1, omega // 2, omega - 1, omega):
            places = rng.sample(range(k * 256), ones)
            if ones == omega:
                places = rng.sample(range(256), min(omega, 256) // 2)         # many in one polynomial, bits 0 and 255 among them
                places = sorted(set(places) | {0, 255, 256 * (k - 1), 256 * k - 1})
                places += [256 + j for j in range(omega - len(places))]
            h = [[0] * 256 for _ in range(k)]
            for p in places:
                h[p // 256][p % 256] = 1
            mask = bytearray(32 * k)
            for i in range(k):
                for j in range(256):
                    if h[i][j]:
                        mask[32 * i + j // 8] |= 1 << (j % 8)
            lines.append(f"hintpack {k} {omega} {bytes(mask).hex()}")
            want.append(M.hint_bit_pack(h, omega).hex())
            assert M.hint_bit_unpack(bytes.fromhex(want[-1]), k, omega) == h
    assert run(lines) == want


def test_norm_bounds_on_both_sides(run):
    """the tests of Algorithm 7 on crafted values: ||c t0|| against gamma2 (never met in a searched instance), ||z|| against gamma1 - beta,
    ||LowBits(r)|| against gamma2 - beta"""
    lines, want = [], []
    for name, (k, l, eta, tau, cb, g1, g2, beta, omega) in M.PARAMS.items():
        for bound in (g2, g1 - beta):
            vals = [0, 1, bound - 2, bound - 1, bound, bound + 1, (Q - 1) // 2, (Q + 1) // 2, Q - bound - 1, Q - bound, Q - bound + 1, Q - bound + 2, Q - 1]
            lines.append(f"norm {bound} " + " ".join(str(v) for v in vals))
            want.append(" ".join(str(int(abs(M.mod_pm(v, Q)) >= bound)) for v in vals))
        bound = g2 - beta
        vals = [0, 1, -1, bound - 1, bound, bound + 1, -(bound - 1), -bound, -(bound + 1), g2, -g2 + 1, -g2]
        lines.append(f"low {bound} " + " ".join(str(v) for v in vals))
        want.append(" ".join(str(int(abs(v) >= bound)) for v in vals))
    assert run(lines) == want
    assert want[0].split()[3:6] == ["0", "1", "1"]


def test_kappa_overflow_rule(run):
    """an attempt at kappa draws the nonces kappa ... kappa + l - 1: it may start while kappa + l <= 65536"""
    for l in (4, 5, 7):
        last = (65536 // l) * l                                               # kappa after 65536 // l attempts
        vals = [0, l, last - l, last, last + l, 65536 - l, 65536 - l + 1, 65536]
        assert run([f"kappa {l} " + " ".join(str(v) for v in vals)]) == [" ".join(str(int(v + l > 65536)) for v in vals)]
        assert int(last - l + l > 65536) == 0 and int(last + l > 65536) == 1
