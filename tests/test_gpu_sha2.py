"""Batched SHA-256 and SHA-512 on the MI355X (tools_amd/sha2.py, psf_sha2_dev / psf_sha2) against hashlib: both functions at the message lengths around
every padding edge of both (pad fits, pad spills into a block of its own, whole blocks), at batch sizes below, at and across a wave and a workgroup,
with packed, padded and misaligned strides, truncated digests (FIPS 205's Trunc), the empty message with a NULL input, and the host form.  Every output
sits between guard bytes at a pointer one byte past an aligned address."""
import hashlib
import random

import numpy as np
import pytest

from tests.helpers.mlkem_gpu import _out, _put, _take

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127, 128, 129, 200, 1000]
COUNTS = [1, 3, 67, 131]
FUNCS = {0: (hashlib.sha256, 32), 1: (hashlib.sha512, 64)}


@pytest.fixture(scope="module")
def H():
    import tools_amd
    return tools_amd.sha2


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _messages(func, count, in_len):
    rng = random.Random(1009 * func + 31 * count + in_len)
    return [rng.randbytes(in_len) for _ in range(count)]


def _dev(torch, H, func, msgs, out_len, in_pad=0, out_pad=0, off=1):
    """sha2_dev over the messages, message c at in_len + in_pad from the one before, digest c at out_len + out_pad; returns the digests"""
    count, in_len = len(msgs), len(msgs[0])
    in_stride, out_stride = in_len + in_pad, out_len + out_pad
    bi, pi = _put(torch, [m + bytes(in_pad) for m in msgs], off) if in_stride else (None, None)
    nbytes = (count - 1) * out_stride + out_len
    bo, po = _out(torch, nbytes, off)
    torch.cuda.synchronize()
    H.sha2_dev(func, count, pi, in_len, po, out_len, in_stride=in_stride, out_stride=out_stride)
    flat = b"".join(_take(torch, bo, nbytes, nbytes, (func, count, in_len), off))
    gaps = [flat[c * out_stride + out_len:(c + 1) * out_stride] for c in range(count - 1)]
    del bi
    return [flat[c * out_stride:c * out_stride + out_len] for c in range(count)], gaps


@pytest.mark.parametrize("func", sorted(FUNCS))
@pytest.mark.parametrize("count", COUNTS)
def test_digests_equal_hashlib_at_every_length(torch, H, func, count):
    h, size = FUNCS[func]
    for in_len in LENGTHS:
        msgs = _messages(func, count, in_len)
        got, _ = _dev(torch, H, func, msgs, size)
        assert got == [h(m).digest() for m in msgs], (func, count, in_len)


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_padded_and_misaligned_strides_and_truncated_digests(torch, H, func):
    from tests.helpers.mlkem_gpu import FILL
    h, size = FUNCS[func]
    for in_len, in_pad, out_pad, off in ((64, 0, 0, 0), (64, 4, 8, 0), (65, 3, 5, 1), (119, 1, 1, 2), (128, 7, 3, 3), (56, 8, 0, 4)):
        for out_len in [16, 24, 32] + ([64] if size == 64 else []):
            msgs = _messages(func, 67, in_len)
            got, gaps = _dev(torch, H, func, msgs, out_len, in_pad, out_pad, off)
            assert got == [h(m).digest()[:out_len] for m in msgs], (func, in_len, in_pad, out_pad, off, out_len)
            assert all(g == bytes([FILL]) * out_pad for g in gaps), "wrote between two digests"


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_the_empty_message_needs_no_input_pointer(torch, H, func):
    h, size = FUNCS[func]
    bo, po = _out(torch, 5 * size)
    H.sha2_dev(func, 5, None, 0, po, size)
    assert _take(torch, bo, 5 * size, size, "empty") == [h(b"").digest()] * 5


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_the_host_form_equals_hashlib(H, func):
    h, size = FUNCS[func]
    for in_len in (0, 55, 56, 64, 111, 112, 128, 1000):
        msgs = _messages(func, 67, in_len)
        assert [bytes(r) for r in H.sha2(func, msgs)] == [h(m).digest() for m in msgs], (func, in_len)
        assert [bytes(r) for r in H.sha2(func, np.frombuffer(b"".join(msgs), np.uint8).reshape(67, in_len), 16)] == [h(m).digest()[:16] for m in msgs]
