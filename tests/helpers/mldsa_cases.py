"""Sampler inputs with a stated property, shared by tests/test_mldsa_core_cpu.py and tests/test_gpu_fips204.py.  They were found by a search over
seed(tag, i, n) with the model (tests/helpers/mldsa_model.py); check() asserts with the model that each still has its property.

What cannot be found: a RejNTTPoly stream that needs a sixth block has more than 24 rejections among its first 280 candidates at a rejection rate of
0.00098 per candidate, and a SampleInBall that needs a second block has more than 68 rejections among its first 128 bytes at a rejection rate below 1/4:
both have probability below 2^-100.  Their caps are exercised through max_blocks in the CPU test instead."""
import hashlib

from tests.helpers import mldsa_model as M


def seed(tag, i, n):
    return hashlib.shake_256(b"psf-mldsa-" + tag + i.to_bytes(4, "little")).digest(n)


# RejNTTPoly, 34 bytes: a rejected candidate in the first block and in the last (fifth) block needed
NTT_REJECTS_FIRST_AND_LAST = [seed(b"ntt", 2715, 34), seed(b"ntt", 3286, 34)]
# RejBoundedPoly, 64 bytes (the nonce is 0).  eta = 2 needs one block (272 half bytes, 15/16 accepted) or two about equally often; eta = 4 needs two
# (9/16 accepted), and a third with probability near 10^-5.  Every one of them has rejected candidates in its first and in its last block.
BOUNDED2_ONE_BLOCK = seed(b"b2", 1, 64)
BOUNDED2_TWO_BLOCKS = seed(b"b2", 0, 64)
BOUNDED4_THREE_BLOCKS = seed(b"b4", 40979, 64)
BOUNDED4_TWO_BLOCKS = seed(b"b4", 0, 64)


def check():
    for s in NTT_REJECTS_FIRST_AND_LAST:
        st = {}
        M.rej_ntt_poly(s, st)
        assert st["blocks"] == 5 and st["rejected"][0] > 0 and st["rejected"][-1] > 0, st
    for s, eta, blocks in ((BOUNDED2_ONE_BLOCK, 2, 1), (BOUNDED2_TWO_BLOCKS, 2, 2), (BOUNDED4_TWO_BLOCKS, 4, 2), (BOUNDED4_THREE_BLOCKS, 4, 3)):
        st = {}
        M.rej_bounded_poly(s + bytes(2), eta, st)
        assert st["blocks"] == blocks and st["rejected"][0] > 0 and st["rejected"][-1] > 0, (eta, st)
