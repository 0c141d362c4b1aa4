"""The harness of the device tests of SLH-DSA's SHA-2 sets (tests/test_gpu_slhdsa_sha2.py): tests/helpers/slhdsa_gpu.py's two functions over the sizes
of tests/helpers/slhdsa_sha2_model.py -- every buffer one byte past a 16-byte boundary with guard bytes around every output, a workspace filled with a
non-zero byte, the guards checked, and the workspace all zero after KeyGen; `offs`, `pk_stride`, `msg_stride` and `gap` as described there.  Nothing
here imports the library or torch: both are arguments."""
from tests.helpers import slhdsa_gpu as G
from tests.helpers import slhdsa_sha2_model as M
from tests.helpers.slhdsa_gpu import Scratch, offsets  # noqa: F401


def dev_keygen(torch, D, name, sk_seeds, sk_prfs, pk_seeds, offs=None):
    """keygen_dev over the instances; returns (pks, sks) as lists of bytes"""
    return G.dev_keygen(torch, D, name, sk_seeds, sk_prfs, pk_seeds, offs=offs, model=M)


def dev_verify(torch, D, name, pks, msgs, sigs, offs=None, pk_stride=None, msg_stride=None, gap=0xC3):
    """verify_dev over the instances; `pks`: a list with one key per instance, or bytes (one key for all: pk_stride = 0); returns ok as a list"""
    return G.dev_verify(torch, D, name, pks, msgs, sigs, offs=offs, pk_stride=pk_stride, msg_stride=msg_stride, gap=gap, model=M)
