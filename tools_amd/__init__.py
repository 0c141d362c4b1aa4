"""tools_amd -- MI355X-native preimage sampling (PSF trait of qfall/tools) over libpsf_mi355x.so.

Host-side mirror of the reference's interface for this path (src/primitive/psf.rs:39-81):
GadgetParameters.init_default, PSFPerturbation / PSFGPV / PSFGPVRing with
trap_gen / samp_d / samp_p / f_a / check_domain; compression (LossyCompressionFIPS203), encodings (utils::common_encodings),
rq (MatPolynomialRingZq matrix products, and the products of the cyclic ring X^n - 1), sample (uniform, centred-binomial and
discrete-Gaussian fills), fips203 (SHA3 / SHAKE, the byte-exact samplers of FIPS 203 and its NTT-domain representation) and mlkem (batched
ML-KEM KeyGen / Encaps / Decaps and the input checks, bytes in and bytes out), fips204 (the byte-exact samplers of FIPS 204 and its NTT-domain
order) and mldsa (batched ML-DSA KeyGen, Sign and Verify), slhdsa (batched SLH-DSA KeyGen, Sign and Verify for the SHAKE parameter sets),
sha2 (batched SHA-256 / SHA-512) and slhdsa_sha2 (batched SLH-DSA KeyGen and Verify for the SHA-2 parameter sets).
Everything computes on the GPU through the C ABI.
"""
from ._ffi import PsfError, LIB_PATH  # noqa: F401
from .psf import GadgetParameters, GadgetParametersRing, PSFPerturbation, PSFGPV, PSFGPVRing  # noqa: F401
from . import gadget  # noqa: F401
from . import textio  # noqa: F401
from . import serde_json  # noqa: F401
from . import compression  # noqa: F401
from . import encodings  # noqa: F401
from . import rq  # noqa: F401
from . import sample  # noqa: F401
from . import fips203  # noqa: F401
from . import mlkem  # noqa: F401
from . import fips204  # noqa: F401
from . import mldsa  # noqa: F401
from . import slhdsa  # noqa: F401
from . import sha2  # noqa: F401
from . import slhdsa_sha2  # noqa: F401
