// psf_slhdsa_sha2_api.hpp -- what psf_slhdsa_sha2.hip (SLH-DSA KeyGen / Verify for the SHA-2 sets) offers psf_slhdsa_sha2_sign.hip (signing for them), as
// psf_slhdsa_api.hpp does for the SHAKE sets: the parameter set of a `param` (PSF_SLHDSA_SHA2_*), defined in psf_slhdsa_sha2.hip.
#pragma once
#include "psf_slhdsa_sha2_core.hpp"

namespace psf {
namespace slh2 {

bool set_of(int param, Params* p);

}  // namespace slh2
}  // namespace psf
