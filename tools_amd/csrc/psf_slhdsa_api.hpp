// psf_slhdsa_api.hpp -- what psf_slhdsa.hip (SLH-DSA KeyGen / Verify) offers psf_slhdsa_sign.hip (SLH-DSA signing), as psf_mldsa_api.hpp does for
// ML-DSA: the parameter set of a `param`, defined in psf_slhdsa.hip.
#pragma once
#include "psf_slhdsa_core.hpp"

namespace psf {
namespace slh {

bool set_of(int param, Params* p);

}  // namespace slh
}  // namespace psf
