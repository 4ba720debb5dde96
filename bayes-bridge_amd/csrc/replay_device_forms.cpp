// Variant 1 of the host replay (replay_impl.hpp): the sampler templates once
// more, in a namespace of their own, with the device's forms of the arithmetic
// -- pos_pow's roots and integer powers, right_mass_direct,
// series_accept_direct -- evaluated by the host's libm.
#define BBX_REPLAY_DEVICE_FORMS 1
#include "replay_impl.hpp"

namespace replay_device_forms_api {

void polya_gamma(uint64_t seed, uint64_t stream, int64_t n, int shape_is_double,
                 const void* shape, const double* tilt, double* out,
                 int32_t* attempts, int32_t* restarts) {
  if (shape_is_double)
    replay_device_forms::polya_gamma(seed, stream, n,
                                     static_cast<const double*>(shape), tilt,
                                     out, attempts, restarts);
  else
    replay_device_forms::polya_gamma(seed, stream, n,
                                     static_cast<const int32_t*>(shape), tilt,
                                     out, attempts, restarts);
}

void tilted_stable(uint64_t seed, uint64_t stream, int64_t n, double a,
                   const double* tilt, double* out, int32_t* winner) {
  replay_device_forms::tilted_stable(seed, stream, n, a, tilt, out, winner);
}

void truncated_normal(uint64_t seed, uint64_t stream, int64_t n,
                      const double* psi, const unsigned char* positive,
                      double* out, int32_t* trials) {
  replay_device_forms::truncated_normal(seed, stream, n, psi, positive, out,
                                        trials);
}

}  // namespace replay_device_forms_api
