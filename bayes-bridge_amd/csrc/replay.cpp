// libbbx_hostrng.so, second part: a sequential host replay of the device
// chain's Philox draws (normals, Polya-Gamma, tilted stable, truncated normal,
// inverse Gaussian, Gamma), element by
// element, for the tests that pin the kernels draw by draw
// (tests/test_hip_sampler_replay.py).  The loops are in replay_impl.hpp.
// Plain C++ (g++), no HIP.
#include "../../include/bbx.h"
#include "replay_impl.hpp"

namespace replay_device_forms_api {   // replay_device_forms.cpp
void polya_gamma(uint64_t seed, uint64_t stream, int64_t n, int shape_is_double,
                 const void* shape, const double* tilt, double* out,
                 int32_t* attempts, int32_t* restarts);
void tilted_stable(uint64_t seed, uint64_t stream, int64_t n, double a,
                   const double* tilt, double* out, int32_t* winner);
void truncated_normal(uint64_t seed, uint64_t stream, int64_t n,
                      const double* psi, const unsigned char* positive,
                      double* out, int32_t* trials);
}  // namespace replay_device_forms_api

namespace ref = replay_reference_forms;

extern "C" {

int bbx_replay_philox_block(const uint32_t* counter, const uint32_t* key,
                            uint32_t* out) {
  if (!counter || !key || !out) return BBX_ERR_INVALID;
  ref::HostPhilox::block(counter, key, out);
  return BBX_OK;
}

int bbx_replay_philox_counter(uint64_t seed, uint64_t stream, uint64_t index,
                              uint32_t trial, uint32_t* counter, uint32_t* key) {
  if (!counter || !key) return BBX_ERR_INVALID;
  const ref::HostPhilox g(seed, stream, index, trial);
  for (int k = 0; k < 4; ++k) counter[k] = g.ctr[k];
  key[0] = g.key[0];
  key[1] = g.key[1];
  return BBX_OK;
}

int bbx_replay_uniform(uint64_t seed, uint64_t stream, uint64_t index,
                       uint32_t trial, int64_t n, double* out) {
  if (!out || n < 0) return BBX_ERR_INVALID;
  ref::uniforms(seed, stream, index, trial, n, out);
  return BBX_OK;
}

int bbx_replay_normal(uint64_t seed, uint64_t stream, int64_t n, double* out) {
  if (!out || n < 0) return BBX_ERR_INVALID;
  ref::normal(seed, stream, n, out);
  return BBX_OK;
}

int bbx_replay_polya_gamma(uint64_t seed, uint64_t stream, int64_t n,
                           int shape_is_double, const void* shape,
                           const double* tilt, int variant, double* out,
                           int32_t* attempts, int32_t* restarts) {
  if (!shape || !tilt || !out || n < 0 || (variant != 0 && variant != 1))
    return BBX_ERR_INVALID;
  if (variant == 1)
    replay_device_forms_api::polya_gamma(seed, stream, n, shape_is_double, shape,
                                         tilt, out, attempts, restarts);
  else if (shape_is_double)
    ref::polya_gamma(seed, stream, n, static_cast<const double*>(shape), tilt,
                     out, attempts, restarts);
  else
    ref::polya_gamma(seed, stream, n, static_cast<const int32_t*>(shape), tilt,
                     out, attempts, restarts);
  return BBX_OK;
}

int bbx_replay_tilted_stable(uint64_t seed, uint64_t stream, int64_t n,
                             double char_exp, const double* tilt, int variant,
                             double* out, int32_t* winner) {
  if (!tilt || !out || n < 0 || (variant != 0 && variant != 1))
    return BBX_ERR_INVALID;
  if (!(char_exp > 0.) || !(char_exp < 1.)) return BBX_ERR_INVALID;
  for (int64_t j = 0; j < n; ++j)
    if (!(tilt[j] >= 0.) || !(tilt[j] <= 1.7e308)) return BBX_ERR_INVALID;
  if (variant == 1)
    replay_device_forms_api::tilted_stable(seed, stream, n, char_exp, tilt, out,
                                           winner);
  else
    ref::tilted_stable(seed, stream, n, char_exp, tilt, out, winner);
  return BBX_OK;
}

int bbx_replay_truncated_normal(uint64_t seed, uint64_t stream, int64_t n,
                                const double* psi,
                                const unsigned char* positive, int variant,
                                double* out, int32_t* trials) {
  if (!psi || !positive || !out || n < 0 || (variant != 0 && variant != 1))
    return BBX_ERR_INVALID;
  if (variant == 1)
    replay_device_forms_api::truncated_normal(seed, stream, n, psi, positive,
                                              out, trials);
  else
    ref::truncated_normal(seed, stream, n, psi, positive, out, trials);
  return BBX_OK;
}

int bbx_replay_inverse_gaussian(uint64_t seed, uint64_t stream, int64_t n,
                                const double* m, double lambda, int variant,
                                double* out, int32_t* branch, double* margin) {
  if (!m || !out || n < 0 || (variant != 0 && variant != 1))
    return BBX_ERR_INVALID;
  if (!(lambda > 0.)) return BBX_ERR_INVALID;
  // (no device form of its own: both variants are the one expression)
  ref::inverse_gaussian(seed, stream, n, m, lambda, out, branch, margin);
  return BBX_OK;
}

int bbx_replay_gamma(uint64_t seed, uint64_t stream, uint64_t index,
                     int64_t n, double shape, double* out) {
  if (!out || n < 0 || !(shape > 0.)) return BBX_ERR_INVALID;
  for (int64_t k = 0; k < n; ++k)
    out[k] = ref::gamma(seed, stream, index + (uint64_t)k, shape);
  return BBX_OK;
}

}  // extern "C"
