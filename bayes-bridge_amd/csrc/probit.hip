// The probit model's latent update: z_i | beta ~ N(psi_i, 1) restricted to
// z > 0 (y_i = 1) or z <= 0 (y_i = 0) -- Albert & Chib (1993) -- drawn by the
// rejection sampler TruncatedNormal (samplers.hpp), with the log-likelihood
// sum_i log Phi(+-psi_i) and sum_i z_i, the centring term of X~^T z, collected
// on the way.  The stand-alone sampler bbx_device_truncated_normal lives here
// too.
//
// The row kernel, its launch and the sampler's host front are
// latent_rows.hpp's; this file states the per-row expressions.
//
// One lane per row.  A trial is one Philox block, one log and either a sqrt
// and a cospi or an exp; every trial is accepted with probability >= 1/2, so
// a wave of 64 rows waits ~7 trials for its slowest lane.  Trial t of element i
// reads Philox(seed, stream, i, t): the draw is a function of (seed, stream,
// i, psi_i, y_i) alone, whatever the grid.
#include <cmath>

#include "latent_rows.hpp"

namespace bbx {

namespace {

__device__ inline double probit_draw(uint64_t seed, uint64_t stream, int64_t i,
                                     double psi, bool positive) {
  if (!(fabs(psi) <= 1.7e308)) return psi - psi;
  return TruncatedNormal::draw_trials(
      [&](uint32_t t) { return Philox(seed, stream, (uint64_t)i, t); }, psi,
      positive, nullptr);
}

// Y: double (a chain's outcome) or unsigned char (the stand-alone sampler's
// `positive`); the sums are those of log Phi(s_i psi_i) and of z_i.
template <class Y>
struct ProbitRows {
  const Y* __restrict__ y;
  const double* __restrict__ psi;
  double* __restrict__ latent;
  static constexpr bool reads_tau = false;
  struct Once {};
  __device__ Once once(double) const { return {}; }
  __device__ double draw(const Once&, uint64_t seed, uint64_t stream,
                         int64_t i) const {
    return probit_draw(seed, stream, i, psi[i], y[i] != 0);
  }
  __device__ void row(const Once&, uint64_t seed, uint64_t stream, int64_t i,
                      double& ll, double& w) const {
    const double eta = psi[i];
    const bool positive = y[i] != 0.;
    const double z = probit_draw(seed, stream, i, eta, positive);
    latent[i] = z;
    w = z;
    ll = log_norm_cdf(positive ? eta : -eta);
  }
};

}  // namespace

template <>
int launch_latent_rows<BBX_MODEL_PROBIT>(bbx_chain* c, uint64_t stream,
                                         int* row_blocks) {
  return launch_rows(c, stream,
                     ProbitRows<double>{c->outcome.as<double>(),
                                        c->psi.as<double>(),
                                        c->latent.as<double>()},
                     row_blocks);
}

}  // namespace bbx

using namespace bbx;

static int device_truncated_normal_impl(int device, uint64_t seed,
                                        int64_t n_draw, const double* psi,
                                        const unsigned char* positive,
                                        double* out) {
  const std::string who = "bbx_device_truncated_normal: ";
  if (n_draw < 0) return fail(BBX_ERR_INVALID, who + "n_draw < 0");
  if (!psi || !positive || !out)
    return fail(BBX_ERR_INVALID, who + "NULL argument");
  return device_latent_draw(
      who, device, seed, n_draw, 0.,
      {{psi, sizeof(double) * (size_t)n_draw}, {positive, (size_t)n_draw}},
      [](const DevMem* d) {
        return ProbitRows<unsigned char>{d[1].as<unsigned char>(),
                                         d[0].as<double>(), nullptr};
      },
      out);
}

extern "C" int bbx_device_truncated_normal(int device, uint64_t seed,
                                           int64_t n_draw, const double* psi,
                                           const unsigned char* positive,
                                           double* out) {
  return no_throw([&]() -> int {
    return device_truncated_normal_impl(device, seed, n_draw, psi, positive,
                                        out);
  });
}
