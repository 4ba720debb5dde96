// The censored-outcome model's latent update (log-normal AFT, Tobit): each row
// has a value b_i and a status -- 0 observed (z_i = b_i), 1 right-censored
// (z_i > b_i), 2 left-censored (z_i <= b_i) -- and z_i ~ N(psi_i, 1 / tau).  A
// censored row's latent is a truncated normal (Chib 1992): with psi' = (psi_i -
// b_i) sqrt(tau), u ~ N(psi', 1) on u > 0 (status 1) or u <= 0 (status 2) by the
// rejection sampler TruncatedNormal (samplers.hpp), used as it is, and z_i =
// b_i + u / sqrt(tau).  The same pass collects the log-likelihood
//   observed        1/2 log tau - 1/2 tau (b - psi)^2     (-1/2 log 2 pi dropped)
//   right-censored  log Phi(psi')
//   left-censored   log Phi(-psi')
// and sum_i z_i, the centring term of X~^T z.  tau is drawn beforehand by the
// linear model's kernels with z for y (chain.hip).  The stand-alone sampler
// bbx_device_censored_normal lives here too.
//
// The row kernel, its launch and the sampler's host front are
// latent_rows.hpp's; this file states the per-row expressions.
//
// One lane per row.  An observed lane copies its value and takes no trial; a
// censored lane's trial is one Philox block, accepted with probability >= 1/2
// (psi' on the allowed side) or >= 0.76 (Robert's exponential), so a wave
// waits for its slowest censored lane while its observed lanes sit idle: the
// cost follows the waves that hold a censored row, not the censored share.
// Trial t of row i reads Philox(seed, stream, i, t): the draw is a function of
// (seed, stream, i, psi_i, b_i, status_i, tau) alone, whatever the grid.
#include <cmath>

#include "latent_rows.hpp"

namespace bbx {

namespace {

// The latent of one row and its log-likelihood term.  rt = sqrt(tau), hlt =
// 1/2 log tau.  A psi' that is not finite (psi_i not finite, or the product
// out of range) gives a NaN term and, on a censored row, a NaN latent; no row
// loops on one.
__device__ inline double censored_row(uint64_t seed, uint64_t stream, int64_t i,
                                      double psi, double b, unsigned status,
                                      double tau, double rt, double hlt,
                                      double* term) {
  const double p = (psi - b) * rt;
  const bool bad = !(fabs(p) <= 1.7e308);
  if (status == 0) {
    *term = bad ? p - p : hlt - 0.5 * (p * p);
    return b;
  }
  if (bad) {
    *term = p - p;
    return p - p;
  }
  const bool positive = status == 1;
  *term = log_norm_cdf(positive ? p : -p);
  const double u = TruncatedNormal::draw_trials(
      [&](uint32_t t) { return Philox(seed, stream, (uint64_t)i, t); }, p,
      positive, nullptr);
  return b + u / rt;
}

// The sums are those of the log-likelihood terms and of z_i, under tau.
struct CensoredRows {
  const double* __restrict__ bound;
  const unsigned char* __restrict__ status;
  const double* __restrict__ psi;
  double* __restrict__ latent;
  static constexpr bool reads_tau = true;
  struct Once {
    double tau, rt, hlt;
  };
  __device__ Once once(double tau) const {
    return {tau, sqrt(tau), 0.5 * log(tau)};
  }
  __device__ double draw(const Once& k, uint64_t seed, uint64_t stream,
                         int64_t i) const {
    double term;
    return censored_row(seed, stream, i, psi[i], bound[i], status[i], k.tau,
                        k.rt, k.hlt, &term);
  }
  __device__ void row(const Once& k, uint64_t seed, uint64_t stream, int64_t i,
                      double& ll, double& w) const {
    const double z = censored_row(seed, stream, i, psi[i], bound[i], status[i],
                                  k.tau, k.rt, k.hlt, &ll);
    latent[i] = z;
    w = z;
  }
};

}  // namespace

template <>
int launch_latent_rows<BBX_MODEL_CENSORED>(bbx_chain* c, uint64_t stream,
                                           int* row_blocks) {
  return launch_rows(c, stream,
                     CensoredRows{c->outcome.as<double>(),
                                  c->status.as<unsigned char>(),
                                  c->psi.as<double>(), c->latent.as<double>()},
                     row_blocks);
}

}  // namespace bbx

using namespace bbx;

static int device_censored_normal_impl(int device, uint64_t seed,
                                       int64_t n_draw, const double* psi,
                                       const double* bound,
                                       const unsigned char* status, double tau,
                                       double* out) {
  const std::string who = "bbx_device_censored_normal: ";
  if (n_draw < 0) return fail(BBX_ERR_INVALID, who + "n_draw < 0");
  if (!psi || !bound || !status || !out)
    return fail(BBX_ERR_INVALID, who + "NULL argument");
  if (!(tau > 0.) || !std::isfinite(tau))
    return fail(BBX_ERR_INVALID,
                who + "tau must be finite and positive");
  for (int64_t i = 0; i < n_draw; ++i) {
    if (status[i] > 2)
      return fail(BBX_ERR_INVALID, who + "status[" +
                                       std::to_string(i) + "] is not 0, 1 or 2");
    if (!std::isfinite(bound[i]))
      return fail(BBX_ERR_INVALID, who + "bound[" +
                                       std::to_string(i) + "] is not finite");
  }
  const size_t nb = sizeof(double) * (size_t)n_draw;
  return device_latent_draw(
      who, device, seed, n_draw, tau,
      {{psi, nb}, {bound, nb}, {status, (size_t)n_draw}},
      [](const DevMem* d) {
        return CensoredRows{d[1].as<double>(), d[2].as<unsigned char>(),
                            d[0].as<double>(), nullptr};
      },
      out);
}

extern "C" int bbx_device_censored_normal(int device, uint64_t seed,
                                          int64_t n_draw, const double* psi,
                                          const double* bound,
                                          const unsigned char* status,
                                          double tau, double* out) {
  return no_throw([&]() -> int {
    return device_censored_normal_impl(device, seed, n_draw, psi, bound, status,
                                       tau, out);
  });
}
