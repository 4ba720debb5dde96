// Posterior prediction and pointwise predictive scores of the censored-outcome
// model (log-normal AFT, Tobit) from draws of the coefficients and of the
// precision tau: the streaming summary of predict.hip (predict_summary.hpp) in
// one more instantiation, and the survival summary S(c | x) = 1 - Phi((c - eta)
// sqrt(tau)) at given points c of the latent scale, in a translation unit of
// its own.
#include "predict_summary.hpp"

using namespace bbx;
using namespace bbx::pred;

namespace {

// One thread per (row i, point j), idx = j n + i: the Moments of S_j over the
// draws, pass by pass as predict_summary_kernel keeps its own.  state[2][n T];
// out: mean[T][n], then sd[T][n].
__global__ __launch_bounds__(PRED_BLOCK) void censored_survival_kernel(
    PredArgs a, int64_t n_point, const double* __restrict__ points,
    double* __restrict__ state, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * PRED_BLOCK + threadIdx.x;
  const int64_t n = a.n, total = n * n_point;
  if (idx >= total) return;
  const int64_t i = idx % n;
  const double pt = points[idx / n];
  Moments mom;
  if (a.k0 > 0) mom.load(state, total, idx);
  const double off = a.offset ? a.offset[i] : 0.;
  for (int d = 0; d < a.kn; ++d) {
    double eta = a.eta[(int64_t)d * n + i];
    if (a.offset) eta += off;
    const double rt = sqrt(a.tau[a.k0 + d]);
    // 1 - Phi(x) = erfc(x / sqrt 2) / 2: absolute error ~1e-16
    const double s = 0.5 * erfc(0.70710678118654752440 * ((pt - eta) * rt));
    mom.push(s, (double)(a.k0 + d + 1));
  }
  if (a.k0 + a.kn < a.n_draw) {
    mom.store(state, total, idx);
    return;
  }
  mom.finish((double)a.n_draw, out, out + total, idx);
}

}  // namespace

// bbx_design_predictive_summary with eta as the predicted quantity and, with
// an outcome (y, status), the full density: 1/2 log(tau_s / (2 pi)) - 1/2 tau_s
// (y - eta)^2 + c on an observed row, log Phi(-a) + c on a right-censored and
// log Phi(a) + c on a left-censored one, a = (y - eta) sqrt(tau_s), tau_s the
// precision of draw s, through the same driver (predictive_summary_impl): tau
// travels in the linear model's per-draw slots, the status in the row slot of
// the logit model's n_trial.  exp_mean != 0: the predicted quantity is exp(eta)
// (the log-normal AFT model's median time).  With n_point > 0 the survival
// summary runs on every pass's linear predictors beside it.
extern "C" int bbx_design_predictive_summary_censored(
    bbx_design* design, int64_t n_draw, int exp_mean, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const unsigned char* status, const double* ll_const, int draws_per_pass,
    double* mean, double* sd, double* lpd, double* ll_mean, double* ll_var,
    double* mu_draws, int64_t n_point, const double* points, double* surv_mean,
    double* surv_sd) {
  const char* who = "bbx_design_predictive_summary_censored: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if (y && (!status || !obs_prec || !lpd || !ll_mean || !ll_var))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "an outcome is given but status, obs_prec, "
                                     "lpd, ll_mean or ll_var is NULL");
  if (y && n_draw < 2)
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "scoring an outcome needs at least 2 "
                                     "draws");
  if (n_point < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "n_point must not be negative");
  if (n_point > 0 && (!points || !obs_prec || !surv_mean || !surv_sd))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "n_point > 0 but points, obs_prec, "
                                     "surv_mean or surv_sd is NULL");
  if (obs_prec && (y || n_point > 0))
    for (int64_t d = 0; d < n_draw; ++d)
      if (!(obs_prec[d] > 0.) || !std::isfinite(obs_prec[d]))
        return fail(BBX_ERR_INVALID, std::string(who) + "obs_prec[" +
                                         std::to_string(d) +
                                         "] is not finite and positive");
  for (int64_t j = 0; j < n_point; ++j)
    if (points[j] != points[j])
      return fail(BBX_ERR_INVALID, std::string(who) + "points[" +
                                       std::to_string(j) + "] is a NaN");
  std::vector<double> status_row;
  if (y) {
    status_row.resize((size_t)design->n);
    for (int64_t i = 0; i < design->n; ++i) {
      if (!std::isfinite(y[i]))
        return fail(BBX_ERR_INVALID, std::string(who) + "y[" +
                                         std::to_string(i) + "] is not finite");
      if (status[i] > 2)
        return fail(BBX_ERR_INVALID, std::string(who) + "status[" +
                                         std::to_string(i) +
                                         "] is not 0, 1 or 2");
      status_row[(size_t)i] = (double)status[i];
    }
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const int64_t total = design->n * n_point;
    const size_t tb = sizeof(double) * (size_t)total;
    DevMem d_points, d_state, d_out;
    if (n_point > 0) {
      BBX_TRY(d_points.alloc(sizeof(double) * (size_t)n_point));
      BBX_TRY(d_state.alloc(2 * tb));
      BBX_TRY(d_out.alloc(2 * tb));
      BBX_HIP(hipMemcpyAsync(d_points.ptr, points,
                             sizeof(double) * (size_t)n_point,
                             hipMemcpyHostToDevice, design->stream));
    }
    // (obs_prec: uploaded by the driver whenever it is given)
    const PredCall q{design, exp_mean ? PRED_LOGNORMAL : PRED_CENSORED, n_draw,
                     coef,   n_point > 0 || y ? obs_prec : nullptr,
                     offset, y,
                     y ? status_row.data() : nullptr,
                     ll_const, draws_per_pass,
                     mean,   sd, lpd, ll_mean, ll_var, mu_draws};
    BBX_TRY(predictive_summary_impl(
        q, [&](hipStream_t s, bool score, const PredArgs& a) {
          if (exp_mean)
            launch_summary<PRED_LOGNORMAL>(s, score, a);
          else
            launch_summary<PRED_CENSORED>(s, score, a);
          if (n_point > 0) {
            const dim3 grid((unsigned)((total + PRED_BLOCK - 1) / PRED_BLOCK));
            BBX_LAUNCH(censored_survival_kernel, grid, dim3(PRED_BLOCK), 0, s,
                       a, n_point, d_points.as<const double>(),
                       d_state.as<double>(), d_out.as<double>());
          }
        }));
    // (the driver has synchronised the stream behind the last pass)
    if (n_point > 0) {
      BBX_HIP(hipMemcpy(surv_mean, d_out.ptr, tb, hipMemcpyDeviceToHost));
      BBX_HIP(hipMemcpy(surv_sd, d_out.as<double>() + total, tb,
                        hipMemcpyDeviceToHost));
    }
    return BBX_OK;
  });
}
