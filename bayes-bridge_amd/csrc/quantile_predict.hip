// Posterior prediction and pointwise predictive scores of the quantile
// regression model from draws of the coefficients and of the precision tau:
// the streaming summary of predict.hip (predict_summary.hpp) in one more
// instantiation, in a translation unit of its own.
#include "predict_summary.hpp"

using namespace bbx;
using namespace bbx::pred;

// bbx_design_predictive_summary with eta as the predicted quantity and, with
// an outcome, the asymmetric-Laplace density log tau_s + log(q (1 - q)) - tau_s
// rho_q(y - eta) + c, tau_s the precision of draw s and rho_q(r) = r (q - 1[r <
// 0]), through the same driver (predictive_summary_impl): tau and the draw's
// constant travel in the linear model's per-draw slots, q where Student-t's df
// does.
extern "C" int bbx_design_predictive_summary_quantile(
    bbx_design* design, int64_t n_draw, double quantile, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws) {
  const char* who = "bbx_design_predictive_summary_quantile: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if (!(quantile > 0.) || !(quantile < 1.))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "quantile must lie in (0, 1)");
  if (y && (!obs_prec || !lpd || !ll_mean || !ll_var))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "an outcome is given but obs_prec, lpd, "
                                     "ll_mean or ll_var is NULL");
  if (y && n_draw < 2)
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "scoring an outcome needs at least 2 "
                                     "draws");
  if (y) {
    for (int64_t d = 0; d < n_draw; ++d)
      if (!(obs_prec[d] > 0.) || !std::isfinite(obs_prec[d]))
        return fail(BBX_ERR_INVALID, std::string(who) + "obs_prec[" +
                                         std::to_string(d) +
                                         "] is not finite and positive");
    for (int64_t i = 0; i < design->n; ++i)
      if (!std::isfinite(y[i]))
        return fail(BBX_ERR_INVALID, std::string(who) + "y[" +
                                         std::to_string(i) + "] is not finite");
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const PredCall q{design, PRED_QUANTILE, n_draw,  coef,     obs_prec,
                     offset, y,              nullptr, ll_const, draws_per_pass,
                     mean,   sd,             lpd,     ll_mean,  ll_var,
                     mu_draws, quantile};
    return predictive_summary_impl(q, launch_summary<PRED_QUANTILE>);
  });
}
