// Posterior prediction and pointwise predictive scores of the probit model
// from draws of the coefficients: the streaming summary of predict.hip
// (predict_summary.hpp) in one more instantiation, in a translation unit of
// its own.
#include "predict_summary.hpp"

using namespace bbx;
using namespace bbx::pred;

// bbx_design_predictive_summary with Phi(eta) as the predicted quantity and,
// with an outcome, ll = log Phi(eta) (y = 1) or log Phi(-eta) (y = 0) + c,
// through the same driver (predictive_summary_impl).
extern "C" int bbx_design_predictive_summary_probit(
    bbx_design* design, int64_t n_draw, const double* coef,
    const double* offset, const double* y, const double* ll_const,
    int draws_per_pass, double* mean, double* sd, double* lpd, double* ll_mean,
    double* ll_var, double* mu_draws) {
  const char* who = "bbx_design_predictive_summary_probit: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if (y && (!lpd || !ll_mean || !ll_var))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "an outcome is given but lpd, ll_mean or "
                                     "ll_var is NULL");
  if (y && n_draw < 2)
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "scoring an outcome needs at least 2 "
                                     "draws");
  if (y) {
    for (int64_t i = 0; i < design->n; ++i)
      if (!(y[i] == 0. || y[i] == 1.))
        return fail(BBX_ERR_INVALID, std::string(who) + "y[" +
                                         std::to_string(i) + "] is not 0 or 1");
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const PredCall q{design, PRED_PROBIT, n_draw,  coef,     nullptr,
                     offset, y,           nullptr, ll_const, draws_per_pass,
                     mean,   sd,          lpd,     ll_mean,  ll_var,
                     mu_draws};
    return predictive_summary_impl(q, launch_summary<PRED_PROBIT>);
  });
}
