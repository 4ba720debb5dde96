// Posterior prediction and pointwise predictive scores of the Weibull
// proportional-hazards model from draws of the coefficients and of the shape:
// the streaming summary of predict.hip (predict_summary.hpp) in one more
// instantiation, in a translation unit of its own.
#include "predict_summary.hpp"

using namespace bbx;
using namespace bbx::pred;

// bbx_design_predictive_summary with the median survival time
// exp((log(log 2) - eta) / k_s) as the predicted quantity and, with an
// outcome, the whole log density d ((log k_s + (k_s - 1) lt) + eta) -
// exp(eta + k_s lt) + c, k_s the shape of draw s, through the same driver
// (predictive_summary_impl): the shapes and their logs travel in the linear
// model's per-draw slots, log t in the row slot of the logit model's n_trial.
extern "C" int bbx_design_predictive_summary_weibull(
    bbx_design* design, int64_t n_draw, const double* coef,
    const double* shape, const double* event, const double* log_time,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws) {
  const char* who = "bbx_design_predictive_summary_weibull: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!shape) return fail(BBX_ERR_INVALID, std::string(who) + "shape is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if ((event == nullptr) != (log_time == nullptr))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "event and log_time are given together "
                                     "or not at all");
  if (event && (!lpd || !ll_mean || !ll_var))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "an outcome is given but lpd, ll_mean or "
                                     "ll_var is NULL");
  if (event && n_draw < 2)
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "scoring an outcome needs at least 2 "
                                     "draws");
  for (int64_t d = 0; d < n_draw; ++d) {
    if (!(shape[d] > 0.) || !std::isfinite(shape[d]))
      return fail(BBX_ERR_INVALID, std::string(who) + "shape[" +
                                       std::to_string(d) +
                                       "] is not finite and positive");
  }
  if (event) {
    for (int64_t i = 0; i < design->n; ++i) {
      if (!(event[i] == 0. || event[i] == 1.))
        return fail(BBX_ERR_INVALID, std::string(who) + "event[" +
                                         std::to_string(i) + "] is not 0 or 1");
      if (!std::isfinite(log_time[i]))
        return fail(BBX_ERR_INVALID, std::string(who) + "log_time[" +
                                         std::to_string(i) +
                                         "] is not finite");
    }
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const PredCall q{design, PRED_WEIBULL, n_draw,   coef,     shape,
                     nullptr, event,       log_time, ll_const, draws_per_pass,
                     mean,    sd,          lpd,      ll_mean,  ll_var,
                     mu_draws};
    return predictive_summary_impl(q, launch_summary<PRED_WEIBULL>);
  });
}
