// Posterior prediction and pointwise predictive scores of the
// negative-binomial model from draws of the coefficients and of the
// dispersion: the streaming summary of predict.hip (predict_summary.hpp) in
// one more instantiation, in a translation unit of its own.
#include "predict_summary.hpp"

using namespace bbx;
using namespace bbx::pred;

// bbx_design_predictive_summary with mu = exp(eta +
// offset), the full log-likelihood term G(y, r_s) + y t - (y + r_s)
// softplus(t) + c, t = eta + offset - log r_s, and r_s the dispersion of draw
// s, through the same driver (predictive_summary_impl).
extern "C" int bbx_design_predictive_summary_negbin(
    bbx_design* design, int64_t n_draw, const double* coef,
    const double* dispersion, const double* offset, const double* y,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws) {
  const char* who = "bbx_design_predictive_summary_negbin: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!dispersion)
    return fail(BBX_ERR_INVALID, std::string(who) + "dispersion is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if (y && (!lpd || !ll_mean || !ll_var))
    return fail(BBX_ERR_INVALID, std::string(who) +
                                     "y is given but lpd, ll_mean or ll_var is "
                                     "NULL");
  for (int64_t d = 0; d < n_draw; ++d) {
    if (!(dispersion[d] > 0.) || !std::isfinite(dispersion[d]))
      return fail(BBX_ERR_INVALID, std::string(who) + "dispersion[" +
                                       std::to_string(d) +
                                       "] is not finite and positive");
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const PredCall q{design, PRED_NEGBIN, n_draw,  coef,     dispersion,
                     offset, y,           nullptr, ll_const, draws_per_pass,
                     mean,   sd,          lpd,     ll_mean,  ll_var,
                     mu_draws};
    return predictive_summary_impl(q, launch_summary<PRED_NEGBIN>);
  });
}
