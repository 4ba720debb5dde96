// Posterior prediction and pointwise predictive scores of the linear, logit
// and Poisson models from draws of the coefficients
// (bbx_design_predictive_summary, include/bbx.h), and of the negative-binomial
// model from draws of the coefficients and of the dispersion
// (bbx_design_predictive_summary_negbin, negbin_predict.hip: one more
// instantiation of the same kernel, predict_summary.hpp, under a family code
// that is no BBX_PRED_* of the header).  The ordinal model's kernel
// (ordinal_predict.hip) follows the same method with K means per row.
//
// Per draw s the linear predictor eta_s = X~ beta_s is formed on the device by
// the launches of bbx_design_dot (launch_prep_v + launch_dot, as ham::eta_of),
// so a draw's eta has that call's bits.  The draws go through in passes of K
// (PredPasses): K products into a K x n buffer, then ONE summary kernel that
// walks the K etas of every row in draw order and pushes
//
//   mu_s  = eta | 1 / (1 + exp(-eta)) | exp(eta)     (eta = X~ beta_s + offset)
//           (negative binomial: exp(eta), as the Poisson model)
//   ll_s  = the row's log-likelihood term of draw s (see pred_terms)
//
// into the row's Moments and Scores, whose recurrences and rules for
// non-finite draws predict_summary.hpp states: one push per draw whatever K
// is, so the results do not depend on K.  The state (six doubles per row,
// SoA) lives in HBM between passes and in registers within one; the first
// pass starts it in registers and the last one writes the five results
// instead.  Rows along the lanes, one row per thread: eta, the state and the
// optional mu draws (draw-major) are read and written 64 consecutive doubles
// per wave.  No atomics, no reduction across rows: the same inputs give the
// same bits.
//
// Per-draw traffic: 8 B per row for eta plus (48 B read + 48 B written) / K
// for the state; K = 16 makes the state's share 6 B.  K x n x 8 B (twice that
// with mu_draws) stays within PRED_BUDGET, but K never goes below 1.
#include "predict_summary.hpp"

using namespace bbx;
using namespace bbx::pred;

extern "C" int bbx_design_predictive_summary(
    bbx_design* design, int family, int64_t n_draw, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const double* n_trial, const double* ll_const, int draws_per_pass,
    double* mean, double* sd, double* lpd, double* ll_mean, double* ll_var,
    double* mu_draws) {
  const char* who = "bbx_design_predictive_summary: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (family < BBX_PRED_LINEAR || family > BBX_PRED_POISSON)
    return fail(BBX_ERR_INVALID, std::string(who) + "family " +
                                     std::to_string(family) +
                                     " is not 0 (linear), 1 (logit) or 2 "
                                     "(Poisson)");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if (y && !lpd)
    return fail(BBX_ERR_INVALID, std::string(who) + "y is given but lpd is NULL");
  if (y && !ll_mean)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "y is given but ll_mean is NULL");
  if (y && !ll_var)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "y is given but ll_var is NULL");
  if (family == BBX_PRED_LINEAR && !obs_prec)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the linear model needs obs_prec");
  if (family != BBX_PRED_LINEAR && obs_prec)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "obs_prec is an argument of the linear "
                                   "model only");
  if (obs_prec) {
    for (int64_t d = 0; d < n_draw; ++d) {
      if (!(obs_prec[d] > 0.) || !std::isfinite(obs_prec[d]))
        return fail(BBX_ERR_INVALID, std::string(who) + "obs_prec[" +
                                         std::to_string(d) +
                                         "] is not finite and positive");
    }
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const PredCall q{design, family,  n_draw,  coef,   obs_prec,
                     offset, y,       n_trial, ll_const, draws_per_pass,
                     mean,   sd,      lpd,     ll_mean, ll_var,
                     mu_draws};
    return predictive_summary_impl(
        q, family == BBX_PRED_LINEAR  ? launch_summary<BBX_PRED_LINEAR>
           : family == BBX_PRED_LOGIT ? launch_summary<BBX_PRED_LOGIT>
                                      : launch_summary<BBX_PRED_POISSON>);
  });
}
