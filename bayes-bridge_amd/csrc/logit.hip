// Binomial-logit likelihood (model/logistic_model.py:49-74) for the
// Hamiltonian coefficient samplers: its gradient, its Hessian-vector product
// at a fixed location, and the trajectory / No-U-Turn drivers of
// hamiltonian.hpp with this family's block between "eta is complete" and
// "grad_loglik is complete".
//
// With eta = X~ beta, y = n_success, m = n_trial, per row:
//   ll_i = y eta - m logaddexp(0, eta)        (NumPy's branch form)
//   p_i  = 1 / (1 + exp(-eta)),  w_i = y - m p_i,  grad = X~^T w
// Hessian-vector product at a fixed location: d_i = m (p_i (1 - p_i)),
//   u = X~ v,  out = X~^T (-(d u))           (= -X~^T (m weight (X~ v)))
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the three expressions above on rows (y_i, m_i).  No overflow:
// every value is finite for a finite eta, and no flag is ever raised.
#include <math.h>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// npy_logaddexp(0, x): x == 0 -> log 2; x < 0 -> log1p(exp(x)); else
// x + log1p(exp(-x)); NaN -> NaN
__device__ inline double logaddexp0(double x) {
  if (x == 0.) return M_LN2;
  return x > 0. ? x + log1p(exp(-x)) : log1p(exp(x));
}

}  // namespace bbx

using namespace bbx;

// One logit likelihood on a design: rows (n_success_i, n_trial_i)
struct bbx_logit : GlmRowsCore {};

namespace {

struct LogitRows {
  using Handle = bbx_logit;
  static constexpr const char* name = "logit";
  static constexpr bool raises = false;
  static LogitRows make(const bbx_logit*) { return LogitRows{}; }
  __device__ double loc(double x, double, double m) const {
    const double p = 1. / (1. + exp(-x));
    return m * (p * (1. - p));
  }
  __device__ bool grad(double x, double y, double m, double& w,
                       double& l) const {
    const double p = 1. / (1. + exp(-x));
    w = y - m * p;
    l = y * x - m * logaddexp0(x);
    return false;
  }
};

int logit_row(int64_t i, double y, double m) {
  if (!std::isfinite(y) || !std::isfinite(m))
    return fail(BBX_ERR_INVALID,
                "row " + std::to_string(i) + ": a count is not finite");
  if (y < 0.)
    return fail(BBX_ERR_INVALID,
                "n_success[" + std::to_string(i) + "] is negative");
  if (m <= 0.)
    return fail(BBX_ERR_INVALID,
                "n_trial[" + std::to_string(i) + "] is not positive");
  if (y > m)
    return fail(BBX_ERR_INVALID, "n_success[" + std::to_string(i) +
                                     "] exceeds n_trial");
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_logit_create(bbx_design* design, const double* n_success,
                                const double* n_trial, bbx_logit** out) {
  return no_throw([&] {
    BBX_TRY(glm_create_head(design, n_success && n_trial, out));
    return glm_create_rows(design, "logit", n_success, n_trial, logit_row,
                           out);
  });
}

BBX_HAM_ENTRY_POINTS(logit, GlmFamilyT<LogitRows>)
