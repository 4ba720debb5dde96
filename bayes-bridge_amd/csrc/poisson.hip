// Poisson (incidence-rate) likelihood with a log link and an exposure offset
// for the Hamiltonian coefficient samplers: its gradient, its Hessian-vector
// product at a fixed location, and the trajectory / No-U-Turn drivers of
// hamiltonian.hpp with this family's block between "eta is complete" and
// "grad_loglik is complete".
//
// With eta = X~ beta, count y >= 0 and offset o = log(exposure), per row:
//   mu_i = exp(eta_i + o_i)
//   ll_i = y eta - mu          (sum y o - log y! is constant in beta: dropped)
//   w_i  = y - mu,  grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v, out = X~^T (-(mu u))
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the three expressions above on rows (y_i, o_i).
//
// Overflow: where eta + o is past exp's range, mu = inf and ll_i = -inf (NaN
// where eta itself is +inf and y > 0).  The test that raises CoxTraj::zero
// (and skip) is therefore mu == inf, not ll_i == -inf.
#include <math.h>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One Poisson likelihood on a design: rows (y_i, log exposure_i)
struct bbx_poisson : GlmRowsCore {};

namespace {

struct PoissonRows {
  using Handle = bbx_poisson;
  static constexpr const char* name = "poisson";
  static constexpr bool raises = true;
  static PoissonRows make(const bbx_poisson*) { return PoissonRows{}; }
  __device__ double loc(double x, double, double o) const {
    return exp(x + o);
  }
  __device__ bool grad(double x, double y, double o, double& w,
                       double& l) const {
    const double m = exp(x + o);
    w = y - m;
    l = y * x - m;
    return m == INFINITY;
  }
};

}  // namespace

extern "C" int bbx_poisson_create(bbx_design* design, const double* y,
                                  const double* log_exposure,
                                  bbx_poisson** out) {
  return no_throw([&] {
    BBX_TRY(glm_create_head(design, y != nullptr, out));
    return glm_create_rows(design, "poisson", y, log_exposure, glm_count_row,
                           out);
  });
}

BBX_HAM_ENTRY_POINTS(poisson, GlmFamilyT<PoissonRows>)
