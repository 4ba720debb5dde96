// Negative-binomial likelihood with a log link, an exposure offset and a
// dispersion ("size") r for the Hamiltonian coefficient samplers: its
// gradient, its Hessian-vector product at a fixed location, the trajectory /
// No-U-Turn drivers of hamiltonian.hpp with this family's block between "eta
// is complete" and "grad_loglik is complete", and the reduction the
// dispersion's own update needs.
//
// Counts y >= 0 with mean mu = exp(eta + o), eta = X~ beta, o = log(exposure),
// and variance mu + mu^2 / r.  With theta = log r and t = (eta + o) - theta,
// per row (negbin_terms.hpp):
//   ll_i    = y t - (y + r) softplus(t)   (G(y, r) - log y! is constant in
//                                          beta: dropped here)
//   w_i     = y - (y + r) sigma(t),  grad = X~^T w
//   omega_i = (y + r) (sigma(t) (1 - sigma(t)))
// Hessian-vector product at a fixed location: u = X~ v, out = X~^T (-(omega u))
// Dispersion: L(r) = sum_i G(y_i, r) + y_i t_i - (y_i + r) softplus(t_i) for
// up to NegBinDisp::MAXC values of r in one pass over the rows.
//
// No overflow: the only exp is exp(-|t|) <= 1, so ll_i, w_i and omega_i are
// finite for every finite t; there is no mu = exp(eta) as in poisson.hip.  An
// infinite eta gives ll_i = -inf (t = -inf with y > 0, t = +inf with y = 0)
// or NaN.  The test that raises CoxTraj::zero (and skip) is ll_i == -inf.
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the three expressions above on rows (y_i, o_i), with the
// handle's r and log r in the policy, and the dispersion sums as a candidate
// policy of glm_rows.hpp's glm_cand_kernel: a row's term for r_k is computed
// from (eta + o, y) and negbin_gtab(r_k) alone, so the sum for a given r
// depends neither on K nor on its place among the K values.
#include <math.h>

#include <cmath>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"
#include "negbin_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One negative-binomial likelihood on a design: rows (y_i, log exposure_i)
struct bbx_negbin : GlmCandCore {
  double r = 1., logr = 0.;
};

namespace {

// the handle's r and log r, by value in the kernel's arguments
struct NegBinRows {
  using Handle = bbx_negbin;
  static constexpr const char* name = "negbin";
  static constexpr bool raises = true;
  double r, logr;
  static NegBinRows make(const bbx_negbin* c) {
    return NegBinRows{c->r, c->logr};
  }
  __device__ double loc(double x, double y, double o) const {
    const double tt = (x + o) - logr;
    double sp, sg;
    negbin_link(tt, &sp, &sg);
    return (y + r) * (sg * (1. - sg));
  }
  __device__ bool grad(double x, double y, double o, double& w,
                       double& l) const {
    const double tt = (x + o) - logr;
    double sp, sg;
    negbin_link(tt, &sp, &sg);
    w = y - (y + r) * sg;
    l = negbin_beta_part(y, r, tt, sp);
    return l == -INFINITY;
  }
};

// The dispersion sums: G(y, r_k) + y t - (y + r_k) softplus(t), t = (eta + o)
// - log r_k, per value r_k of the caller's array
struct NegBinDisp {
  using Handle = bbx_negbin;
  using Sum = double;
  static constexpr int MAXC = 8;   // values of r per dispersion call
  static constexpr int TAB = NEGBIN_GTAB;
  static constexpr const char* family = "negbin";
  static constexpr const char* who = "bbx_negbin_dispersion_loglik: ";
  static constexpr const char* count = "n_r";
  static constexpr const char* arg = "r";
  static constexpr const char* must = "positive";
  struct Row {
    double y, a_o;
  };
  __device__ static Row row(double eta, double2 yo) {
    return Row{yo.x, eta + yo.y};
  }
  __device__ static double term(const Row& w, const double* tab) {
    const double r = tab[NEGBIN_TAB_R], logr = tab[NEGBIN_TAB_R + 1];
    const double tk = w.a_o - logr;
    double sp, sg;
    negbin_link(tk, &sp, &sg);
    return negbin_G(w.y, r, tab) + negbin_beta_part(w.y, r, tk, sp);
  }
  static size_t stride(const bbx_negbin*) { return 1; }
  static bool valid(const bbx_negbin*, const double* r) {
    return finite_positive(*r);
  }
  static void fill(const bbx_negbin*, const double* r, double* tab) {
    negbin_gtab(*r, tab);
  }
};

int negbin_create_impl(bbx_design* h, const double* y,
                       const double* log_exposure, double dispersion,
                       bbx_negbin** out) {
  BBX_TRY(glm_create_head(h, y != nullptr, out));
  if (!finite_positive(dispersion))
    return fail(BBX_ERR_INVALID, "the dispersion is not finite and positive");
  return glm_create_rows(
      h, "negbin", y, log_exposure, glm_count_row,
      [&](bbx_negbin* c) {
        c->r = dispersion;
        c->logr = log(dispersion);
        return alloc_cand<NegBinDisp>(c);
      },
      out);
}

}  // namespace

extern "C" int bbx_negbin_create(bbx_design* design, const double* y,
                                 const double* log_exposure, double dispersion,
                                 bbx_negbin** out) {
  return no_throw([&] {
    return negbin_create_impl(design, y, log_exposure, dispersion, out);
  });
}

extern "C" int bbx_negbin_set_dispersion(bbx_negbin* c, double r) {
  BBX_TRY(ham::check(c, "negbin"));
  if (!finite_positive(r))
    return fail(BBX_ERR_INVALID,
                "bbx_negbin_set_dispersion: the dispersion is not finite and "
                "positive");
  if (c->nuts_open)
    return fail(BBX_ERR_STATE,
                "bbx_negbin_set_dispersion: a No-U-Turn tree is installed on "
                "the handle (bbx_negbin_nuts_begin); take its sample "
                "(bbx_negbin_nuts_sample) first");
  c->r = r;
  c->logr = log(r);
  c->have_location = false;   // omega was formed with the previous r
  return BBX_OK;
}

extern "C" int bbx_negbin_dispersion_loglik(bbx_negbin* c, const double* beta,
                                            int n_r, const double* r,
                                            double* out) {
  return cand_loglik<NegBinDisp>(c, beta, n_r, r, out);
}

BBX_HAM_ENTRY_POINTS(negbin, GlmFamilyT<NegBinRows>)
