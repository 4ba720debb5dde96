// Weibull proportional-hazards likelihood of right-censored times for the
// Hamiltonian coefficient samplers: its gradient, its Hessian-vector product
// at a fixed location, the trajectory / No-U-Turn drivers of hamiltonian.hpp
// with this family's block between "eta is complete" and "grad_loglik is
// complete", and the reduction the shape's own update needs.
//
// Rows (d_i, lt_i): d = 1 for an event at t, 0 for a row censored at t, and
// lt = log t.  With eta = X~ beta and the shape k > 0 the hazard is
// h(t | x) = k t^(k - 1) exp(eta), and per row, with every product rounded
// before the sum it enters (fp-contract off):
//   m_i  = exp(eta_i + (k * lt_i))
//   ll_i = (d_i * eta_i) - m_i     (d (log k + (k - 1) lt) is constant in
//                                   beta: dropped here)
//   w_i  = d_i - m_i,  grad = X~^T w
// Hessian-vector product at a fixed location: the location's value is m_i,
// u = X~ v, out = X~^T (-(m u)).
// Shape: L(k) = sum_i (d_i * ((log k + ((k - 1) * lt_i)) + eta_i)) - m_i, the
// whole log density, for up to WeibullShape::MAXC values of k in one pass over
// the rows (weibull_terms.hpp states the term).
//
// At k = 1 the product k * lt is lt, so m, ll, w and the location are the
// Poisson handle's on rows (y = d, o = lt), bit for bit.
//
// Overflow, as in poisson.hip: where eta + k lt is past exp's range, m = inf
// and ll_i = -inf (NaN where eta itself is +inf and d = 1).  The test that
// raises CoxTraj::zero (and skip) is m == inf, not ll_i == -inf.  In the shape
// sums such a row's term is d times a finite number minus inf = -inf, and the
// sum for that k is exactly -inf for finite eta: no inf - inf is formed.
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the expressions above on rows (d_i, lt_i), with the handle's k
// in the policy, and the shape sums as a candidate policy of glm_rows.hpp's
// glm_cand_kernel: a row's term for k_j is computed from (eta, d, lt) and the
// pair (k_j, log k_j) alone, so the sum for a given k depends neither on K nor
// on its place among the K values.
#include <math.h>

#include <cmath>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"
#include "weibull_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One Weibull likelihood on a design: rows (d_i, log t_i)
struct bbx_weibull : GlmCandCore {
  double k = 1., logk = 0.;
};

namespace {

// the handle's k and log k, by value in the kernel's arguments (the
// beta-dependent part reads k alone: log k belongs to the whole density)
struct WeibullRows {
  using Handle = bbx_weibull;
  static constexpr const char* name = "weibull";
  static constexpr bool raises = true;
  double k, logk;
  static WeibullRows make(const bbx_weibull* c) {
    return WeibullRows{c->k, c->logk};
  }
  __device__ double loc(double x, double, double lt) const {
    return exp(weibull_arg(x, k, lt));
  }
  __device__ bool grad(double x, double d, double lt, double& w,
                       double& l) const {
    const double m = exp(weibull_arg(x, k, lt));
    w = d - m;
    l = d * x - m;
    return m == INFINITY;
  }
};

// The shape sums: the whole log density (weibull_terms.hpp) per value k_j of
// the caller's array.  The NPART partials are re-added in long double and
// rounded once: partials of one size added in double one after the other lose
// several ulps, which the slice sampler would not notice but the tests' bound
// (4 float64 roundings) does.
struct WeibullShape {
  using Handle = bbx_weibull;
  using Sum = long double;
  static constexpr int MAXC = 8;   // values of k per shape call
  static constexpr int TAB = 2;    // (k, log k)
  static constexpr const char* family = "weibull";
  static constexpr const char* who = "bbx_weibull_shape_loglik: ";
  static constexpr const char* count = "n_k";
  static constexpr const char* arg = "k";
  static constexpr const char* must = "positive";
  struct Row {
    double eta, d, lt;
  };
  __device__ static Row row(double eta, double2 dlt) {
    return Row{eta, dlt.x, dlt.y};
  }
  __device__ static double term(const Row& w, const double* tab) {
    return weibull_full(w.eta, w.d, w.lt, tab[0], tab[1]);
  }
  static size_t stride(const bbx_weibull*) { return 1; }
  static bool valid(const bbx_weibull*, const double* k) {
    return finite_positive(*k);
  }
  static void fill(const bbx_weibull*, const double* k, double* tab) {
    tab[0] = *k;
    tab[1] = log(*k);
  }
};

int weibull_row(int64_t i, double di, double lti) {
  if (!(di == 0. || di == 1.))
    return fail(BBX_ERR_INVALID,
                "event[" + std::to_string(i) + "] is not 0 or 1");
  if (!std::isfinite(lti))
    return fail(BBX_ERR_INVALID,
                "log_time[" + std::to_string(i) + "] is not finite");
  return BBX_OK;
}

int weibull_create_impl(bbx_design* h, const double* event,
                        const double* log_time, double shape,
                        bbx_weibull** out) {
  BBX_TRY(glm_create_head(h, true, out));
  if (!event) return fail(BBX_ERR_INVALID, "NULL event array");
  if (!log_time) return fail(BBX_ERR_INVALID, "NULL log_time array");
  if (!finite_positive(shape))
    return fail(BBX_ERR_INVALID, "the shape is not finite and positive");
  return glm_create_rows(
      h, "weibull", event, log_time, weibull_row,
      [&](bbx_weibull* c) {
        c->k = shape;
        c->logk = log(shape);
        return alloc_cand<WeibullShape>(c);
      },
      out);
}

}  // namespace

extern "C" int bbx_weibull_create(bbx_design* design, const double* event,
                                  const double* log_time, double shape,
                                  bbx_weibull** out) {
  return no_throw([&] {
    return weibull_create_impl(design, event, log_time, shape, out);
  });
}

extern "C" int bbx_weibull_set_shape(bbx_weibull* c, double k) {
  BBX_TRY(ham::check(c, "weibull"));
  if (!finite_positive(k))
    return fail(BBX_ERR_INVALID,
                "bbx_weibull_set_shape: the shape is not finite and positive");
  if (c->nuts_open)
    return fail(BBX_ERR_STATE,
                "bbx_weibull_set_shape: a No-U-Turn tree is installed on the "
                "handle (bbx_weibull_nuts_begin); take its sample "
                "(bbx_weibull_nuts_sample) first");
  c->k = k;
  c->logk = log(k);
  c->have_location = false;   // m was formed with the previous k
  return BBX_OK;
}

extern "C" int bbx_weibull_shape_loglik(bbx_weibull* c, const double* beta,
                                        int n_k, const double* k,
                                        double* out) {
  return cand_loglik<WeibullShape>(c, beta, n_k, k, out);
}

BBX_HAM_ENTRY_POINTS(weibull, GlmFamilyT<WeibullRows>)
