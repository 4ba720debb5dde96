// Proportional-odds (cumulative logit) likelihood of an ordered outcome with
// an optional per-row offset and K - 1 cutpoints for the Hamiltonian
// coefficient samplers: its gradient, its Hessian-vector product at a fixed
// location, the trajectory / No-U-Turn drivers of hamiltonian.hpp with this
// family's block between "eta is complete" and "grad_loglik is complete", and
// the reduction the cutpoints' own update needs.
//
// Categories y in {0, ..., K - 1}, 2 <= K <= ORDINAL_MAXCAT, cutpoints
// c_1 < ... < c_{K-1}, c_0 = -inf, c_K = +inf, and
// P(y_i <= k) = sigma(c_{k+1} - (eta_i + o_i)), eta = X~ beta.  There is no
// intercept: the cutpoints are the intercepts.  With a = c_{y+1} - (eta + o),
// b = c_y - (eta + o) and delta_k = c_{k+1} - c_k, per row
// (ordinal_terms.hpp):
//   ll_i = (g_y - softplus(-a)) - softplus(b),
//          g_k = log(1 - exp(-delta_k)) for 0 < k < K - 1, else 0
//   w_i  = sigma(b) - sigma(-a),                   grad = X~^T w
//   d_i  = sigma(a) sigma(-a) + sigma(b) sigma(-b)
// Hessian-vector product at a fixed location: u = X~ v, out = X~^T (-(d u))
// Cutpoints: L(c) = sum_i ll_i for up to OrdinalCuts::MAXC whole cutpoint vectors
// in one pass over the rows.
//
// ll_i is the whole log-probability of the row: g_y depends on the cutpoints
// and is kept everywhere.  No overflow: the only exp is exp(-|x|) <= 1, so
// ll_i, w_i and d_i are finite for every finite eta.  An infinite eta gives
// ll_i = -inf where the category's probability is 0; the test that raises
// CoxTraj::zero (and skip) is ll_i == -inf.  THE END CATEGORY ON THE SIDE OF
// AN INFINITE ETA (y = K - 1 at eta = +inf, y = 0 at eta = -inf) gives
// ll_i = 0, w_i = 0, d_i = 0, the limits: the end categories' absent term is
// a select on the table's +-inf sentinel, not inf - inf.  Every other NaN
// stays a NaN (a NaN eta, +inf - inf in the offset sum).
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the three expressions above on rows (y_i, o_i), with a pointer
// to the handle's table of (lower cut, upper cut, g) per category in the
// policy, and the cutpoint sums as a candidate policy of glm_rows.hpp's
// glm_cand_kernel: a row's term for candidate k is computed from (eta + o, y)
// and ordinal_tab of candidate k alone, so the sum of a given cutpoint vector
// depends neither on the number of candidates nor on its place among them.
#include <math.h>

#include <cmath>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"
#include "ordinal_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One proportional-odds likelihood on a design: rows (y_i, offset_i)
struct bbx_ordinal : GlmCandCore {
  DevMem tab;   // ORDINAL_TABLE: ordinal_tab of the handle's cutpoints
  int K = 0;
};

namespace {

// the handle's table, by pointer in the kernel's arguments
struct OrdinalRows {
  using Handle = bbx_ordinal;
  static constexpr const char* name = "ordinal";
  static constexpr bool raises = true;
  const double* tab;
  static OrdinalRows make(const bbx_ordinal* c) {
    return OrdinalRows{c->tab.as<const double>()};
  }
  __device__ double loc(double x, double y, double o) const {
    const double* t = tab + ORDINAL_TAB * (int)y;
    double na, b, sp, sg, ssa, ssb;
    ordinal_ab(x + o, t[0], t[1], &na, &b);
    ordinal_link(na, &sp, &sg, &ssa);
    ordinal_link(b, &sp, &sg, &ssb);
    return ssa + ssb;
  }
  __device__ bool grad(double x, double y, double o, double& w,
                       double& l) const {
    const double* t = tab + ORDINAL_TAB * (int)y;
    double na, b, spa, sga, spb, sgb, ss;
    ordinal_ab(x + o, t[0], t[1], &na, &b);
    ordinal_link(na, &spa, &sga, &ss);
    ordinal_link(b, &spb, &sgb, &ss);
    w = sgb - sga;
    l = (t[2] - spa) - spb;
    // (l == -INFINITY without the literal: see ordinal_is_inf)
    return ordinal_is_inf(l) && l < 0.;
  }
};

// The cutpoint sums: ll_i per whole cutpoint vector (K - 1 numbers) of the
// caller's array.  y is a valid category (checked at create): the table index
// is in range.
struct OrdinalCuts {
  using Handle = bbx_ordinal;
  using Sum = double;
  static constexpr int MAXC = 8;   // cutpoint vectors per call
  static constexpr int TAB = ORDINAL_TABLE;
  static constexpr const char* family = "ordinal";
  static constexpr const char* who = "bbx_ordinal_cutpoint_loglik: ";
  static constexpr const char* count = "n_c";
  static constexpr const char* arg = "cuts";
  static constexpr const char* must = "strictly increasing";
  struct Row {
    double xo;
    int cat;   // the category's place in a table
  };
  __device__ static Row row(double eta, double2 yo) {
    return Row{eta + yo.y, ORDINAL_TAB * (int)yo.x};
  }
  __device__ static double term(const Row& w, const double* tab) {
    const double* t = tab + w.cat;
    return ordinal_ll(w.xo, t[0], t[1], t[2]);
  }
  static size_t stride(const bbx_ordinal* c) { return c->K - 1; }
  static bool valid(const bbx_ordinal* c, const double* cuts) {
    return ordinal_cuts_ok(c->K, cuts);
  }
  static void fill(const bbx_ordinal* c, const double* cuts, double* tab) {
    ordinal_tab(c->K, cuts, tab);
  }
};

// the handle's table from K - 1 cutpoints, up in stream order; the host's
// copy is free when this returns
int upload_table(bbx_ordinal* c, const double* cuts) {
  double tab[ORDINAL_TABLE] = {};
  ordinal_tab(c->K, cuts, tab);
  BBX_HIP(hipMemcpyAsync(c->tab.ptr, tab, sizeof(tab), hipMemcpyHostToDevice,
                         c->h->stream));
  BBX_HIP(hipStreamSynchronize(c->h->stream));
  return BBX_OK;
}

int ordinal_create_impl(bbx_design* h, const double* y, const double* offset,
                        int K, const double* cuts, bbx_ordinal** out) {
  BBX_TRY(glm_create_head(h, y != nullptr, out));
  if (K < 2 || K > ORDINAL_MAXCAT)
    return fail(BBX_ERR_INVALID, "n_category outside [2, " +
                                     std::to_string(ORDINAL_MAXCAT) + "]");
  if (!cuts) return fail(BBX_ERR_INVALID, "NULL cutpoints");
  if (!ordinal_cuts_ok(K, cuts))
    return fail(BBX_ERR_INVALID,
                "the cutpoints are not finite and strictly increasing");
  BBX_TRY(glm_create_rows(
      h, "ordinal", y, offset,
      [&](int64_t i, double yi, double oi) {
        if (!(yi >= 0. && yi <= (double)(K - 1)) || yi != floor(yi))
          return fail(BBX_ERR_INVALID,
                      "y[" + std::to_string(i) + "] is not a category in [0, " +
                          std::to_string(K - 1) + "]");
        if (!std::isfinite(oi))
          return fail(BBX_ERR_INVALID,
                      "offset[" + std::to_string(i) + "] is not finite");
        return (int)BBX_OK;
      },
      [&](bbx_ordinal* c) {
        c->K = K;
        BBX_TRY(c->tab.alloc(sizeof(double) * ORDINAL_TABLE));
        return alloc_cand<OrdinalCuts>(c);
      },
      out));
  const int st = upload_table(*out, cuts);
  if (st != BBX_OK) {
    bbx_ordinal* c = *out;
    *out = nullptr;
    return ham::discard(c, st);
  }
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_ordinal_create(bbx_design* design, const double* y,
                                  const double* offset, int n_category,
                                  const double* cutpoints, bbx_ordinal** out) {
  return no_throw([&] {
    return ordinal_create_impl(design, y, offset, n_category, cutpoints, out);
  });
}

extern "C" int bbx_ordinal_set_cutpoints(bbx_ordinal* c,
                                         const double* cutpoints) {
  BBX_TRY(ham::check(c, "ordinal"));
  if (!cutpoints)
    return fail(BBX_ERR_INVALID, "bbx_ordinal_set_cutpoints: NULL cutpoints");
  if (!ordinal_cuts_ok(c->K, cutpoints))
    return fail(BBX_ERR_INVALID,
                "bbx_ordinal_set_cutpoints: the cutpoints are not finite and "
                "strictly increasing");
  if (c->nuts_open)
    return fail(BBX_ERR_STATE,
                "bbx_ordinal_set_cutpoints: a No-U-Turn tree is installed on "
                "the handle (bbx_ordinal_nuts_begin); take its sample "
                "(bbx_ordinal_nuts_sample) first");
  BBX_HIP(hipSetDevice(c->device));
  c->have_location = false;   // d was formed with the previous cutpoints
  return no_throw([&] { return upload_table(c, cutpoints); });
}

extern "C" int bbx_ordinal_cutpoint_loglik(bbx_ordinal* c, const double* beta,
                                           int n_c, const double* cuts,
                                           double* out) {
  return cand_loglik<OrdinalCuts>(c, beta, n_c, cuts, out);
}

BBX_HAM_ENTRY_POINTS(ordinal, GlmFamilyT<OrdinalRows>)
