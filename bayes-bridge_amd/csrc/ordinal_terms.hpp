// The per-row terms of the proportional-odds (cumulative logit) likelihood
// that ordinal.hip (the handle's row kernel and the cutpoint sums) and
// ordinal_predict.hip (the streaming summary) share.
//
// Categories y in {0, ..., K - 1}, cutpoints c_1 < ... < c_{K-1}, c_0 = -inf,
// c_K = +inf, P(y <= k) = sigma(c_{k+1} - (eta + o)).  With
// a = c_{y+1} - (eta + o) (upper), b = c_y - (eta + o) (lower) and
// delta_k = c_{k+1} - c_k:
//   softplus(x) = max(x, 0) + log1p(exp(-|x|))
//   sigma(x)    = 1 / (1 + e) for x >= 0, e / (1 + e) below, e = exp(-|x|)
//   g_k  = log(1 - exp(-delta_k)) for 0 < k < K - 1, else 0
//   ll   = (g_y - softplus(-a)) - softplus(b)
//   w    = sigma(b) - sigma(-a)
//   d    = sigma(a) sigma(-a) + sigma(b) sigma(-b),
//          sigma(x) sigma(-x) = e / ((1 + e) (1 + e))
// ll is log(sigma(a) - sigma(b)) in product form: sigma(a) - sigma(b) =
// sigma(a) sigma(-b) (1 - exp(-delta)).  The difference itself loses every
// digit once |eta| passes 37; no term here cancels, and the only exp is
// exp(-|x|) <= 1: for a finite eta everything is finite.
//
// A category's (lower cut, upper cut, g) come from a table of ORDINAL_TAB
// doubles per category, made on the host (ordinal_tab).  The end categories
// hold -inf / +inf there, and the row terms SELECT on them: a = +inf for
// y = K - 1 and b = -inf for y = 0 whatever eta is, so that softplus(-a),
// sigma(-a) (softplus(b), sigma(b)) and their part of d are exactly 0.
#pragma once
#include <math.h>

#include <cmath>

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr int ORDINAL_MAXCAT = 16;   // categories at most
constexpr int ORDINAL_TAB = 3;       // doubles per category: lower, upper, g
constexpr int ORDINAL_TABLE = ORDINAL_MAXCAT * ORDINAL_TAB;

// g of a gap delta > 0: log(1 - exp(-delta)) without cancellation
inline double ordinal_gap_term(double delta) {
  return delta <= M_LN2 ? log(-expm1(-delta)) : log1p(-exp(-delta));
}

// the table of one cutpoint vector (host); cuts[K - 1]
inline void ordinal_tab(int K, const double* cuts, double* tab) {
  for (int k = 0; k < K; ++k) {
    const double lo = k == 0 ? -INFINITY : cuts[k - 1];
    const double hi = k == K - 1 ? INFINITY : cuts[k];
    tab[ORDINAL_TAB * k] = lo;
    tab[ORDINAL_TAB * k + 1] = hi;
    tab[ORDINAL_TAB * k + 2] =
        (k > 0 && k < K - 1) ? ordinal_gap_term(hi - lo) : 0.;
  }
}

// finite and strictly increasing
inline bool ordinal_cuts_ok(int K, const double* cuts) {
  for (int k = 0; k < K - 1; ++k) {
    if (!std::isfinite(cuts[k])) return false;
    if (k > 0 && !(cuts[k - 1] < cuts[k])) return false;
  }
  return true;
}

#if defined(__HIPCC__)
// softplus(x), sigma(x) and sigma(x) sigma(-x) from one exp
__device__ __forceinline__ void ordinal_link(double x, double* softplus,
                                             double* sigma, double* ss) {
  const double e = exp(-fabs(x));
  const double q = 1. + e;
  *softplus = fmax(x, 0.) + log1p(e);
  *sigma = x >= 0. ? 1. / q : e / q;
  *ss = e / (q * q);
}

// x is an infinity, tested against the inline constants 0.5 and 0 (only 0 and
// the infinities are their own halves): a comparison with INFINITY holds a
// 64-bit literal in a scalar register pair per sign, and the gradient mode of
// the row kernel has none to spare
__device__ __forceinline__ bool ordinal_is_inf(double x) {
  return x * .5 == x && x != 0.;
}

// -a and b of a row: xo = eta + o; (lo, hi) the category's cuts.  The end
// categories' sentinel passes through as it is, whatever xo holds.
__device__ __forceinline__ void ordinal_ab(double xo, double lo, double hi,
                                           double* neg_a, double* b) {
  *neg_a = ordinal_is_inf(hi) ? -hi : -(hi - xo);
  *b = ordinal_is_inf(lo) ? lo : lo - xo;
}

// ll of a row alone (the cutpoint sums, the predictive scores)
__device__ __forceinline__ double ordinal_ll(double xo, double lo, double hi,
                                             double g) {
  double na, b;
  ordinal_ab(xo, lo, hi, &na, &b);
  const double ea = exp(-fabs(na)), eb = exp(-fabs(b));
  return (g - (fmax(na, 0.) + log1p(ea))) - (fmax(b, 0.) + log1p(eb));
}
#endif

}  // namespace bbx
