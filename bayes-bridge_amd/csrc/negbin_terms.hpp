// The per-row terms of the negative-binomial likelihood that negbin.hip (the
// handle's row kernel) and predict.hip (the streaming summary) share.
//
// With t = eta + o - log r:
//   softplus(t) = max(t, 0) + log1p(exp(-|t|))
//   sigma(t)    = 1 / (1 + exp(-|t|)) for t >= 0, exp(-|t|) / (1 + exp(-|t|))
//                 below: no exp of a positive argument, nothing overflows
//   G(y, r)     = sum_{j < y} log(r + j) = lgamma(y + r) - lgamma(r)
// G comes from a table of NEGBIN_GTAB doubles per value of r, made on the host
// (negbin_gtab).  tab[j] = sum_{i < j} log(r + i) for j <= NEGBIN_GSUM is the
// sum of logs itself: a count up to NEGBIN_GSUM -- most counts -- is one load.
// Above it, with b = r + NEGBIN_GSUM, d = y - NEGBIN_GSUM, a = b + d and
// Stirling's lgamma(x) = (x - 1/2) log x - x + log(2 pi) / 2 + s(x),
//   G = tab[NEGBIN_GSUM] + lgamma(a) - lgamma(b)
//     = tab[NEGBIN_GSUM] + (a - 1/2) log1p(d / b) + d (log b - 1) + s(a) - s(b)
// with log b - 1 and s(b) from the table: one log1p and a short polynomial
// on the device.  The difference of the two lgammas is never formed from
// their values (each is r log r in size, and the difference is lost to
// rounding from r = 1e8 on); every term here is of the size of y log r.  a
// and b are at least NEGBIN_GSUM = 8, where s(x) through x^-11 is within
// 2e-14 of the exact remainder.
#pragma once
#include <math.h>

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr int NEGBIN_GSUM = 8;                 // counts up to it: a table entry
constexpr int NEGBIN_GTAB = NEGBIN_GSUM + 5;   // doubles per value of r
constexpr int NEGBIN_TAB_LOGB = NEGBIN_GSUM + 1;   // log(r + NEGBIN_GSUM) - 1
constexpr int NEGBIN_TAB_SB = NEGBIN_GSUM + 2;     // s(r + NEGBIN_GSUM)
constexpr int NEGBIN_TAB_R = NEGBIN_GSUM + 3;      // r; log r follows

// the remainder of Stirling's series for lgamma(x), x >= NEGBIN_GSUM
__host__ __device__ inline double negbin_stirling_rest(double x) {
  const double i = 1. / x, i2 = i * i;
  double s = -691. / 360360.;
  s = s * i2 + 1. / 1188.;
  s = s * i2 - 1. / 1680.;
  s = s * i2 + 1. / 1260.;
  s = s * i2 - 1. / 360.;
  s = s * i2 + 1. / 12.;
  return s * i;
}

// the table of one r (host)
inline void negbin_gtab(double r, double* tab) {
  double g = 0.;
  for (int j = 0; j <= NEGBIN_GSUM; ++j) {
    tab[j] = g;
    g += log(r + (double)j);
  }
  const double b = r + (double)NEGBIN_GSUM;
  tab[NEGBIN_TAB_LOGB] = log(b) - 1.;
  tab[NEGBIN_TAB_SB] = negbin_stirling_rest(b);
  tab[NEGBIN_TAB_R] = r;
  tab[NEGBIN_TAB_R + 1] = log(r);
}

// exp(-|t|), softplus(t) and sigma(t) from one exp
__device__ __forceinline__ void negbin_link(double t, double* softplus,
                                            double* sigma) {
  const double e = exp(-fabs(t));
  *softplus = fmax(t, 0.) + log1p(e);
  *sigma = t >= 0. ? 1. / (1. + e) : e / (1. + e);
}

// `tab`: the NEGBIN_GTAB entries of this r
__device__ __forceinline__ double negbin_G(double y, double r,
                                           const double* __restrict__ tab) {
  if (y > (double)NEGBIN_GSUM) {
    const double b = r + (double)NEGBIN_GSUM, d = y - (double)NEGBIN_GSUM;
    const double a = b + d;
    return tab[NEGBIN_GSUM] +
           ((a - .5) * log1p(d / b) + d * tab[NEGBIN_TAB_LOGB]) +
           (negbin_stirling_rest(a) - tab[NEGBIN_TAB_SB]);
  }
  // (a count that is no count -- negative, NaN -- reads entry 0, not memory
  // before the table)
  return tab[y >= 0. ? (int)y : 0];
}

// y t - (y + r) softplus(t): the part of a row's log-likelihood that depends
// on the coefficients.  Finite for every finite t.
__device__ __forceinline__ double negbin_beta_part(double y, double r, double t,
                                                   double softplus) {
  return y * t - (y + r) * softplus;
}

}  // namespace bbx
