// The per-row terms of the Weibull proportional-hazards likelihood that
// weibull.hip (the handle's row kernel and its shape sums) and
// weibull_predict.hip (the streaming summary) share.
//
// A row holds d in {0, 1} (1: an event) and lt = log t; eta = X~ beta and the
// shape is k > 0, with log k given beside it.  Every expression below is
// written with its association, and fp-contract is off: a product is rounded
// before the sum it enters.
//   a    = eta + (k * lt)                     the argument of the one exp
//   m    = exp(a)                             the cumulative hazard
//   full = d * ((log k + ((k - 1) * lt)) + eta) - m
//                                             the row's whole log density
//   med  = exp((log(log 2) - eta) / k)        the median survival time
// At k = 1 the product k * lt is lt itself, so a is the Poisson handle's
// eta + o bit for bit.  Where a is past exp's range m = +inf and full = -inf
// for a finite eta and lt (d times a finite number, minus inf); NaN only where
// eta itself is +inf with d = 1.
#pragma once
#include <math.h>

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr double WEIBULL_LOG_LOG2 = -0.36651292058166435;   // log(log 2)

__device__ __forceinline__ double weibull_arg(double eta, double k,
                                              double lt) {
  const double klt = k * lt;
  return eta + klt;
}

__device__ __forceinline__ double weibull_full(double eta, double d, double lt,
                                               double k, double logk) {
  const double m = exp(weibull_arg(eta, k, lt));
  const double km1lt = (k - 1.) * lt;
  return d * ((logk + km1lt) + eta) - m;
}

__device__ __forceinline__ double weibull_median(double eta, double k) {
  return exp((WEIBULL_LOG_LOG2 - eta) / k);
}

}  // namespace bbx
