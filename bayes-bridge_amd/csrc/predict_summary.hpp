// What the streaming summaries of posterior prediction share: the per-row
// accumulators (Moments, Scores) and the host driver of the passes
// (PredPasses), which ordinal_predict.hip's own kernel uses too, and the
// summary kernel of the one-mean families with its host side (predict.hip:
// linear, logit, Poisson; negbin_predict.hip: negative binomial;
// weibull_predict.hip: Weibull; probit_predict.hip: probit;
// student_t_predict.hip: Student-t; censored_predict.hip: censored normal;
// quantile_predict.hip: quantile).
// Kernels and
// drivers are static: a translation unit holds the instantiations it launches
// and no others.  predict.hip describes the method.
//
// THE ACCUMULATORS' CONTRACT.  A thread owns a row and pushes its draws in
// draw order, k = 1, 2, ... the 1-based index over ALL draws; between two
// passes the state lives in a state-major array ([state][n]: coalesced), and
// a store followed by a load is the identity.  So a result is a function of
// the row's draws alone: it does not depend on the pass size.
//   Moments (mean, M2), Welford:
//     delta = x - mean;  mean += delta / k;  M2 += delta * (x - mean)
//     Once a draw has overflowed (a Poisson mu of +inf, its ll of -inf) the
//     mean is that infinity and stays it, as the plain sum would: inf - inf in
//     the update would turn it into a NaN.  A NaN draw or the opposite infinity
//     still gives a NaN.  (M2 is a NaN from there on: the spread of infinite
//     values has no value.)  Results: mean, sd = sqrt(M2 / S)
//   Scores: the Moments of ll and the online log-sum-exp (max, sum):
//     ll > max ? (sum = sum * exp(max - ll) + 1, max = ll)
//              : (sum += exp(ll - max)), but a draw of -inf adds exactly 0
//     (all draws -inf: lpd = -inf, not a NaN);  a NaN draw makes the sum a NaN
//     results: lpd = max + log(sum) - log(S), mean of ll, M2 / (S - 1)
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>

#include <string>
#include <vector>

#include "common.hpp"
#include "negbin_terms.hpp"
#include "samplers.hpp"   // log_norm_cdf
#include "weibull_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {
namespace pred {

constexpr int PRED_BLOCK = 256;
constexpr int PRED_DRAWS = 16;                    // default draws per pass
constexpr size_t PRED_BUDGET = size_t(256) << 20; // eta (+ mu draws) of a pass
constexpr int PRED_STATE = 6;  // Moments of mu, then Scores
// The negative-binomial model's code.  Not a BBX_PRED_* of include/bbx.h:
// bbx_design_predictive_summary refuses it, the family has its own entry point
// and its instantiation lives in negbin_predict.hip.
constexpr int PRED_NEGBIN = 3;
// The Weibull model's, likewise: its entry point and its instantiation live in
// weibull_predict.hip.  Its "mean" is the median survival time.
constexpr int PRED_WEIBULL = 4;
// The probit model's, likewise (probit_predict.hip): mu = Phi(eta),
// ll = log Phi(+-eta).
constexpr int PRED_PROBIT = 5;
// The Student-t regression model's, likewise (student_t_predict.hip): mu = eta,
// ll = the full t-density at the draw's tau and the model's df.
constexpr int PRED_STUDENT_T = 6;
// The censored-outcome model's, likewise (censored_predict.hip): mu = eta, ll =
// the full normal density on an observed row, log Phi of the censored side's
// tail on a censored one.
constexpr int PRED_CENSORED = 7;
// The same with mu = exp(eta): the median time of the log-normal AFT model,
// whose latent scale is log t.
constexpr int PRED_LOGNORMAL = 8;
// The quantile model's, likewise (quantile_predict.hip): mu = eta, the
// conditional q-quantile; ll = the asymmetric-Laplace density at the draw's tau
// and the model's level q.
constexpr int PRED_QUANTILE = 9;
constexpr bool pred_censored(int family) {
  return family == PRED_CENSORED || family == PRED_LOGNORMAL;
}

struct PredArgs {
  int64_t n;
  int64_t k0;       // draws folded into the state before this pass
  int kn;           // draws of this pass
  int64_t n_draw;   // all draws: the last pass writes the results
  const double* eta;      // [kn][n]
  const double* tau;      // [n_draw] linear, Student-t, censored, quantile:
                          // obs_prec;
                          // Weibull: the shape k
  const double* hlt;      // [n_draw] linear: 0.5 log(obs_prec); Weibull: log k;
                          // Student-t: the draw's normalising constant;
                          // censored: 0.5 log(obs_prec / (2 pi)); quantile:
                          // log(obs_prec) + log(q (1 - q))
  const double* gtab;     // [n_draw][NEGBIN_GTAB] negbin: negbin_gtab(r);
                          // Student-t: [2] = (df + 1) / 2, df; quantile:
                          // [1] = q
  const double* offset;   // [n] or null
  const double* y;        // [n]   (SCORE)
  const double* m;        // [n] or null (logit, SCORE); Weibull: log t (SCORE);
                          // censored: the row status 0, 1, 2 (SCORE)
  const double* c;        // [n] or null (SCORE)
  double* state;          // [PRED_STATE][n]
  double* out;            // [5][n]: mean, sd, lpd, ll_mean, ll_var
  double* mu_draws;       // [kn][n] or null
};

// sigma(x) = 1 / (1 + exp(-x)) from e = exp(-|x|) <= 1: nothing overflows,
// absolute error ~1e-16
__device__ __forceinline__ double pred_sigma(double x) {
  const double e = exp(-fabs(x));
  return x >= 0. ? 1. / (1. + e) : e / (1. + e);
}

// mu and (SCORE) ll of one draw of one row; eta holds the row's offset
template <int FAMILY, bool SCORE>
__device__ __forceinline__ void pred_terms(double eta, double y, double m,
                                           double c, bool has_c, double tau,
                                           double hlt, const double* gtab,
                                           double* mu, double* ll) {
  if (FAMILY == BBX_PRED_LINEAR) {
    *mu = eta;
    if (SCORE) {
      const double r = y - eta;
      *ll = hlt - 0.5 * tau * r * r;
    }
  } else if (FAMILY == BBX_PRED_LOGIT) {
    *mu = pred_sigma(eta);
    if (SCORE) {
      const double sp = fmax(eta, 0.) + log1p(exp(-fabs(eta)));
      *ll = y * eta - m * sp;
    }
  } else if (FAMILY == BBX_PRED_POISSON) {
    *mu = exp(eta);
    if (SCORE) *ll = y * eta - *mu;
  } else if (FAMILY == PRED_WEIBULL) {
    // Weibull: y is the event indicator, m is log t, tau and hlt are the
    // draw's k and log k; the predicted quantity is the median survival time
    *mu = weibull_median(eta, tau);
    if (SCORE) *ll = weibull_full(eta, y, m, tau, hlt);
  } else if (FAMILY == PRED_STUDENT_T) {
    // hlt = lgamma((df+1)/2) - lgamma(df/2) + 1/2 log(tau / (df pi))
    *mu = eta;
    if (SCORE) {
      const double r = y - eta;
      *ll = hlt - gtab[0] * log1p(tau * (r * r) / gtab[1]);
    }
  } else if (FAMILY == PRED_QUANTILE) {
    // hlt = log tau + log(q (1 - q)); rho_q(r) = r (q - 1[r < 0])
    *mu = eta;
    if (SCORE) {
      const double r = y - eta;
      const double q = gtab[0];
      *ll = hlt - tau * (r * (r < 0. ? q - 1. : q));
    }
  } else if (pred_censored(FAMILY)) {
    // y is the row's value, m its status; hlt = 1/2 log(tau / (2 pi))
    *mu = FAMILY == PRED_LOGNORMAL ? exp(eta) : eta;
    if (SCORE) {
      const double a = (y - eta) * sqrt(tau);
      *ll = m == 0. ? hlt - 0.5 * (a * a) : log_norm_cdf(m == 1. ? -a : a);
    }
  } else if (FAMILY == PRED_PROBIT) {
    // Phi(eta) = erfc(-eta / sqrt 2) / 2: absolute error ~1e-16, what a mean
    // needs; the score is the log of the outcome's own tail
    *mu = 0.5 * erfc(-0.70710678118654752440 * eta);
    if (SCORE) *ll = log_norm_cdf(y != 0. ? eta : -eta);
  } else {
    // negative binomial: r and log r of the draw are in its table
    *mu = exp(eta);
    if (SCORE) {
      const double r = gtab[NEGBIN_TAB_R];
      const double t = eta - gtab[NEGBIN_TAB_R + 1];
      double sp, sg;
      negbin_link(t, &sp, &sg);
      *ll = negbin_G(y, r, gtab) + negbin_beta_part(y, r, t, sp);
    }
  }
  if (SCORE && has_c) *ll += c;
}

// Welford's mean with the contract's rule for an infinite one
__device__ __forceinline__ double welford_mean(double mean, double x,
                                               double delta, double k) {
  if (isinf(mean)) return (x != x || x == -mean) ? NAN : mean;
  return mean + delta / k;
}

// The two accumulators of the head comment, by value in a thread's
// registers.  `st` is the accumulator's first state plane, `n` the length of
// a plane, `i` the row.
struct Moments {
  double mean = 0., m2 = 0.;   // fresh
  __device__ __forceinline__ void load(const double* st, int64_t n,
                                       int64_t i) {
    mean = st[i];
    m2 = st[n + i];
  }
  __device__ __forceinline__ void push(double x, double k) {
    const double delta = x - mean;
    mean = welford_mean(mean, x, delta, k);
    m2 += delta * (x - mean);
  }
  __device__ __forceinline__ void store(double* st, int64_t n,
                                        int64_t i) const {
    st[i] = mean;
    st[n + i] = m2;
  }
  // the mean and the population sd over the S draws, each into its own plane
  __device__ __forceinline__ void finish(double S, double* mean_out,
                                         double* sd_out, int64_t i) const {
    mean_out[i] = mean;
    sd_out[i] = sqrt(m2 / S);
  }
};

struct Scores {
  Moments ll;
  double lmax = -INFINITY, lsum = 0.;
  __device__ __forceinline__ void load(const double* st, int64_t n,
                                       int64_t i) {
    ll.load(st, n, i);
    lmax = st[2 * n + i];
    lsum = st[3 * n + i];
  }
  __device__ __forceinline__ void push(double x, double k) {
    ll.push(x, k);
    if (x > lmax) {
      lsum = lsum * exp(lmax - x) + 1.;
      lmax = x;
    } else if (x != -INFINITY) {   // (-inf adds exactly 0; a NaN gets here)
      lsum += exp(x - lmax);
    }
  }
  __device__ __forceinline__ void store(double* st, int64_t n,
                                        int64_t i) const {
    ll.store(st, n, i);
    st[2 * n + i] = lmax;
    st[3 * n + i] = lsum;
  }
  // lpd, ll_mean, ll_var into three planes from `out`
  __device__ __forceinline__ void finish(double S, double* out, int64_t n,
                                         int64_t i) const {
    out[i] = lmax + log(lsum) - log(S);
    out[n + i] = ll.mean;
    out[2 * n + i] = ll.m2 / (S - 1.);
  }
};

template <int FAMILY, bool SCORE>
static __global__ __launch_bounds__(PRED_BLOCK) void predict_summary_kernel(
    PredArgs a) {
  const int64_t i = (int64_t)blockIdx.x * PRED_BLOCK + threadIdx.x;
  const int64_t n = a.n;
  if (i >= n) return;
  Moments mom;
  Scores sc;   // (used with an outcome only)
  if (a.k0 > 0) {
    mom.load(a.state, n, i);
    if (SCORE) sc.load(a.state + 2 * n, n, i);
  }
  const bool has_off = a.offset != nullptr;
  const double off = has_off ? a.offset[i] : 0.;
  const double y = SCORE ? a.y[i] : 0.;
  const bool has_m = FAMILY == BBX_PRED_LOGIT || FAMILY == PRED_WEIBULL ||
                     pred_censored(FAMILY);
  const double m = SCORE && has_m && a.m ? a.m[i] : 1.;
  const bool has_c = SCORE && a.c != nullptr;
  const double c = has_c ? a.c[i] : 0.;
  // (the negative-binomial body unrolled holds more wave-uniform values than
  // there are scalar registers)
#pragma unroll FAMILY == PRED_NEGBIN ? 1 : 4
  for (int d = 0; d < a.kn; ++d) {
    double eta = a.eta[(int64_t)d * n + i];
    if (has_off) eta += off;
    const double k = (double)(a.k0 + d + 1);
    double tau = 0., hlt = 0.;
    if (((FAMILY == BBX_PRED_LINEAR || FAMILY == PRED_STUDENT_T ||
          FAMILY == PRED_QUANTILE || pred_censored(FAMILY)) &&
         SCORE) ||
        FAMILY == PRED_WEIBULL) {
      tau = a.tau[a.k0 + d];
      hlt = a.hlt[a.k0 + d];
    }
    double mu, ll = 0.;
    const double* gtab =
        FAMILY == PRED_NEGBIN && SCORE
            ? a.gtab + (a.k0 + d) * (int64_t)NEGBIN_GTAB
        : (FAMILY == PRED_STUDENT_T || FAMILY == PRED_QUANTILE) && SCORE
            ? a.gtab
            : nullptr;
    pred_terms<FAMILY, SCORE>(eta, y, m, c, has_c, tau, hlt, gtab, &mu, &ll);
    if (a.mu_draws) a.mu_draws[(int64_t)d * n + i] = mu;
    mom.push(mu, k);
    if (SCORE) sc.push(ll, k);
  }
  if (a.k0 + a.kn < a.n_draw) {
    mom.store(a.state, n, i);
    if (SCORE) sc.store(a.state + 2 * n, n, i);
    return;
  }
  const double S = (double)a.n_draw;
  mom.finish(S, a.out, a.out + n, i);
  if (SCORE) sc.finish(S, a.out + 2 * n, n, i);
}

template <int FAMILY>
static void launch_summary(hipStream_t s, bool score, const PredArgs& a) {
  const dim3 grid((unsigned)((a.n + PRED_BLOCK - 1) / PRED_BLOCK));
  // (named first: a comma inside the launch macro's argument would split it)
  auto kernel = score ? predict_summary_kernel<FAMILY, true>
                      : predict_summary_kernel<FAMILY, false>;
  BBX_LAUNCH(kernel, grid, dim3(PRED_BLOCK), 0, s, a);
}

// The host side every family shares: the draws go through in passes of `per`
// draws -- `per` products into the eta buffer, then the family's summary
// kernel(s) over them and, where asked for, the pass's mu draws back -- all on
// the design's stream, in the order uploads, products and summaries pass by
// pass, the results back, ONE synchronisation (finish): the host arrays
// handed to begin, upload and row outlive their copies.  (Internal linkage, as
// the static functions around it: the library exports none of it.)
namespace {
struct PredPasses {
  bbx_design* h = nullptr;
  int64_t n_draw = 0, per = 0, pitch = 0;
  size_t nb = 0;             // bytes of an n-vector
  DevMem d_beta, d_eta, d_mu, d_up[5];
  int n_up = 0;
  double* mu_host = nullptr;   // [S][n] or null: every draw's mu, pass by pass
  // Sizes the pass (draws_per_pass, or 0: PRED_DRAWS, fewer where the eta and,
  // with mu_draws, the mu of a pass would exceed PRED_BUDGET, never below 1),
  // allocates them and uploads the draws coef[S][P].
  int begin(bbx_design* design, int64_t S, const double* coef,
            int draws_per_pass, double* mu_draws = nullptr) {
    const size_t d8 = sizeof(double);
    h = design;
    n_draw = S;
    mu_host = mu_draws;
    nb = d8 * (size_t)h->n;
    const int64_t P = h->P;
    const int64_t fit = (int64_t)(PRED_BUDGET / (nb * (mu_host ? 2 : 1)));
    per = draws_per_pass;
    if (per == 0)
      per = std::max<int64_t>(1, std::min<int64_t>(PRED_DRAWS, fit));
    per = std::min(per, S);
    // every draw starts 256 bytes apart, as the staging vector of
    // bbx_design_dot does: the product kernels take the same path
    pitch = (P + 31) / 32 * 32;
    BBX_TRY(d_beta.alloc(d8 * (size_t)pitch * (size_t)S));
    BBX_TRY(d_eta.alloc(nb * (size_t)per));
    if (mu_host) BBX_TRY(d_mu.alloc(nb * (size_t)per));
    BBX_HIP(hipMemcpy2DAsync(d_beta.ptr, d8 * (size_t)pitch, coef,
                             d8 * (size_t)P, d8 * (size_t)P, (size_t)S,
                             hipMemcpyHostToDevice, h->stream));
    return BBX_OK;
  }
  // a host array on the device for the length of the call (at most 5)
  int upload(const double* host, size_t bytes, const double** dev) {
    DevMem& d = d_up[n_up++];
    BBX_TRY(d.alloc(bytes));
    BBX_HIP(hipMemcpyAsync(d.ptr, host, bytes, hipMemcpyHostToDevice,
                           h->stream));
    *dev = d.as<const double>();
    return BBX_OK;
  }
  // an optional n-vector: *dev stays null for a null host
  int row(const double* host, const double** dev) {
    return host ? upload(host, nb, dev) : BBX_OK;
  }
  // `pass(k0, kn)` launches the family's summary of the kn draws from k0,
  // whose linear predictors are in eta[kn][n]
  template <class Pass>
  int run(Pass&& pass) {
    for (int64_t k0 = 0; k0 < n_draw; k0 += per) {
      const int kn = (int)(k0 + per < n_draw ? per : n_draw - k0);
      for (int d = 0; d < kn; ++d) {
        const double* b = d_beta.as<const double>() + (k0 + d) * pitch;
        BBX_TRY(launch_prep_v(h, b, nullptr, nullptr, part_slot(h, PS_C)));
        BBX_TRY(launch_dot(h, b, nullptr,
                           d_eta.as<double>() + (int64_t)d * h->n, nullptr));
      }
      pass(k0, kn);
      BBX_HIP(hipGetLastError());
      if (mu_host)
        BBX_HIP(hipMemcpyAsync(mu_host + k0 * h->n, d_mu.ptr, nb * (size_t)kn,
                               hipMemcpyDeviceToHost, h->stream));
    }
    return BBX_OK;
  }
  // The results out[mean_k ..., sd_k ..., lpd, ll_mean, ll_var][n], k < K, to
  // the host arrays res[5] (the last three with `score` only), then the
  // call's one synchronisation.
  int finish(const double* out, int64_t K, bool score, double* const res[5]) {
    for (int r = 0; r < (score ? 5 : 2); ++r) {
      const int64_t plane = r < 2 ? r * K : 2 * K + r - 2;
      BBX_HIP(hipMemcpyAsync(res[r], out + plane * h->n, nb * (r < 2 ? K : 1),
                             hipMemcpyDeviceToHost, h->stream));
    }
    BBX_HIP(hipStreamSynchronize(h->stream));
    return BBX_OK;
  }
};
}  // namespace

struct PredCall {
  bbx_design* h;
  int family;
  int64_t n_draw;
  const double *coef, *obs_prec, *offset, *y, *n_trial, *ll_const;
  int draws_per_pass;
  double *mean, *sd, *lpd, *ll_mean, *ll_var, *mu_draws;
  double df = 0.;   // Student-t: the degrees of freedom; quantile: the level q
};

// `launch(stream, score, args)` starts the summary kernel of q.family: the
// translation unit chooses which instantiations it holds.
template <class Launch>
static int predictive_summary_impl(const PredCall& q, Launch&& launch) {
  const int64_t n = q.h->n, S = q.n_draw;
  const size_t d8 = sizeof(double);
  const bool score = q.y != nullptr;
  const bool linear = q.family == BBX_PRED_LINEAR;
  const bool negbin = q.family == PRED_NEGBIN;
  const bool weibull = q.family == PRED_WEIBULL;
  const bool student_t = q.family == PRED_STUDENT_T;
  const bool censored = pred_censored(q.family);
  const bool quantile = q.family == PRED_QUANTILE;

  PredPasses p;
  DevMem d_state, d_out;
  BBX_TRY(p.begin(q.h, S, q.coef, q.draws_per_pass, q.mu_draws));
  BBX_TRY(d_state.alloc(p.nb * PRED_STATE));
  BBX_TRY(d_out.alloc(p.nb * 5));
  std::vector<double> tau_host;
  if (negbin && score) {
    // (obs_prec holds the draws' dispersion)
    tau_host.resize((size_t)NEGBIN_GTAB * (size_t)S);
    for (int64_t d = 0; d < S; ++d)
      negbin_gtab(q.obs_prec[d], &tau_host[d * NEGBIN_GTAB]);
  }
  if (linear && score) {
    tau_host.resize(2 * (size_t)S);
    for (int64_t d = 0; d < S; ++d) {
      tau_host[d] = q.obs_prec[d];
      tau_host[S + d] = 0.5 * log(q.obs_prec[d]);
    }
  }
  if (weibull) {
    // (obs_prec holds the draws' shape: the median needs it without an
    // outcome too)
    tau_host.resize(2 * (size_t)S);
    for (int64_t d = 0; d < S; ++d) {
      tau_host[d] = q.obs_prec[d];
      tau_host[S + d] = log(q.obs_prec[d]);
    }
  }
  if (student_t && score) {
    // per draw tau and the density's constant, then (df + 1) / 2 and df
    tau_host.resize(2 * (size_t)S + 2);
    const double lg = std::lgamma((q.df + 1.) / 2.) - std::lgamma(q.df / 2.);
    for (int64_t d = 0; d < S; ++d) {
      tau_host[d] = q.obs_prec[d];
      tau_host[S + d] = lg + 0.5 * log(q.obs_prec[d] / (q.df * M_PI));
    }
    tau_host[2 * S] = (q.df + 1.) / 2.;
    tau_host[2 * S + 1] = q.df;
  }
  if (quantile && score) {
    // per draw tau and log tau + log(q (1 - q)), then q
    tau_host.resize(2 * (size_t)S + 1);
    const double lqq = log(q.df * (1. - q.df));
    for (int64_t d = 0; d < S; ++d) {
      tau_host[d] = q.obs_prec[d];
      tau_host[S + d] = log(q.obs_prec[d]) + lqq;
    }
    tau_host[2 * S] = q.df;
  }
  if (censored && q.obs_prec) {
    // (without an outcome too: the survival summary needs the draws' tau)
    tau_host.resize(2 * (size_t)S);
    for (int64_t d = 0; d < S; ++d) {
      tau_host[d] = q.obs_prec[d];
      tau_host[S + d] = 0.5 * log(q.obs_prec[d] / (2. * M_PI));
    }
  }
  const double* tab = nullptr;
  if (!tau_host.empty())
    BBX_TRY(p.upload(tau_host.data(), d8 * tau_host.size(), &tab));

  PredArgs a{};
  a.n = n;
  a.n_draw = S;
  a.eta = p.d_eta.as<const double>();
  if (linear || weibull || student_t || censored || quantile) {
    a.tau = tab;
    a.hlt = tab ? tab + S : nullptr;
    if (student_t || quantile) a.gtab = tab ? tab + 2 * S : nullptr;
  } else {
    a.gtab = tab;
  }
  BBX_TRY(p.row(q.offset, &a.offset));
  BBX_TRY(p.row(score ? q.y : nullptr, &a.y));
  BBX_TRY(p.row(
      score && (q.family == BBX_PRED_LOGIT || weibull || censored) ? q.n_trial
                                                                    : nullptr,
      &a.m));
  BBX_TRY(p.row(score ? q.ll_const : nullptr, &a.c));
  a.state = d_state.as<double>();
  a.out = d_out.as<double>();
  a.mu_draws = p.d_mu.as<double>();
  BBX_TRY(p.run([&](int64_t k0, int kn) {
    a.k0 = k0;
    a.kn = kn;
    launch(q.h->stream, score, a);
  }));
  double* const res[5] = {q.mean, q.sd, q.lpd, q.ll_mean, q.ll_var};
  return p.finish(a.out, 1, score, res);
}

}  // namespace pred
}  // namespace bbx
