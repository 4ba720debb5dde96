// The streaming summary kernel of posterior prediction and its host driver,
// shared by predict.hip (linear, logit, Poisson: bbx_design_predictive_summary)
// and negbin_predict.hip (negative binomial:
// bbx_design_predictive_summary_negbin).  The kernel and the driver are static
// templates: a translation unit holds the instantiations it launches and no
// others.  predict.hip describes the method.
#pragma once
#include <math.h>

#include <cmath>

#include <string>
#include <vector>

#include "common.hpp"
#include "negbin_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {
namespace pred {

constexpr int PRED_BLOCK = 256;
constexpr int PRED_DRAWS = 16;                    // default draws per pass
constexpr size_t PRED_BUDGET = size_t(256) << 20; // eta (+ mu draws) of a pass
constexpr int PRED_STATE = 6;  // mean, M2 of mu; mean, M2 of ll; max, sum
// The negative-binomial model's code.  Not a BBX_PRED_* of include/bbx.h:
// bbx_design_predictive_summary refuses it, the family has its own entry point
// and its instantiation lives in negbin_predict.hip.
constexpr int PRED_NEGBIN = 3;

struct PredArgs {
  int64_t n;
  int64_t k0;       // draws folded into the state before this pass
  int kn;           // draws of this pass
  int64_t n_draw;   // all draws: the last pass writes the results
  const double* eta;      // [kn][n]
  const double* tau;      // [n_draw] linear: obs_prec
  const double* hlt;      // [n_draw] linear: 0.5 log(obs_prec)
  const double* gtab;     // [n_draw][NEGBIN_GTAB] negbin: negbin_gtab(r)
  const double* offset;   // [n] or null
  const double* y;        // [n]   (SCORE)
  const double* m;        // [n] or null (logit, SCORE)
  const double* c;        // [n] or null (SCORE)
  double* state;          // [PRED_STATE][n]
  double* out;            // [5][n]: mean, sd, lpd, ll_mean, ll_var
  double* mu_draws;       // [kn][n] or null
};

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
    const double e = exp(-fabs(eta));
    *mu = eta >= 0. ? 1. / (1. + e) : e / (1. + e);
    if (SCORE) {
      const double sp = fmax(eta, 0.) + log1p(e);
      *ll = y * eta - m * sp;
    }
  } else if (FAMILY == BBX_PRED_POISSON) {
    *mu = exp(eta);
    if (SCORE) *ll = y * eta - *mu;
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

// Welford's mean.  Once a draw has overflowed (a Poisson mu of +inf, its ll of
// -inf) the mean is that infinity and stays it, as the plain sum would:
// inf - inf in the update would turn it into a NaN.  A NaN draw or the
// opposite infinity still gives a NaN.  (M2 is a NaN from there on: the
// spread of infinite values has no value.)
__device__ __forceinline__ double welford_mean(double mean, double x,
                                               double delta, double k) {
  if (isinf(mean)) return (x != x || x == -mean) ? NAN : mean;
  return mean + delta / k;
}

template <int FAMILY, bool SCORE>
static __global__ __launch_bounds__(PRED_BLOCK) void predict_summary_kernel(
    PredArgs a) {
  const int64_t i = (int64_t)blockIdx.x * PRED_BLOCK + threadIdx.x;
  const int64_t n = a.n;
  if (i >= n) return;
  double mean = 0., m2 = 0., lmean = 0., lm2 = 0., lmax = -INFINITY, lsum = 0.;
  if (a.k0 > 0) {
    mean = a.state[i];
    m2 = a.state[n + i];
    if (SCORE) {
      lmean = a.state[2 * n + i];
      lm2 = a.state[3 * n + i];
      lmax = a.state[4 * n + i];
      lsum = a.state[5 * n + i];
    }
  }
  const bool has_off = a.offset != nullptr;
  const double off = has_off ? a.offset[i] : 0.;
  const double y = SCORE ? a.y[i] : 0.;
  const double m = SCORE && FAMILY == BBX_PRED_LOGIT && a.m ? a.m[i] : 1.;
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
    if (FAMILY == BBX_PRED_LINEAR && SCORE) {
      tau = a.tau[a.k0 + d];
      hlt = a.hlt[a.k0 + d];
    }
    double mu, ll = 0.;
    const double* gtab =
        FAMILY == PRED_NEGBIN && SCORE
            ? a.gtab + (a.k0 + d) * (int64_t)NEGBIN_GTAB
            : nullptr;
    pred_terms<FAMILY, SCORE>(eta, y, m, c, has_c, tau, hlt, gtab, &mu, &ll);
    if (a.mu_draws) a.mu_draws[(int64_t)d * n + i] = mu;
    const double delta = mu - mean;
    mean = welford_mean(mean, mu, delta, k);
    m2 += delta * (mu - mean);
    if (SCORE) {
      const double ld = ll - lmean;
      lmean = welford_mean(lmean, ll, ld, k);
      lm2 += ld * (ll - lmean);
      if (ll > lmax) {
        lsum = lsum * exp(lmax - ll) + 1.;
        lmax = ll;
      } else if (ll != -INFINITY) {   // (-inf adds exactly 0; a NaN gets here)
        lsum += exp(ll - lmax);
      }
    }
  }
  if (a.k0 + a.kn < a.n_draw) {
    a.state[i] = mean;
    a.state[n + i] = m2;
    if (SCORE) {
      a.state[2 * n + i] = lmean;
      a.state[3 * n + i] = lm2;
      a.state[4 * n + i] = lmax;
      a.state[5 * n + i] = lsum;
    }
    return;
  }
  const double S = (double)a.n_draw;
  a.out[i] = mean;
  a.out[n + i] = sqrt(m2 / S);
  if (SCORE) {
    a.out[2 * n + i] = lmax + log(lsum) - log(S);
    a.out[3 * n + i] = lmean;
    a.out[4 * n + i] = lm2 / (S - 1.);
  }
}

template <int FAMILY>
static void launch_summary(hipStream_t s, bool score, const PredArgs& a) {
  const dim3 grid((unsigned)((a.n + PRED_BLOCK - 1) / PRED_BLOCK));
  // (named first: a comma inside the launch macro's argument would split it)
  auto kernel = score ? predict_summary_kernel<FAMILY, true>
                      : predict_summary_kernel<FAMILY, false>;
  BBX_LAUNCH(kernel, grid, dim3(PRED_BLOCK), 0, s, a);
}

struct PredCall {
  bbx_design* h;
  int family;
  int64_t n_draw;
  const double *coef, *obs_prec, *offset, *y, *n_trial, *ll_const;
  int draws_per_pass;
  double *mean, *sd, *lpd, *ll_mean, *ll_var, *mu_draws;
};

// `launch(stream, score, args)` starts the summary kernel of q.family: the
// translation unit chooses which instantiations it holds.
template <class Launch>
static int predictive_summary_impl(const PredCall& q, Launch&& launch) {
  bbx_design* h = q.h;
  hipStream_t s = h->stream;
  const int64_t n = h->n, P = h->P, S = q.n_draw;
  const size_t d8 = sizeof(double);
  const size_t nb = d8 * (size_t)n;
  const bool score = q.y != nullptr;
  const bool linear = q.family == BBX_PRED_LINEAR;
  const bool negbin = q.family == PRED_NEGBIN;

  int64_t K = q.draws_per_pass;
  if (K == 0) {
    K = PRED_DRAWS;
    const int64_t fit =
        (int64_t)(PRED_BUDGET / (nb * (q.mu_draws ? 2 : 1)));
    if (K > fit) K = fit;
    if (K < 1) K = 1;
  }
  if (K > S) K = S;

  // every draw starts 256 bytes apart, as the staging vector of
  // bbx_design_dot does: the product kernels take the same path
  const int64_t pitch = (P + 31) / 32 * 32;
  DevMem d_beta, d_tau, d_eta, d_state, d_out, d_mu, d_row[4];
  BBX_TRY(d_beta.alloc(d8 * (size_t)pitch * (size_t)S));
  BBX_TRY(d_eta.alloc(nb * (size_t)K));
  BBX_TRY(d_state.alloc(nb * PRED_STATE));
  BBX_TRY(d_out.alloc(nb * 5));
  if (q.mu_draws) BBX_TRY(d_mu.alloc(nb * (size_t)K));
  BBX_HIP(hipMemcpy2DAsync(d_beta.ptr, d8 * (size_t)pitch, q.coef,
                           d8 * (size_t)P, d8 * (size_t)P, (size_t)S,
                           hipMemcpyHostToDevice, s));
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
  if (!tau_host.empty()) {
    BBX_TRY(d_tau.alloc(d8 * tau_host.size()));
    BBX_HIP(hipMemcpyAsync(d_tau.ptr, tau_host.data(), d8 * tau_host.size(),
                           hipMemcpyHostToDevice, s));
  }
  const double* rows[4] = {q.offset, score ? q.y : nullptr,
                           score && q.family == BBX_PRED_LOGIT ? q.n_trial
                                                               : nullptr,
                           score ? q.ll_const : nullptr};
  for (int r = 0; r < 4; ++r) {
    if (!rows[r]) continue;
    BBX_TRY(d_row[r].alloc(nb));
    BBX_HIP(hipMemcpyAsync(d_row[r].ptr, rows[r], nb, hipMemcpyHostToDevice,
                           s));
  }

  PredArgs a{};
  a.n = n;
  a.n_draw = S;
  a.eta = d_eta.as<const double>();
  if (linear) {
    a.tau = d_tau.as<const double>();
    a.hlt = d_tau.ptr ? d_tau.as<const double>() + S : nullptr;
  } else {
    a.gtab = d_tau.as<const double>();
  }
  a.offset = d_row[0].as<const double>();
  a.y = d_row[1].as<const double>();
  a.m = d_row[2].as<const double>();
  a.c = d_row[3].as<const double>();
  a.state = d_state.as<double>();
  a.out = d_out.as<double>();
  a.mu_draws = d_mu.as<double>();
  for (int64_t k0 = 0; k0 < S; k0 += K) {
    const int kn = (int)(k0 + K < S ? K : S - k0);
    for (int d = 0; d < kn; ++d) {
      const double* b = d_beta.as<const double>() + (k0 + d) * pitch;
      BBX_TRY(launch_prep_v(h, b, nullptr, nullptr, part_slot(h, PS_C)));
      BBX_TRY(launch_dot(h, b, nullptr, d_eta.as<double>() + (int64_t)d * n,
                         nullptr));
    }
    a.k0 = k0;
    a.kn = kn;
    launch(s, score, a);
    BBX_HIP(hipGetLastError());
    if (q.mu_draws)
      BBX_HIP(hipMemcpyAsync(q.mu_draws + k0 * n, d_mu.ptr, nb * (size_t)kn,
                             hipMemcpyDeviceToHost, s));
  }
  double* outs[5] = {q.mean, q.sd, q.lpd, q.ll_mean, q.ll_var};
  for (int r = 0; r < (score ? 5 : 2); ++r)
    BBX_HIP(hipMemcpyAsync(outs[r], d_out.as<double>() + (int64_t)r * n, nb,
                           hipMemcpyDeviceToHost, s));
  BBX_HIP(hipStreamSynchronize(s));
  return BBX_OK;
}


}  // namespace pred
}  // namespace bbx
