// Posterior prediction and pointwise predictive scores of the linear, logit
// and Poisson models from draws of the coefficients
// (bbx_design_predictive_summary, include/bbx.h).
//
// Per draw s the linear predictor eta_s = X~ beta_s is formed on the device by
// the launches of bbx_design_dot (launch_prep_v + launch_dot, as ham::eta_of),
// so a draw's eta has that call's bits.  The draws go through in blocks of K:
// K products into a K x n buffer, then ONE summary kernel that walks the K
// etas of every row in draw order and updates the row's running statistics:
//
//   mu_s  = eta | 1 / (1 + exp(-eta)) | exp(eta)     (eta = X~ beta_s + offset)
//   ll_s  = the row's log-likelihood term of draw s (see pred_terms)
//   Welford on mu and on ll, k the 1-based draw index:
//     delta = x - mean;  mean += delta / k;  M2 += delta * (x - mean)
//     (an infinite mean stays: welford_mean)
//   lpd online: ll > M ? (sum = sum * exp(M - ll) + 1, M = ll)
//                      : (sum += exp(ll - M));  a draw of -inf adds exactly 0
//
// One update per draw whatever K is, so the results do not depend on K.  The
// state (six doubles per row, SoA) lives in HBM between blocks and in
// registers within one; the first block starts it in registers and the last
// one writes the five results instead.  Rows along the lanes, one row per
// thread: eta, the state and the optional mu draws (draw-major) are read and
// written 64 consecutive doubles per wave.  No atomics, no reduction across
// rows: the same inputs give the same bits.
//
// Per-draw traffic: 8 B per row for eta plus (48 B read + 48 B written) / K
// for the state; K = 16 makes the state's share 6 B.  K x n x 8 B (twice that
// with mu_draws) stays within PRED_BUDGET, but K never goes below 1.
#include <math.h>

#include <cmath>

#include <string>
#include <vector>

#include "common.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

namespace {

constexpr int PRED_BLOCK = 256;
constexpr int PRED_DRAWS = 16;                    // default draws per pass
constexpr size_t PRED_BUDGET = size_t(256) << 20; // eta (+ mu draws) of a pass
constexpr int PRED_STATE = 6;  // mean, M2 of mu; mean, M2 of ll; max, sum

struct PredArgs {
  int64_t n;
  int64_t k0;       // draws folded into the state before this pass
  int kn;           // draws of this pass
  int64_t n_draw;   // all draws: the last pass writes the results
  const double* eta;      // [kn][n]
  const double* tau;      // [n_draw] linear: obs_prec
  const double* hlt;      // [n_draw] linear: 0.5 log(obs_prec)
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
                                           double hlt, double* mu,
                                           double* ll) {
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
  } else {
    *mu = exp(eta);
    if (SCORE) *ll = y * eta - *mu;
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
__global__ __launch_bounds__(PRED_BLOCK) void predict_summary_kernel(
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
#pragma unroll 4
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
    pred_terms<FAMILY, SCORE>(eta, y, m, c, has_c, tau, hlt, &mu, &ll);
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
void launch_summary(hipStream_t s, bool score, const PredArgs& a) {
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

int predictive_summary_impl(const PredCall& q) {
  bbx_design* h = q.h;
  hipStream_t s = h->stream;
  const int64_t n = h->n, P = h->P, S = q.n_draw;
  const size_t d8 = sizeof(double);
  const size_t nb = d8 * (size_t)n;
  const bool score = q.y != nullptr;
  const bool linear = q.family == BBX_PRED_LINEAR;

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
  if (linear && score) {
    tau_host.resize(2 * (size_t)S);
    for (int64_t d = 0; d < S; ++d) {
      tau_host[d] = q.obs_prec[d];
      tau_host[S + d] = 0.5 * log(q.obs_prec[d]);
    }
    BBX_TRY(d_tau.alloc(d8 * 2 * (size_t)S));
    BBX_HIP(hipMemcpyAsync(d_tau.ptr, tau_host.data(), d8 * 2 * (size_t)S,
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
  a.tau = d_tau.as<const double>();
  a.hlt = d_tau.ptr ? d_tau.as<const double>() + S : nullptr;
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
    if (q.family == BBX_PRED_LINEAR) {
      launch_summary<BBX_PRED_LINEAR>(s, score, a);
    } else if (q.family == BBX_PRED_LOGIT) {
      launch_summary<BBX_PRED_LOGIT>(s, score, a);
    } else {
      launch_summary<BBX_PRED_POISSON>(s, score, a);
    }
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

}  // namespace

extern "C" int bbx_design_predictive_summary(
    bbx_design* design, int family, int64_t n_draw, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const double* n_trial, const double* ll_const, int draws_per_pass,
    double* mean, double* sd, double* lpd, double* ll_mean, double* ll_var,
    double* mu_draws) {
  const char* who = "bbx_design_predictive_summary: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the design is NULL or destroyed");
  if (family < BBX_PRED_LINEAR || family > BBX_PRED_POISSON)
    return fail(BBX_ERR_INVALID, std::string(who) + "family " +
                                     std::to_string(family) +
                                     " is not 0 (linear), 1 (logit) or 2 "
                                     "(Poisson)");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_draw must be at least 1");
  if (!coef) return fail(BBX_ERR_INVALID, std::string(who) + "coef is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, std::string(who) + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, std::string(who) + "sd is NULL");
  if (y && !lpd)
    return fail(BBX_ERR_INVALID, std::string(who) + "y is given but lpd is NULL");
  if (y && !ll_mean)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "y is given but ll_mean is NULL");
  if (y && !ll_var)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "y is given but ll_var is NULL");
  if (family == BBX_PRED_LINEAR && !obs_prec)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "the linear model needs obs_prec");
  if (family != BBX_PRED_LINEAR && obs_prec)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "obs_prec is an argument of the linear "
                                   "model only");
  if (obs_prec) {
    for (int64_t d = 0; d < n_draw; ++d) {
      if (!(obs_prec[d] > 0.) || !std::isfinite(obs_prec[d]))
        return fail(BBX_ERR_INVALID, std::string(who) + "obs_prec[" +
                                         std::to_string(d) +
                                         "] is not finite and positive");
    }
  }
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID,
                std::string(who) + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    BBX_HIP(hipSetDevice(design->device));
    const PredCall q{design, family,  n_draw,  coef,   obs_prec,
                     offset, y,       n_trial, ll_const, draws_per_pass,
                     mean,   sd,      lpd,     ll_mean, ll_var,
                     mu_draws};
    return predictive_summary_impl(q);
  });
}
