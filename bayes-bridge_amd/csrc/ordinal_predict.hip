// Posterior prediction and pointwise predictive scores of the
// proportional-odds model from draws of the coefficients and of the
// cutpoints: the category probabilities' posterior mean and spread per row
// and, with an outcome, the scoring states of predict_summary.hpp on the
// row's log-probability.  A kernel of its own: a row has K probabilities, not
// one mean, so the state is 2 K + 4 values per row, laid out state-major
// ([state][n]: every access is coalesced), and the launch has one plane of
// workgroups per category (blockIdx.y = k: Welford's mean and M2 of p_k in
// two registers) plus, with an outcome, one for the scores.  A plane reads the
// pass's linear predictors once; K + 1 planes read them from the cache.  No
// thread shares a state with another: no atomics, and the updates of a row
// run in draw order whatever the pass size.
//
//   p_k = sigma(c_{k+1} - xo) - sigma(c_k - xo)   (absolute error ~1e-16: what
//                                                  a mean needs)
//   ll  = (g_y - softplus(xo - c_{y+1})) - softplus(c_y - xo)   (the stable
//                                                  form of ordinal_terms.hpp)
#include "predict_summary.hpp"
// (after it: the device qualifiers are the HIP runtime's, which common.hpp
// brings in)
#include "ordinal_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {
namespace pred {

struct OrdinalPredArgs {
  int64_t n;
  int64_t k0;       // draws folded into the state before this pass
  int kn;           // draws of this pass
  int64_t n_draw;   // all draws: the last pass writes the results
  int K;            // categories
  const double* eta;      // [kn][n]
  const double* tab;      // [n_draw][K][ORDINAL_TAB]: ordinal_tab of a draw
  const double* offset;   // [n] or null
  const double* y;        // [n] (the scoring plane)
  double* state;          // [2 K + 4][n]: mean_k, M2_k ...; ll mean, M2, max, sum
  double* out;            // [2 K + 3][n]: mean_k ..., sd_k ..., lpd, ll_mean, ll_var
};

__device__ __forceinline__ double ordinal_sigma(double x) {
  const double e = exp(-fabs(x));
  return x >= 0. ? 1. / (1. + e) : e / (1. + e);
}

static __global__ __launch_bounds__(PRED_BLOCK) void ordinal_summary_kernel(
    OrdinalPredArgs a) {
  const int64_t i = (int64_t)blockIdx.x * PRED_BLOCK + threadIdx.x;
  const int64_t n = a.n;
  if (i >= n) return;
  const int plane = blockIdx.y;   // < K: a category; K: the scores
  const int K = a.K;
  const bool has_off = a.offset != nullptr;
  const double off = has_off ? a.offset[i] : 0.;
  const bool last = a.k0 + a.kn >= a.n_draw;
  const double S = (double)a.n_draw;
  const int64_t tstride = (int64_t)ORDINAL_TAB * K;
  if (plane < K) {
    double* st = a.state + (int64_t)(2 * plane) * n;
    double mean = 0., m2 = 0.;
    if (a.k0 > 0) {
      mean = st[i];
      m2 = st[n + i];
    }
    // (the table's entries of a draw are wave-uniform: two draws in flight
    // hold as many scalar registers as the kernel can spare)
#pragma unroll 2
    for (int d = 0; d < a.kn; ++d) {
      double xo = a.eta[(int64_t)d * n + i];
      if (has_off) xo += off;
      const double* t = a.tab + (a.k0 + d) * tstride + ORDINAL_TAB * plane;
      const double p = ordinal_sigma(t[1] - xo) - ordinal_sigma(t[0] - xo);
      const double k = (double)(a.k0 + d + 1);
      const double delta = p - mean;
      mean = welford_mean(mean, p, delta, k);
      m2 += delta * (p - mean);
    }
    if (!last) {
      st[i] = mean;
      st[n + i] = m2;
      return;
    }
    a.out[(int64_t)plane * n + i] = mean;
    a.out[(int64_t)(K + plane) * n + i] = sqrt(m2 / S);
    return;
  }
  double* st = a.state + (int64_t)(2 * K) * n;
  double lmean = 0., lm2 = 0., lmax = -INFINITY, lsum = 0.;
  if (a.k0 > 0) {
    lmean = st[i];
    lm2 = st[n + i];
    lmax = st[2 * n + i];
    lsum = st[3 * n + i];
  }
  // (a valid category: checked on the host)
  const int cat = ORDINAL_TAB * (int)a.y[i];
#pragma unroll 1
  for (int d = 0; d < a.kn; ++d) {
    double xo = a.eta[(int64_t)d * n + i];
    if (has_off) xo += off;
    const double* t = a.tab + (a.k0 + d) * tstride + cat;
    const double ll = ordinal_ll(xo, t[0], t[1], t[2]);
    const double k = (double)(a.k0 + d + 1);
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
  if (!last) {
    st[i] = lmean;
    st[n + i] = lm2;
    st[2 * n + i] = lmax;
    st[3 * n + i] = lsum;
    return;
  }
  double* out = a.out + (int64_t)(2 * K) * n;
  out[i] = lmax + log(lsum) - log(S);
  out[n + i] = lmean;
  out[2 * n + i] = lm2 / (S - 1.);
}

struct OrdinalPredCall {
  bbx_design* h;
  int64_t n_draw;
  int K;
  const double *coef, *cuts, *offset, *y;
  int draws_per_pass;
  double *mean, *sd, *lpd, *ll_mean, *ll_var;
};

// predictive_summary_impl for this family: the same passes, the same single
// synchronisation
static int ordinal_summary_impl(const OrdinalPredCall& q) {
  bbx_design* h = q.h;
  hipStream_t s = h->stream;
  const int64_t n = h->n, P = h->P, S = q.n_draw;
  const int K = q.K;
  const size_t d8 = sizeof(double);
  const size_t nb = d8 * (size_t)n;
  const bool score = q.y != nullptr;

  int64_t per = q.draws_per_pass;
  if (per == 0) {
    per = PRED_DRAWS;
    const int64_t fit = (int64_t)(PRED_BUDGET / nb);
    if (per > fit) per = fit;
    if (per < 1) per = 1;
  }
  if (per > S) per = S;

  // every draw starts 256 bytes apart, as the staging vector of
  // bbx_design_dot does: the product kernels take the same path
  const int64_t pitch = (P + 31) / 32 * 32;
  const size_t tstride = (size_t)ORDINAL_TAB * K;
  DevMem d_beta, d_tab, d_eta, d_state, d_out, d_off, d_y;
  BBX_TRY(d_beta.alloc(d8 * (size_t)pitch * (size_t)S));
  BBX_TRY(d_eta.alloc(nb * (size_t)per));
  BBX_TRY(d_state.alloc(nb * (size_t)(2 * K + 4)));
  BBX_TRY(d_out.alloc(nb * (size_t)(2 * K + 3)));
  BBX_TRY(d_tab.alloc(d8 * tstride * (size_t)S));
  BBX_HIP(hipMemcpy2DAsync(d_beta.ptr, d8 * (size_t)pitch, q.coef,
                           d8 * (size_t)P, d8 * (size_t)P, (size_t)S,
                           hipMemcpyHostToDevice, s));
  // (the host arrays below outlive their copies: this function synchronises
  // before it returns)
  std::vector<double> tab(tstride * (size_t)S);
  for (int64_t d = 0; d < S; ++d)
    ordinal_tab(K, q.cuts + d * (K - 1), &tab[(size_t)d * tstride]);
  BBX_HIP(hipMemcpyAsync(d_tab.ptr, tab.data(), d8 * tab.size(),
                         hipMemcpyHostToDevice, s));
  if (q.offset) {
    BBX_TRY(d_off.alloc(nb));
    BBX_HIP(hipMemcpyAsync(d_off.ptr, q.offset, nb, hipMemcpyHostToDevice, s));
  }
  if (score) {
    BBX_TRY(d_y.alloc(nb));
    BBX_HIP(hipMemcpyAsync(d_y.ptr, q.y, nb, hipMemcpyHostToDevice, s));
  }

  OrdinalPredArgs a{};
  a.n = n;
  a.n_draw = S;
  a.K = K;
  a.eta = d_eta.as<const double>();
  a.tab = d_tab.as<const double>();
  a.offset = d_off.as<const double>();
  a.y = d_y.as<const double>();
  a.state = d_state.as<double>();
  a.out = d_out.as<double>();
  const dim3 grid((unsigned)((n + PRED_BLOCK - 1) / PRED_BLOCK),
                  (unsigned)(K + (score ? 1 : 0)));
  for (int64_t k0 = 0; k0 < S; k0 += per) {
    const int kn = (int)(k0 + per < S ? per : S - k0);
    for (int d = 0; d < kn; ++d) {
      const double* b = d_beta.as<const double>() + (k0 + d) * pitch;
      BBX_TRY(launch_prep_v(h, b, nullptr, nullptr, part_slot(h, PS_C)));
      BBX_TRY(launch_dot(h, b, nullptr, d_eta.as<double>() + (int64_t)d * n,
                         nullptr));
    }
    a.k0 = k0;
    a.kn = kn;
    BBX_LAUNCH(ordinal_summary_kernel, grid, dim3(PRED_BLOCK), 0, s, a);
    BBX_HIP(hipGetLastError());
  }
  BBX_HIP(hipMemcpyAsync(q.mean, d_out.ptr, nb * (size_t)K,
                         hipMemcpyDeviceToHost, s));
  BBX_HIP(hipMemcpyAsync(q.sd, d_out.as<double>() + (int64_t)K * n,
                         nb * (size_t)K, hipMemcpyDeviceToHost, s));
  double* outs[3] = {q.lpd, q.ll_mean, q.ll_var};
  for (int r = 0; score && r < 3; ++r)
    BBX_HIP(hipMemcpyAsync(outs[r],
                           d_out.as<double>() + (int64_t)(2 * K + r) * n, nb,
                           hipMemcpyDeviceToHost, s));
  BBX_HIP(hipStreamSynchronize(s));
  return BBX_OK;
}

}  // namespace pred
}  // namespace bbx

using namespace bbx;
using namespace bbx::pred;

extern "C" int bbx_design_predictive_summary_ordinal(
    bbx_design* design, int64_t n_draw, int n_category, const double* coef,
    const double* cutpoints, const double* offset, const double* y,
    int draws_per_pass, double* mean, double* sd, double* lpd, double* ll_mean,
    double* ll_var) {
  const std::string who = "bbx_design_predictive_summary_ordinal: ";
  if (!design || !design_alive(design))
    return fail(BBX_ERR_INVALID, who + "the design is NULL or destroyed");
  if (n_draw < 1)
    return fail(BBX_ERR_INVALID, who + "n_draw must be at least 1");
  if (n_category < 2 || n_category > ORDINAL_MAXCAT)
    return fail(BBX_ERR_INVALID, who + "n_category outside [2, " +
                                     std::to_string(ORDINAL_MAXCAT) + "]");
  if (!coef) return fail(BBX_ERR_INVALID, who + "coef is NULL");
  if (!cutpoints) return fail(BBX_ERR_INVALID, who + "cutpoints is NULL");
  if (!mean) return fail(BBX_ERR_INVALID, who + "mean is NULL");
  if (!sd) return fail(BBX_ERR_INVALID, who + "sd is NULL");
  if (y && (!lpd || !ll_mean || !ll_var))
    return fail(BBX_ERR_INVALID,
                who + "y is given but lpd, ll_mean or ll_var is NULL");
  if (draws_per_pass < 0)
    return fail(BBX_ERR_INVALID, who + "draws_per_pass must not be negative");
  return no_throw([&]() -> int {
    for (int64_t d = 0; d < n_draw; ++d) {
      if (!ordinal_cuts_ok(n_category, cutpoints + d * (n_category - 1)))
        return fail(BBX_ERR_INVALID,
                    who + "cutpoints[" + std::to_string(d) +
                        "] is not finite and strictly increasing");
    }
    for (int64_t i = 0; i < design->n; ++i) {
      if (offset && !std::isfinite(offset[i]))
        return fail(BBX_ERR_INVALID,
                    who + "offset[" + std::to_string(i) + "] is not finite");
      if (y && (!(y[i] >= 0. && y[i] <= (double)(n_category - 1)) ||
                y[i] != floor(y[i])))
        return fail(BBX_ERR_INVALID, who + "y[" + std::to_string(i) +
                                         "] is not a category in [0, " +
                                         std::to_string(n_category - 1) + "]");
    }
    BBX_HIP(hipSetDevice(design->device));
    const OrdinalPredCall q{design, n_draw, n_category, coef,    cutpoints,
                            offset, y,      draws_per_pass, mean, sd,
                            lpd,    ll_mean, ll_var};
    return ordinal_summary_impl(q);
  });
}
