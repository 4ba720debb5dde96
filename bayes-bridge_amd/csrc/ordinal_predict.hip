// Posterior prediction and pointwise predictive scores of the
// proportional-odds model from draws of the coefficients and of the
// cutpoints: the category probabilities' posterior mean and spread per row
// and, with an outcome, the scores of the row's log-probability.  A kernel of
// its own on the accumulators of predict_summary.hpp (their contract is
// stated there): a row has K probabilities, not one mean, so the state is K
// Moments and one Scores per row, 2 K + 4 values laid out state-major, and the
// launch has one plane of workgroups per category (blockIdx.y = k: the
// Moments of p_k) plus, with an outcome, one for the Scores.  A plane reads
// the pass's linear predictors once; K + 1 planes read them from the cache.
// No thread shares a state with another: no atomics.  The passes are
// PredPasses', as for every family.
//
//   p_k = sigma(c_{k+1} - xo) - sigma(c_k - xo)   (pred_sigma: absolute error
//                                                  ~1e-16, what a mean needs)
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
  double* state;          // [2 K + 4][n]: the Moments of p_k ..., the Scores
  double* out;            // [2 K + 3][n]: PredPasses::finish's layout
};

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
    Moments mom;
    if (a.k0 > 0) mom.load(st, n, i);
    // (the table's entries of a draw are wave-uniform: two draws in flight
    // hold as many scalar registers as the kernel can spare)
#pragma unroll 2
    for (int d = 0; d < a.kn; ++d) {
      double xo = a.eta[(int64_t)d * n + i];
      if (has_off) xo += off;
      const double* t = a.tab + (a.k0 + d) * tstride + ORDINAL_TAB * plane;
      const double p = pred_sigma(t[1] - xo) - pred_sigma(t[0] - xo);
      mom.push(p, (double)(a.k0 + d + 1));
    }
    if (!last) {
      mom.store(st, n, i);
      return;
    }
    mom.finish(S, a.out + (int64_t)plane * n, a.out + (int64_t)(K + plane) * n,
               i);
    return;
  }
  double* st = a.state + (int64_t)(2 * K) * n;
  Scores sc;
  if (a.k0 > 0) sc.load(st, n, i);
  // (a valid category: checked on the host)
  const int cat = ORDINAL_TAB * (int)a.y[i];
#pragma unroll 1
  for (int d = 0; d < a.kn; ++d) {
    double xo = a.eta[(int64_t)d * n + i];
    if (has_off) xo += off;
    const double* t = a.tab + (a.k0 + d) * tstride + cat;
    sc.push(ordinal_ll(xo, t[0], t[1], t[2]), (double)(a.k0 + d + 1));
  }
  if (!last) {
    sc.store(st, n, i);
    return;
  }
  sc.finish(S, a.out + (int64_t)(2 * K) * n, n, i);
}

// res: mean[K][n], sd[K][n], lpd[n], ll_mean[n], ll_var[n] on the host
static int ordinal_summary_impl(bbx_design* h, int64_t S, int K,
                                const double* coef, const double* cuts,
                                const double* offset, const double* y,
                                int draws_per_pass, double* const res[5]) {
  const int64_t n = h->n;
  const size_t d8 = sizeof(double);
  const bool score = y != nullptr;

  PredPasses p;
  const size_t tstride = (size_t)ORDINAL_TAB * K;
  DevMem d_state, d_out;
  BBX_TRY(p.begin(h, S, coef, draws_per_pass));
  BBX_TRY(d_state.alloc(p.nb * (size_t)(2 * K + 4)));
  BBX_TRY(d_out.alloc(p.nb * (size_t)(2 * K + 3)));
  std::vector<double> tab(tstride * (size_t)S);
  for (int64_t d = 0; d < S; ++d)
    ordinal_tab(K, cuts + d * (K - 1), &tab[(size_t)d * tstride]);

  OrdinalPredArgs a{};
  a.n = n;
  a.n_draw = S;
  a.K = K;
  a.eta = p.d_eta.as<const double>();
  BBX_TRY(p.upload(tab.data(), d8 * tab.size(), &a.tab));
  BBX_TRY(p.row(offset, &a.offset));
  BBX_TRY(p.row(y, &a.y));
  a.state = d_state.as<double>();
  a.out = d_out.as<double>();
  const dim3 grid((unsigned)((n + PRED_BLOCK - 1) / PRED_BLOCK),
                  (unsigned)(K + (score ? 1 : 0)));
  BBX_TRY(p.run([&](int64_t k0, int kn) {
    a.k0 = k0;
    a.kn = kn;
    BBX_LAUNCH(ordinal_summary_kernel, grid, dim3(PRED_BLOCK), 0, h->stream,
               a);
  }));
  return p.finish(a.out, K, score, res);
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
    double* const res[5] = {mean, sd, lpd, ll_mean, ll_var};
    return ordinal_summary_impl(design, n_draw, n_category, coef, cutpoints,
                                offset, y, draws_per_pass, res);
  });
}
