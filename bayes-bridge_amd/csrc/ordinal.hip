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
// Cutpoints: L(c) = sum_i ll_i for up to ORDINAL_MAXC whole cutpoint vectors
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
// policy, and adds the cutpoint sums: a sibling kernel under the same
// contract, in which each of the candidates has its own accumulator, block
// sum and NPART partials, and a row's term for candidate k is computed from
// (eta, y, o) and table k alone: the sum of a given cutpoint vector depends
// neither on the number of candidates nor on its place among them.
#include <math.h>

#include <cmath>
#include <vector>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"
#include "ordinal_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr int ORDINAL_MAXC = 8;   // cutpoint vectors per call

// The cutpoint mode: n_c sums of ll_i in one pass over the rows, on the row
// kernel's partition and in its order of addition.  `ctab`: n_c tables of
// ordinal_tab, ORDINAL_TABLE doubles apart; `part`: n_c x NPART partials,
// candidate-major.  The running sums of a thread live in LDS (one column per
// thread: no bank conflict, no barrier) under a rolled loop over the
// candidates, as in negbin_disp_kernel: the body unrolled eight times holds
// more live values than the register budget of the row kernels.  y is a valid
// category (checked at create): the table index is in range.
static __global__ __launch_bounds__(VEC_BLOCK) void ordinal_cut_kernel(
    int64_t n, int n_c, const double* __restrict__ eta,
    const double2* __restrict__ yo, const double* __restrict__ ctab,
    double* __restrict__ part) {
  __shared__ double s_acc[ORDINAL_MAXC][VEC_BLOCK];
  for (int k = 0; k < n_c; ++k) s_acc[k][threadIdx.x] = 0.;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += GLM_ROW_U * lap) {
    double xo[GLM_ROW_U];
    int cat[GLM_ROW_U];
#pragma unroll
    for (int u = 0; u < GLM_ROW_U; ++u) {
      const int64_t i = i0 + u * lap;
      xo[u] = 0.;
      cat[u] = 0;
      if (i < n) {
        const double2 c = yo[i];
        cat[u] = ORDINAL_TAB * (int)c.x;
        xo[u] = eta[i] + c.y;
      }
    }
#pragma unroll 1
    for (int k = 0; k < n_c; ++k) {
      const double* tab = ctab + k * ORDINAL_TABLE;
      double acc = s_acc[k][threadIdx.x];
#pragma unroll
      for (int u = 0; u < GLM_ROW_U; ++u) {
        if (i0 + u * lap >= n) break;
        const double* t = tab + cat[u];
        acc += ordinal_ll(xo[u], t[0], t[1], t[2]);
      }
      s_acc[k][threadIdx.x] = acc;
    }
  }
  for (int k = 0; k < n_c; ++k) {
    const double sum = block_sum<VEC_BLOCK>(s_acc[k][threadIdx.x]);
    if (threadIdx.x == 0) part[k * NPART + blockIdx.x] = sum;
  }
}

}  // namespace bbx

using namespace bbx;

// One proportional-odds likelihood on a design: rows (y_i, offset_i)
struct bbx_ordinal : GlmRowsCore {
  DevMem tab;        // ORDINAL_TABLE: ordinal_tab of the handle's cutpoints
  DevMem eta_cut;    // n: eta of the last cutpoint call with coefficients
  DevMem cut_part;   // ORDINAL_MAXC x NPART partials of the cutpoint sums
  DevMem cut_tab;    // ORDINAL_MAXC x ORDINAL_TABLE: the call's tables
  int K = 0;
  bool have_eta_cut = false;
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
        const size_t d8 = sizeof(double);
        BBX_TRY(c->tab.alloc(d8 * ORDINAL_TABLE));
        BBX_TRY(c->eta_cut.alloc(d8 * h->n));
        BBX_TRY(c->cut_part.alloc(d8 * ORDINAL_MAXC * NPART));
        return c->cut_tab.alloc(d8 * ORDINAL_MAXC * ORDINAL_TABLE);
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

// L(c_k), k < n_c, at beta (null: the eta of the previous call): the product
// into eta_cut, the candidates' tables up, one launch of the cut kernel, the
// n_c x NPART partials back in one copy and re-added on the host in index
// order.
int cutpoint_loglik_impl(bbx_ordinal* c, const double* beta, int n_c,
                         const double* cuts, double* out) {
  bbx_design* h = c->h;
  if (beta) {
    c->have_eta_cut = false;
    double* d_in = h->stage_P.as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(launch_prep_v(h, d_in, nullptr, nullptr, part_slot(h, PS_C)));
    BBX_TRY(launch_dot(h, d_in, nullptr, c->eta_cut.as<double>(), nullptr));
  }
  double tab[ORDINAL_MAXC * ORDINAL_TABLE] = {};
  for (int k = 0; k < n_c; ++k)
    ordinal_tab(c->K, cuts + (size_t)k * (c->K - 1), tab + k * ORDINAL_TABLE);
  // (tab outlives the copy: this function synchronises before it returns)
  BBX_HIP(hipMemcpyAsync(c->cut_tab.ptr, tab,
                         sizeof(double) * n_c * ORDINAL_TABLE,
                         hipMemcpyHostToDevice, h->stream));
  BBX_LAUNCH(ordinal_cut_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->n, n_c, c->eta_cut.as<const double>(),
             c->pair.as<const double2>(), c->cut_tab.as<const double>(),
             c->cut_part.as<double>());
  BBX_HIP(hipGetLastError());
  std::vector<double> part((size_t)n_c * NPART);
  BBX_HIP(hipMemcpyAsync(part.data(), c->cut_part.ptr,
                         sizeof(double) * part.size(), hipMemcpyDeviceToHost,
                         h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));   // the one synchronisation
  if (beta) c->have_eta_cut = true;
  for (int k = 0; k < n_c; ++k) {
    double sum = 0.;
    for (int b = 0; b < NPART; ++b) sum += part[(size_t)k * NPART + b];
    out[k] = sum;
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
  const char* who = "bbx_ordinal_cutpoint_loglik: ";
  BBX_TRY(ham::check(c, "ordinal"));
  if (!cuts || !out)
    return fail(BBX_ERR_INVALID, std::string(who) + "NULL argument");
  if (n_c < 1 || n_c > ORDINAL_MAXC)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_c outside [1, " +
                                     std::to_string(ORDINAL_MAXC) + "]");
  for (int k = 0; k < n_c; ++k) {
    if (!ordinal_cuts_ok(c->K, cuts + (size_t)k * (c->K - 1)))
      return fail(BBX_ERR_INVALID, std::string(who) + "cuts[" +
                                       std::to_string(k) +
                                       "] is not finite and strictly "
                                       "increasing");
  }
  if (!beta && !c->have_eta_cut)
    return fail(BBX_ERR_STATE, std::string(who) +
                                   "no linear predictor is cached: the first "
                                   "call on a handle needs beta");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return cutpoint_loglik_impl(c, beta, n_c, cuts, out); });
}

BBX_HAM_ENTRY_POINTS(ordinal, GlmFamilyT<OrdinalRows>)
