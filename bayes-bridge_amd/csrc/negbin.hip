// Negative-binomial likelihood with a log link, an exposure offset and a
// dispersion ("size") r for the Hamiltonian coefficient samplers: its
// gradient, its Hessian-vector product at a fixed location, the trajectory /
// No-U-Turn drivers of hamiltonian.hpp with this family's block between "eta
// is complete" and "grad_loglik is complete", and the reduction the
// dispersion's own update needs.
//
// Counts y >= 0 with mean mu = exp(eta + o), eta = X~ beta, o = log(exposure),
// and variance mu + mu^2 / r.  With theta = log r and t = (eta + o) - theta,
// per row (negbin_terms.hpp):
//   ll_i    = y t - (y + r) softplus(t)   (G(y, r) - log y! is constant in
//                                          beta: dropped here)
//   w_i     = y - (y + r) sigma(t),  grad = X~^T w
//   omega_i = (y + r) (sigma(t) (1 - sigma(t)))
// Hessian-vector product at a fixed location: u = X~ v, out = X~^T (-(omega u))
// Dispersion: L(r) = sum_i G(y_i, r) + y_i t_i - (y_i + r) softplus(t_i) for
// up to NEGBIN_MAXR values of r in one pass over the rows.
//
// No overflow: the only exp is exp(-|t|) <= 1, so ll_i, w_i and omega_i are
// finite for every finite t; there is no mu = exp(eta) as in poisson.hip.  An
// infinite eta gives ll_i = -inf (t = -inf with y > 0, t = +inf with y = 0)
// or NaN.  The test that raises CoxTraj::zero (and skip) is ll_i == -inf.
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the three expressions above on rows (y_i, o_i), with the
// handle's r and log r in the policy, and adds the dispersion sums: a sibling
// kernel under the same contract, in which each of the K values has its own
// accumulator, block sum and NPART partials, and a row's term for r_k is
// computed from (eta, y, o, r_k, log r_k) alone: the sum for a given r depends
// neither on K nor on its place among the K values.
#include <math.h>

#include <cmath>
#include <vector>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"
#include "negbin_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr int NEGBIN_MAXR = 8;   // values of r per dispersion call

// GLM_ROW_U under the name it had in this file.  Nothing in this tree reads
// it; the previous revision's tests/test_hip_negbin.py does, at import, and
// a module that fails to import stops that revision's whole suite when it is
// run over this build.  To be deleted with the next change to this file.
constexpr int NEGBIN_U = 4;
static_assert(NEGBIN_U == GLM_ROW_U, "the row kernels are glm_rows.hpp's");

// The dispersion mode: K sums of G(y, r_k) + y t - (y + r_k) softplus(t) in
// one pass over the rows, on the row kernel's partition and in its order of
// addition.  `gtab`: K tables of negbin_gtab; `part`: K x NPART partials,
// value-major.  The K running sums of a thread live in LDS (one column per
// thread: no bank conflict, no barrier), so that the loop over k is a loop and
// K a number: the K = 8 body unrolled holds more wave-uniform values (r_k,
// log r_k, the table's tail and the polynomial coefficients of exp, log1p and
// log) than there are scalar registers.  A row's term for r_k is a function
// of (eta, y, o) and table k alone.
static __global__ __launch_bounds__(VEC_BLOCK) void negbin_disp_kernel(
    int64_t n, int K, const double* __restrict__ eta,
    const double2* __restrict__ yo, const double* __restrict__ gtab,
    double* __restrict__ part) {
  __shared__ double s_acc[NEGBIN_MAXR][VEC_BLOCK];
  for (int k = 0; k < K; ++k) s_acc[k][threadIdx.x] = 0.;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += GLM_ROW_U * lap) {
    double a_o[GLM_ROW_U], y[GLM_ROW_U];
#pragma unroll
    for (int u = 0; u < GLM_ROW_U; ++u) {
      const int64_t i = i0 + u * lap;
      a_o[u] = y[u] = 0.;
      if (i < n) {
        const double2 c = yo[i];
        y[u] = c.x;
        a_o[u] = eta[i] + c.y;
      }
    }
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      const double* tab = gtab + k * NEGBIN_GTAB;
      const double r = tab[NEGBIN_TAB_R], logr = tab[NEGBIN_TAB_R + 1];
      double acc = s_acc[k][threadIdx.x];
#pragma unroll
      for (int u = 0; u < GLM_ROW_U; ++u) {
        if (i0 + u * lap >= n) break;
        const double tk = a_o[u] - logr;
        double sp, sg;
        negbin_link(tk, &sp, &sg);
        acc += negbin_G(y[u], r, tab) + negbin_beta_part(y[u], r, tk, sp);
      }
      s_acc[k][threadIdx.x] = acc;
    }
  }
  for (int k = 0; k < K; ++k) {
    const double sum = block_sum<VEC_BLOCK>(s_acc[k][threadIdx.x]);
    if (threadIdx.x == 0) part[k * NPART + blockIdx.x] = sum;
  }
}

}  // namespace bbx

using namespace bbx;

// One negative-binomial likelihood on a design: rows (y_i, log exposure_i)
struct bbx_negbin : GlmRowsCore {
  DevMem eta_disp;    // n: eta of the last dispersion call with coefficients
  DevMem disp_part;   // NEGBIN_MAXR x NPART partials of the dispersion sums
  DevMem disp_tab;    // NEGBIN_MAXR x NEGBIN_GTAB: negbin_gtab of the call's r
  double r = 1., logr = 0.;
  bool have_eta_disp = false;
};

namespace {

// the handle's r and log r, by value in the kernel's arguments
struct NegBinRows {
  using Handle = bbx_negbin;
  static constexpr const char* name = "negbin";
  static constexpr bool raises = true;
  double r, logr;
  static NegBinRows make(const bbx_negbin* c) {
    return NegBinRows{c->r, c->logr};
  }
  __device__ double loc(double x, double y, double o) const {
    const double tt = (x + o) - logr;
    double sp, sg;
    negbin_link(tt, &sp, &sg);
    return (y + r) * (sg * (1. - sg));
  }
  __device__ bool grad(double x, double y, double o, double& w,
                       double& l) const {
    const double tt = (x + o) - logr;
    double sp, sg;
    negbin_link(tt, &sp, &sg);
    w = y - (y + r) * sg;
    l = negbin_beta_part(y, r, tt, sp);
    return l == -INFINITY;
  }
};

bool finite_positive(double r) { return std::isfinite(r) && r > 0.; }

int negbin_create_impl(bbx_design* h, const double* y,
                       const double* log_exposure, double dispersion,
                       bbx_negbin** out) {
  BBX_TRY(glm_create_head(h, y != nullptr, out));
  if (!finite_positive(dispersion))
    return fail(BBX_ERR_INVALID, "the dispersion is not finite and positive");
  return glm_create_rows(
      h, "negbin", y, log_exposure, glm_count_row,
      [&](bbx_negbin* c) {
        c->r = dispersion;
        c->logr = log(dispersion);
        const size_t d8 = sizeof(double);
        BBX_TRY(c->eta_disp.alloc(d8 * h->n));
        BBX_TRY(c->disp_part.alloc(d8 * NEGBIN_MAXR * NPART));
        return c->disp_tab.alloc(d8 * NEGBIN_MAXR * NEGBIN_GTAB);
      },
      out);
}

// L(r_k), k < n_r, at beta (null: the eta of the previous call): the product
// into eta_disp, the tables of G up, one launch of the row kernel, the
// K x NPART partials back in one copy and re-added on the host in index order.
int dispersion_loglik_impl(bbx_negbin* c, const double* beta, int n_r,
                           const double* r, double* out) {
  bbx_design* h = c->h;
  if (beta) {
    c->have_eta_disp = false;
    double* d_in = h->stage_P.as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(launch_prep_v(h, d_in, nullptr, nullptr, part_slot(h, PS_C)));
    BBX_TRY(launch_dot(h, d_in, nullptr, c->eta_disp.as<double>(), nullptr));
  }
  double tab[NEGBIN_MAXR * NEGBIN_GTAB];
  for (int k = 0; k < n_r; ++k) negbin_gtab(r[k], tab + k * NEGBIN_GTAB);
  // (tab outlives the copy: this function synchronises before it returns)
  BBX_HIP(hipMemcpyAsync(c->disp_tab.ptr, tab,
                         sizeof(double) * n_r * NEGBIN_GTAB,
                         hipMemcpyHostToDevice, h->stream));
  BBX_LAUNCH(negbin_disp_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->n, n_r, c->eta_disp.as<const double>(),
             c->pair.as<const double2>(), c->disp_tab.as<const double>(),
             c->disp_part.as<double>());
  BBX_HIP(hipGetLastError());
  std::vector<double> part((size_t)n_r * NPART);
  BBX_HIP(hipMemcpyAsync(part.data(), c->disp_part.ptr,
                         sizeof(double) * part.size(), hipMemcpyDeviceToHost,
                         h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));   // the one synchronisation
  if (beta) c->have_eta_disp = true;
  for (int k = 0; k < n_r; ++k) {
    double sum = 0.;
    for (int b = 0; b < NPART; ++b) sum += part[(size_t)k * NPART + b];
    out[k] = sum;
  }
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_negbin_create(bbx_design* design, const double* y,
                                 const double* log_exposure, double dispersion,
                                 bbx_negbin** out) {
  return no_throw([&] {
    return negbin_create_impl(design, y, log_exposure, dispersion, out);
  });
}

extern "C" int bbx_negbin_set_dispersion(bbx_negbin* c, double r) {
  BBX_TRY(ham::check(c, "negbin"));
  if (!finite_positive(r))
    return fail(BBX_ERR_INVALID,
                "bbx_negbin_set_dispersion: the dispersion is not finite and "
                "positive");
  if (c->nuts_open)
    return fail(BBX_ERR_STATE,
                "bbx_negbin_set_dispersion: a No-U-Turn tree is installed on "
                "the handle (bbx_negbin_nuts_begin); take its sample "
                "(bbx_negbin_nuts_sample) first");
  c->r = r;
  c->logr = log(r);
  c->have_location = false;   // omega was formed with the previous r
  return BBX_OK;
}

extern "C" int bbx_negbin_dispersion_loglik(bbx_negbin* c, const double* beta,
                                            int n_r, const double* r,
                                            double* out) {
  const char* who = "bbx_negbin_dispersion_loglik: ";
  BBX_TRY(ham::check(c, "negbin"));
  if (!r || !out) return fail(BBX_ERR_INVALID, std::string(who) + "NULL argument");
  if (n_r < 1 || n_r > NEGBIN_MAXR)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_r outside [1, " +
                                     std::to_string(NEGBIN_MAXR) + "]");
  for (int k = 0; k < n_r; ++k) {
    if (!finite_positive(r[k]))
      return fail(BBX_ERR_INVALID, std::string(who) + "r[" +
                                       std::to_string(k) +
                                       "] is not finite and positive");
  }
  if (!beta && !c->have_eta_disp)
    return fail(BBX_ERR_STATE, std::string(who) +
                                   "no linear predictor is cached: the first "
                                   "call on a handle needs beta");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return dispersion_loglik_impl(c, beta, n_r, r, out); });
}

BBX_HAM_ENTRY_POINTS(negbin, GlmFamilyT<NegBinRows>)
