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
// or NaN.  For -inf the gradient mode raises CoxTraj::zero (and skip) as
// poisson.hip does for an overflow: the log-likelihood reads -inf, the
// trajectory's instability rule fires at this step and a half-tree ends here.
// A NaN raises no flag: it comes out of the sums as a NaN.
//
// One row kernel does the first three and a sibling the dispersion sums, under
// the contract of logit.hip and
// poisson.hip: its reductions are block sums in a fixed order into NPART
// partials over a FIXED partition -- row i belongs to workgroup
// (i / VEC_BLOCK) % NPART -- re-added in a fixed order by their consumers: no
// float atomics, the same inputs give the same bits on every run.  A thread
// keeps NEGBIN_U rows of consecutive laps in flight (their loads are issued
// before the first exp), and y, o are stored interleaved so that a row's pair
// is one 16-byte load; the rows are still added in lap order, so the partials
// do not depend on NEGBIN_U.  In the dispersion mode each of the K values has
// its own accumulator, block sum and NPART partials, and a row's term for r_k
// is computed from (eta, y, o, r_k, log r_k) alone: the sum for a given r
// depends neither on K nor on its place among the K values.
#include <math.h>

#include <cmath>
#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"
#include "negbin_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

static_assert(SCAN_G == NPART, "the row kernel writes one loglik partial per "
                               "workgroup into HamCore::llpart");

constexpr int NEGBIN_U = 4;      // rows in flight per thread
constexpr int NEGBIN_MAXR = 8;   // values of r per dispersion call

enum NegBinMode {
  NB_GRAD = 0,   // w = y - (y + r) sigma, partials of sum ll and of sum w
  NB_LOC = 1,    // omega
  NB_HESS = 2    // w = -(omega u), partials of sum w
};

// the handle's r, by value in the kernel's arguments
struct NegBinR {
  double r, logr;
};

// `a`: eta (NB_GRAD, NB_LOC) or u = X~ v (NB_HESS); `yo`: (y_i, o_i) pairs;
// `om`: the location's omega (NB_HESS); `out`: w or omega; `rr`: r and log r
// (NB_GRAD, NB_LOC).
template <int MODE>
static __global__ __launch_bounds__(VEC_BLOCK) void negbin_row_kernel(
    int64_t n, const double* __restrict__ a, const double2* __restrict__ yo,
    const double* __restrict__ om, double* __restrict__ out, NegBinR rr,
    double* __restrict__ llpart, double* __restrict__ sumw_part, CoxTraj* st,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  double acc = 0., ll = 0.;
  bool over = false;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += NEGBIN_U * lap) {
    double x[NEGBIN_U], s[NEGBIN_U], t[NEGBIN_U];
#pragma unroll
    for (int u = 0; u < NEGBIN_U; ++u) {
      const int64_t i = i0 + u * lap;
      x[u] = s[u] = t[u] = 0.;
      if (i < n) {
        x[u] = a[i];
        if (MODE == NB_HESS) {
          s[u] = om[i];
        } else {
          const double2 c = yo[i];
          s[u] = c.x;
          t[u] = c.y;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NEGBIN_U; ++u) {
      const int64_t i = i0 + u * lap;
      if (i >= n) break;
      double v;
      if (MODE == NB_HESS) {
        v = -(s[u] * x[u]);
      } else {
        const double y = s[u], r = rr.r;
        const double tt = (x[u] + t[u]) - rr.logr;
        double sp, sg;
        negbin_link(tt, &sp, &sg);
        if (MODE == NB_LOC) {
          v = (y + r) * (sg * (1. - sg));
        } else {
          v = y - (y + r) * sg;
          const double l = negbin_beta_part(y, r, tt, sp);
          ll += l;
          over |= (l == -INFINITY);
        }
      }
      out[i] = v;
      acc += v;
    }
  }
  if (MODE == NB_LOC) return;
  acc = block_sum<VEC_BLOCK>(acc);
  if (MODE == NB_GRAD) {
    ll = block_sum<VEC_BLOCK>(ll);
    // `skip` points at st->skip: a workgroup that starts after this store
    // returns at entry and leaves its partials stale.  They are never read:
    // every consumer (cox_loglik_kernel, post_b, the leaf kernel) looks at
    // st->zero first, as after poisson_row_kernel.
    if (over) {
      st->zero = 1;
      st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    sumw_part[blockIdx.x] = acc;
    if (MODE == NB_GRAD) llpart[blockIdx.x] = ll;
  }
}

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
       i0 += NEGBIN_U * lap) {
    double a_o[NEGBIN_U], y[NEGBIN_U];
#pragma unroll
    for (int u = 0; u < NEGBIN_U; ++u) {
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
      for (int u = 0; u < NEGBIN_U; ++u) {
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

// One negative-binomial likelihood on a design (borrowed: the design must
// outlive it).
struct bbx_negbin : HamCore {
  DevMem yo;          // 2 n: (y_i, log exposure_i)
  DevMem omega_loc;   // n: the Hessian's location
  DevMem eta_disp;    // n: eta of the last dispersion call with coefficients
  DevMem disp_part;   // NEGBIN_MAXR x NPART partials of the dispersion sums
  DevMem disp_tab;    // NEGBIN_MAXR x NEGBIN_GTAB: negbin_gtab of the call's r
  double r = 1., logr = 0.;
  bool have_eta_disp = false;
};

namespace {

using ham::cst;
using ham::eta_of;

NegBinR own_r(const bbx_negbin* c) {
  return NegBinR{c->r, c->logr};
}

template <int MODE>
int launch_rows(bbx_negbin* c, const double* a, double* out, const int* skip) {
  bbx_design* h = c->h;
  BBX_LAUNCH(negbin_row_kernel<MODE>, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream, c->n, a,
             c->yo.as<const double2>(), c->omega_loc.as<const double>(), out,
             own_r(c), c->llpart.as<double>(), part_slot(h, PS_SUMW), cst(c),
             skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// From eta (in c->eta, complete in stream order): w, the loglik partials and
// (grad != null) grad = X~^T w.
int likelihood_from_eta(bbx_negbin* c, double* grad) {
  bbx_design* h = c->h;
  BBX_TRY(launch_rows<NB_GRAD>(c, c->eta.as<const double>(),
                               c->tmp.as<double>(), &cst(c)->skip));
  if (!grad) return BBX_OK;
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, grad);
}

// The negative-binomial block of a leapfrog step
struct NegBinLik {
  bbx_negbin* c;
  int operator()(double* grad) const { return likelihood_from_eta(c, grad); }
};

bool finite_positive(double r) { return std::isfinite(r) && r > 0.; }

int negbin_create_impl(bbx_design* h, const double* y,
                       const double* log_exposure, double dispersion,
                       bbx_negbin** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!y) return fail(BBX_ERR_INVALID, "NULL count array");
  if (!finite_positive(dispersion))
    return fail(BBX_ERR_INVALID, "the dispersion is not finite and positive");
  const int64_t n = h->n;
  std::vector<double> yo((size_t)2 * n);
  for (int64_t i = 0; i < n; ++i) {
    const double yi = y[i], oi = log_exposure ? log_exposure[i] : 0.;
    if (!std::isfinite(yi))
      return fail(BBX_ERR_INVALID, "y[" + std::to_string(i) + "] is not finite");
    if (yi < 0.)
      return fail(BBX_ERR_INVALID, "y[" + std::to_string(i) + "] is negative");
    if (!std::isfinite(oi))
      return fail(BBX_ERR_INVALID,
                  "log_exposure[" + std::to_string(i) + "] is not finite");
    yo[2 * i] = yi;
    yo[2 * i + 1] = oi;
  }
  bbx_negbin* c = new bbx_negbin;
  c->r = dispersion;
  c->logr = log(dispersion);
  const size_t d8 = sizeof(double);
  int st = ham::init_core(c, h, "negbin");
  if (st == BBX_OK) st = c->omega_loc.alloc(d8 * n);
  if (st == BBX_OK) st = c->eta_disp.alloc(d8 * n);
  if (st == BBX_OK) st = c->disp_part.alloc(d8 * NEGBIN_MAXR * NPART);
  if (st == BBX_OK) st = c->disp_tab.alloc(d8 * NEGBIN_MAXR * NEGBIN_GTAB);
  if (st == BBX_OK) st = c->yo.alloc(d8 * 2 * n);
  if (st != BBX_OK) return ham::discard(c, st);
  hipError_t e = hipMemcpyAsync(c->yo.ptr, yo.data(), d8 * 2 * n,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("negbin upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

struct NegBinFamily {
  static constexpr const char* name = "negbin";
  using Lik = NegBinLik;
  static int locate(bbx_negbin* c, const double* d_in) {
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(launch_rows<NB_LOC>(c, c->eta.as<const double>(),
                                c->omega_loc.as<double>(), nullptr));
    BBX_HIP(hipStreamSynchronize(c->h->stream));   // beta is free again
    return BBX_OK;
  }
  static int hessian_from_v(bbx_negbin* c, const double* d_v, double* d_out) {
    bbx_design* h = c->h;
    BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
    BBX_TRY(launch_rows<NB_HESS>(c, c->eta.as<const double>(),
                                 c->tmp.as<double>(), nullptr));
    TdotEpilogue ep;
    return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, d_out);
  }
};

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
             c->yo.as<const double2>(), c->disp_tab.as<const double>(),
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

BBX_HAM_ENTRY_POINTS(negbin, NegBinFamily)
