// Poisson (incidence-rate) likelihood with a log link and an exposure offset
// for the Hamiltonian coefficient samplers: its gradient, its Hessian-vector
// product at a fixed location, and the trajectory / No-U-Turn drivers of
// hamiltonian.hpp with this family's block between "eta is complete" and
// "grad_loglik is complete".
//
// With eta = X~ beta, count y >= 0 and offset o = log(exposure), per row:
//   mu_i = exp(eta_i + o_i)
//   ll_i = y eta - mu          (sum y o - log y! is constant in beta: dropped)
//   w_i  = y - mu,  grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v, out = X~^T (-(mu u))
//
// One row kernel does all three, under the contract of logit.hip: its
// reductions (sum ll, sum w) are block sums in a fixed order into NPART
// partials over a FIXED partition -- row i belongs to workgroup
// (i / VEC_BLOCK) % NPART -- re-added in a fixed order by their consumers: no
// float atomics, the same inputs give the same bits on every run.  A thread
// keeps POISSON_U rows of consecutive laps in flight (their loads are issued
// before the first exp), and y, o are stored interleaved so that a row's pair
// is one 16-byte load; the rows are still added in lap order, so the partials
// do not depend on POISSON_U.
//
// Overflow: where eta + o is past exp's range, mu = inf and ll_i = -inf.  The
// gradient mode then also raises CoxTraj::zero (and skip), as the Cox scan
// does for an empty risk-set sum: the log-likelihood reads -inf whatever the
// other rows hold, the trajectory's instability rule fires at this step and a
// half-tree ends here, with no step taken from a gradient that does not
// exist.  A NaN raises no flag: it comes out of the sums as a NaN.
#include <math.h>

#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

static_assert(SCAN_G == NPART, "the row kernel writes one loglik partial per "
                               "workgroup into HamCore::llpart");

constexpr int POISSON_U = 4;   // rows in flight per thread

enum PoissonMode {
  PM_GRAD = 0,   // w = y - mu, partials of sum ll and of sum w
  PM_LOC = 1,    // mu
  PM_HESS = 2    // w = -(mu u), partials of sum w
};

// `a`: eta (PM_GRAD, PM_LOC) or u = X~ v (PM_HESS); `yo`: (y_i, o_i) pairs
// (PM_LOC: o only); `mu`: the location's mu (PM_HESS); `out`: w or mu.
template <int MODE>
static __global__ __launch_bounds__(VEC_BLOCK) void poisson_row_kernel(
    int64_t n, const double* __restrict__ a, const double2* __restrict__ yo,
    const double* __restrict__ mu, double* __restrict__ out,
    double* __restrict__ llpart, double* __restrict__ sumw_part, CoxTraj* st,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  double acc = 0., ll = 0.;
  bool over = false;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += POISSON_U * lap) {
    double x[POISSON_U], s[POISSON_U], t[POISSON_U];
#pragma unroll
    for (int k = 0; k < POISSON_U; ++k) {
      const int64_t i = i0 + k * lap;
      x[k] = s[k] = t[k] = 0.;
      if (i < n) {
        x[k] = a[i];
        if (MODE == PM_HESS) {
          s[k] = mu[i];
        } else {
          const double2 c = yo[i];
          s[k] = c.x;
          t[k] = c.y;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < POISSON_U; ++k) {
      const int64_t i = i0 + k * lap;
      if (i >= n) break;
      double v;
      if (MODE == PM_HESS) {
        v = -(s[k] * x[k]);
      } else {
        const double m = exp(x[k] + t[k]);
        if (MODE == PM_LOC) {
          v = m;
        } else {
          v = s[k] - m;
          ll += s[k] * x[k] - m;
          over |= (m == INFINITY);
        }
      }
      out[i] = v;
      acc += v;
    }
  }
  if (MODE == PM_LOC) return;
  acc = block_sum<VEC_BLOCK>(acc);
  if (MODE == PM_GRAD) {
    ll = block_sum<VEC_BLOCK>(ll);
    // `skip` points at st->skip: a workgroup that starts after this store
    // returns at entry and leaves its partials stale.  They are never read:
    // every consumer (cox_loglik_kernel, post_b, the leaf kernel) looks at
    // st->zero first, as after cox_scan_sum_kernel<SM_INVH>.
    if (over) {
      st->zero = 1;
      st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    sumw_part[blockIdx.x] = acc;
    if (MODE == PM_GRAD) llpart[blockIdx.x] = ll;
  }
}

}  // namespace bbx

using namespace bbx;

// One Poisson likelihood on a design (borrowed: the design must outlive it).
struct bbx_poisson : HamCore {
  DevMem yo;       // 2 n: (y_i, log exposure_i)
  DevMem mu_loc;   // n: the Hessian's location
};

namespace {

using ham::cst;
using ham::eta_of;

template <int MODE>
int launch_rows(bbx_poisson* c, const double* a, double* out, const int* skip) {
  bbx_design* h = c->h;
  BBX_LAUNCH(poisson_row_kernel<MODE>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, a, c->yo.as<const double2>(),
             c->mu_loc.as<const double>(), out, c->llpart.as<double>(),
             part_slot(h, PS_SUMW), cst(c), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// From eta (in c->eta, complete in stream order): w, the loglik partials and
// (grad != null) grad = X~^T w.
int likelihood_from_eta(bbx_poisson* c, double* grad) {
  bbx_design* h = c->h;
  BBX_TRY(launch_rows<PM_GRAD>(c, c->eta.as<const double>(),
                               c->tmp.as<double>(), &cst(c)->skip));
  if (!grad) return BBX_OK;
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, grad);
}

// The Poisson block of a leapfrog step
struct PoissonLik {
  bbx_poisson* c;
  int operator()(double* grad) const { return likelihood_from_eta(c, grad); }
};

int poisson_create_impl(bbx_design* h, const double* y,
                        const double* log_exposure, bbx_poisson** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!y) return fail(BBX_ERR_INVALID, "NULL count array");
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
  bbx_poisson* c = new bbx_poisson;
  const size_t d8 = sizeof(double);
  int st = ham::init_core(c, h, "poisson");
  if (st == BBX_OK) st = c->mu_loc.alloc(d8 * n);
  if (st == BBX_OK) st = c->yo.alloc(d8 * 2 * n);
  if (st != BBX_OK) return ham::discard(c, st);
  hipError_t e = hipMemcpyAsync(c->yo.ptr, yo.data(), d8 * 2 * n,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("poisson upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

struct PoissonFamily {
  static constexpr const char* name = "poisson";
  using Lik = PoissonLik;
  static int locate(bbx_poisson* c, const double* d_in) {
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(launch_rows<PM_LOC>(c, c->eta.as<const double>(),
                                c->mu_loc.as<double>(), nullptr));
    BBX_HIP(hipStreamSynchronize(c->h->stream));   // beta is free again
    return BBX_OK;
  }
  static int hessian_from_v(bbx_poisson* c, const double* d_v, double* d_out) {
    bbx_design* h = c->h;
    BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
    BBX_TRY(launch_rows<PM_HESS>(c, c->eta.as<const double>(),
                                 c->tmp.as<double>(), nullptr));
    TdotEpilogue ep;
    return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, d_out);
  }
};

}  // namespace

extern "C" int bbx_poisson_create(bbx_design* design, const double* y,
                                  const double* log_exposure,
                                  bbx_poisson** out) {
  return no_throw(
      [&] { return poisson_create_impl(design, y, log_exposure, out); });
}

BBX_HAM_ENTRY_POINTS(poisson, PoissonFamily)
