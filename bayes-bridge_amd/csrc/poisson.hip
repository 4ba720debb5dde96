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
using ham::read_state;
using ham::with_p_stage;

int poisson_check(const bbx_poisson* c) {
  if (!c) return fail(BBX_ERR_INVALID, "NULL poisson handle");
  if (!design_alive(c->h))
    return fail(BBX_ERR_STATE,
                "the poisson handle's design has been destroyed");
  return BBX_OK;
}

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
  c->h = h;
  c->device = h->device;
  c->n = n;
  c->P = h->P;
  auto cleanup = [&](int st) {
    ham::free_pinned(c);
    delete c;
    return st;
  };
  if (hipSetDevice(h->device) != hipSuccess)
    return cleanup(fail(BBX_ERR_HIP, "hipSetDevice"));
  const size_t d8 = sizeof(double);
  int st = BBX_OK;
  DevMem* nvec[] = {&c->eta, &c->tmp, &c->mu_loc};
  for (DevMem* m : nvec)
    if (st == BBX_OK) st = m->alloc(d8 * n);
  if (st == BBX_OK) st = c->yo.alloc(d8 * 2 * n);
  DevMem* pvec[] = {&c->q, &c->p, &c->p2, &c->g, &c->gl, &c->v, &c->scale, &c->pp};
  for (DevMem* m : pvec)
    if (st == BBX_OK) st = m->alloc(d8 * c->P);
  if (st == BBX_OK) st = c->llpart.alloc(d8 * SCAN_G);
  if (st == BBX_OK) st = c->post.alloc(d8 * 3 * NPART);
  if (st == BBX_OK) st = c->st.alloc(sizeof(CoxTraj));
  if (st != BBX_OK) return cleanup(st);
  if (hipHostMalloc((void**)&c->host_st, sizeof(CoxTraj)) != hipSuccess) {
    c->host_st = nullptr;
    return cleanup(fail(BBX_ERR_HIP, "hipHostMalloc"));
  }
  hipError_t e = hipMemcpyAsync(c->yo.ptr, yo.data(), d8 * 2 * n,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->st.ptr, 0, sizeof(CoxTraj), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return cleanup(fail(BBX_ERR_HIP, std::string("poisson upload: ") +
                                         hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

int poisson_loglik_grad_dev(bbx_poisson* c, const double* d_beta,
                            double* loglik, double* d_grad) {
  bbx_design* h = c->h;
  // a trajectory that stopped early leaves its skip flag set
  BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
  BBX_HIP(hipGetLastError());
  BBX_TRY(eta_of(c, d_beta));
  BBX_TRY(likelihood_from_eta(c, d_grad));
  BBX_LAUNCH(cox_loglik_kernel, dim3(1), dim3(WAVE), 0, h->stream,
             c->llpart.as<const double>(), cst(c));
  BBX_HIP(hipGetLastError());
  BBX_TRY(read_state(c));
  *loglik = c->host_st->logp;
  return BBX_OK;
}

int poisson_hessian_dev(bbx_poisson* c, const double* d_v, double* d_out) {
  if (!c->have_location)
    return fail(BBX_ERR_STATE, "bbx_poisson_set_location has not succeeded");
  bbx_design* h = c->h;
  BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
  BBX_TRY(launch_rows<PM_HESS>(c, c->eta.as<const double>(),
                               c->tmp.as<double>(), nullptr));
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, d_out);
}

}  // namespace

extern "C" {

int bbx_poisson_create(bbx_design* design, const double* y,
                       const double* log_exposure, bbx_poisson** out) {
  return no_throw(
      [&] { return poisson_create_impl(design, y, log_exposure, out); });
}

int bbx_poisson_destroy(bbx_poisson* c) {
  if (!c) return BBX_OK;
  if (design_alive(c->h)) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->h->stream);
  }
  ham::free_pinned(c);
  delete c;
  return BBX_OK;
}

int bbx_poisson_loglik_grad_dev(bbx_poisson* c, const double* d_beta,
                                double* loglik, double* d_grad) {
  BBX_TRY(poisson_check(c));
  if (!d_beta || !loglik) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw(
      [&] { return poisson_loglik_grad_dev(c, d_beta, loglik, d_grad); });
}

int bbx_poisson_loglik_grad(bbx_poisson* c, const double* beta, double* loglik,
                            double* grad) {
  BBX_TRY(poisson_check(c));
  if (!beta || !loglik) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    double ll = 0.;
    BBX_TRY(with_p_stage(c, beta, grad, [&](const double* d_in, double* d_out) {
      return poisson_loglik_grad_dev(c, d_in, &ll, d_out);
    }));
    *loglik = ll;
    return BBX_OK;
  });
}

int bbx_poisson_set_location(bbx_poisson* c, const double* beta) {
  BBX_TRY(poisson_check(c));
  if (!beta) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    bbx_design* h = c->h;
    c->have_location = false;
    double* d_in = h->stage_P.as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(launch_rows<PM_LOC>(c, c->eta.as<const double>(),
                                c->mu_loc.as<double>(), nullptr));
    BBX_HIP(hipStreamSynchronize(h->stream));   // beta is free again
    c->have_location = true;
    return BBX_OK;
  });
}

int bbx_poisson_hessian_matvec_dev(bbx_poisson* c, const double* d_v,
                                   double* d_out) {
  BBX_TRY(poisson_check(c));
  if (!d_v || !d_out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return poisson_hessian_dev(c, d_v, d_out); });
}

int bbx_poisson_hessian_matvec(bbx_poisson* c, const double* v, double* out) {
  BBX_TRY(poisson_check(c));
  if (!v || !out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return with_p_stage(c, v, out, [&](const double* d_in, double* d_out) {
      return poisson_hessian_dev(c, d_in, d_out);
    });
  });
}

int bbx_poisson_hmc_trajectory(bbx_poisson* c, double dt, int n_step,
                               const double* precond_scale,
                               const double* prior_prec, const double* q0,
                               const double* p0, double logp0,
                               const double* grad0, double hamiltonian_tol,
                               double* q, double* p, double* logp,
                               double* grad, int* n_grad_evals,
                               int* instability, double* hamiltonian) {
  BBX_TRY(poisson_check(c));
  if (!precond_scale || !prior_prec || !q0 || !p0 || !grad0)
    return fail(BBX_ERR_INVALID, "NULL argument");
  if (n_step < 0) return fail(BBX_ERR_INVALID, "n_step < 0");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    PoissonLik lik{c};
    return ham::trajectory_impl(c, lik, dt, n_step, precond_scale, prior_prec,
                                q0, p0, logp0, grad0, hamiltonian_tol, q, p,
                                logp, grad, n_grad_evals, instability,
                                hamiltonian);
  });
}

int bbx_poisson_nuts_begin(bbx_poisson* c, const double* precond_scale,
                           const double* prior_prec, const double* q0,
                           const double* p0, double logp0, const double* grad0,
                           double joint_logp0, double joint_logp_threshold,
                           double hamiltonian_tol) {
  BBX_TRY(poisson_check(c));
  if (!precond_scale || !prior_prec || !q0 || !p0 || !grad0)
    return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return ham::nuts_begin_impl(c, precond_scale, prior_prec, q0, p0, logp0,
                                grad0, joint_logp0, joint_logp_threshold,
                                hamiltonian_tol);
  });
}

int bbx_poisson_nuts_doubling(bbx_poisson* c, double dt, int direction,
                              int height, const double* uniforms,
                              int* n_uniform_used, int* n_steps, int* flags,
                              int* tree, double* averages) {
  BBX_TRY(poisson_check(c));
  BBX_TRY(ham::nuts_doubling_args(c, "bbx_poisson", uniforms, direction,
                                  height));
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    PoissonLik lik{c};
    BBX_TRY(ham::nuts_doubling_impl(c, lik, dt, direction, height, uniforms));
    ham::nuts_doubling_out(c, n_uniform_used, n_steps, flags, tree, averages);
    return BBX_OK;
  });
}

int bbx_poisson_nuts_sample(bbx_poisson* c, double* q, double* logp,
                            double* grad) {
  BBX_TRY(poisson_check(c));
  if (!c->nuts_begun)
    return fail(BBX_ERR_STATE, "bbx_poisson_nuts_begin has not succeeded");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return ham::nuts_sample_impl(c, q, logp, grad); });
}

}  // extern "C"
