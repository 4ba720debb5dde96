// Binomial-logit likelihood (model/logistic_model.py:49-74) for the
// Hamiltonian coefficient samplers: its gradient, its Hessian-vector product
// at a fixed location, and the trajectory / No-U-Turn drivers of
// hamiltonian.hpp with this family's block between "eta is complete" and
// "grad_loglik is complete".
//
// With eta = X~ beta, y = n_success, m = n_trial, per row:
//   ll_i = y eta - m logaddexp(0, eta)        (NumPy's branch form)
//   p_i  = 1 / (1 + exp(-eta)),  w_i = y - m p_i,  grad = X~^T w
// Hessian-vector product at a fixed location: d_i = m (p_i (1 - p_i)),
//   u = X~ v,  out = X~^T (-(d u))           (= -X~^T (m weight (X~ v)))
//
// One row kernel does all three.  Its reductions (sum ll, sum w) are block
// sums in a fixed order into NPART partials over a FIXED partition -- row i
// belongs to workgroup (i / VEC_BLOCK) % NPART, as in cox_weight_kernel --
// re-added in a fixed order by their consumers: no float atomics, the same
// inputs give the same bits on every run.  A thread keeps LOGIT_U rows of
// consecutive laps in flight (their loads are issued before the first exp),
// and y, m are stored interleaved so that a row's counts are one 16-byte
// load; the rows are still added in lap order, so the partials do not depend
// on LOGIT_U.
#include <math.h>

#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

static_assert(SCAN_G == NPART, "the row kernel writes one loglik partial per "
                               "workgroup into HamCore::llpart");

constexpr int LOGIT_U = 4;   // rows in flight per thread

enum LogitMode {
  LM_GRAD = 0,   // w = y - m p, partials of sum ll and of sum w
  LM_LOC = 1,    // d = m (p (1 - p))
  LM_HESS = 2    // w = -(d u), partials of sum w
};

// npy_logaddexp(0, x): x == 0 -> log 2; x < 0 -> log1p(exp(x)); else
// x + log1p(exp(-x)); NaN -> NaN
__device__ inline double logaddexp0(double x) {
  if (x == 0.) return M_LN2;
  return x > 0. ? x + log1p(exp(-x)) : log1p(exp(x));
}

// `a`: eta (LM_GRAD, LM_LOC) or u = X~ v (LM_HESS); `ym`: (y_i, m_i) pairs
// (LM_GRAD, LM_LOC: m only); `d`: the location's d (LM_HESS); `out`: w or d.
template <int MODE>
static __global__ __launch_bounds__(VEC_BLOCK) void logit_row_kernel(
    int64_t n, const double* __restrict__ a, const double2* __restrict__ ym,
    const double* __restrict__ d, double* __restrict__ out,
    double* __restrict__ llpart, double* __restrict__ sumw_part,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  double acc = 0., ll = 0.;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += LOGIT_U * lap) {
    double x[LOGIT_U], s[LOGIT_U], t[LOGIT_U];
#pragma unroll
    for (int k = 0; k < LOGIT_U; ++k) {
      const int64_t i = i0 + k * lap;
      x[k] = s[k] = t[k] = 0.;
      if (i < n) {
        x[k] = a[i];
        if (MODE == LM_HESS) {
          s[k] = d[i];
        } else {
          const double2 c = ym[i];
          s[k] = c.x;
          t[k] = c.y;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LOGIT_U; ++k) {
      const int64_t i = i0 + k * lap;
      if (i >= n) break;
      double v;
      if (MODE == LM_HESS) {
        v = -(s[k] * x[k]);
      } else {
        const double p = 1. / (1. + exp(-x[k]));
        if (MODE == LM_LOC) {
          v = t[k] * (p * (1. - p));
        } else {
          v = s[k] - t[k] * p;
          ll += s[k] * x[k] - t[k] * logaddexp0(x[k]);
        }
      }
      out[i] = v;
      acc += v;
    }
  }
  if (MODE == LM_LOC) return;
  acc = block_sum<VEC_BLOCK>(acc);
  if (MODE == LM_GRAD) ll = block_sum<VEC_BLOCK>(ll);
  if (threadIdx.x == 0) {
    sumw_part[blockIdx.x] = acc;
    if (MODE == LM_GRAD) llpart[blockIdx.x] = ll;
  }
}

}  // namespace bbx

using namespace bbx;

// One logit likelihood on a design (borrowed: the design must outlive it).
struct bbx_logit : HamCore {
  DevMem ym;      // 2 n: (n_success_i, n_trial_i)
  DevMem d_loc;   // n: the Hessian's location
};

namespace {

using ham::cst;
using ham::eta_of;
using ham::read_state;
using ham::with_p_stage;

int logit_check(const bbx_logit* c) {
  if (!c) return fail(BBX_ERR_INVALID, "NULL logit handle");
  if (!design_alive(c->h))
    return fail(BBX_ERR_STATE, "the logit handle's design has been destroyed");
  return BBX_OK;
}

template <int MODE>
int launch_rows(bbx_logit* c, const double* a, double* out, const int* skip) {
  bbx_design* h = c->h;
  BBX_LAUNCH(logit_row_kernel<MODE>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, a, c->ym.as<const double2>(),
             c->d_loc.as<const double>(), out, c->llpart.as<double>(),
             part_slot(h, PS_SUMW), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// From eta (in c->eta, complete in stream order): w, the loglik partials and
// (grad != null) grad = X~^T w.
int likelihood_from_eta(bbx_logit* c, double* grad) {
  bbx_design* h = c->h;
  BBX_TRY(launch_rows<LM_GRAD>(c, c->eta.as<const double>(),
                               c->tmp.as<double>(), &cst(c)->skip));
  if (!grad) return BBX_OK;
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, grad);
}

// The logit block of a leapfrog step
struct LogitLik {
  bbx_logit* c;
  int operator()(double* grad) const { return likelihood_from_eta(c, grad); }
};

int logit_create_impl(bbx_design* h, const double* n_success,
                      const double* n_trial, bbx_logit** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!n_success || !n_trial)
    return fail(BBX_ERR_INVALID, "NULL count array");
  const int64_t n = h->n;
  std::vector<double> ym((size_t)2 * n);
  for (int64_t i = 0; i < n; ++i) {
    const double y = n_success[i], m = n_trial[i];
    if (!std::isfinite(y) || !std::isfinite(m))
      return fail(BBX_ERR_INVALID,
                  "row " + std::to_string(i) + ": a count is not finite");
    if (y < 0.)
      return fail(BBX_ERR_INVALID,
                  "n_success[" + std::to_string(i) + "] is negative");
    if (m <= 0.)
      return fail(BBX_ERR_INVALID,
                  "n_trial[" + std::to_string(i) + "] is not positive");
    if (y > m)
      return fail(BBX_ERR_INVALID, "n_success[" + std::to_string(i) +
                                       "] exceeds n_trial");
    ym[2 * i] = y;
    ym[2 * i + 1] = m;
  }
  bbx_logit* c = new bbx_logit;
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
  DevMem* nvec[] = {&c->eta, &c->tmp, &c->d_loc};
  for (DevMem* m : nvec)
    if (st == BBX_OK) st = m->alloc(d8 * n);
  if (st == BBX_OK) st = c->ym.alloc(d8 * 2 * n);
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
  hipError_t e = hipMemcpyAsync(c->ym.ptr, ym.data(), d8 * 2 * n,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->st.ptr, 0, sizeof(CoxTraj), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return cleanup(fail(BBX_ERR_HIP, std::string("logit upload: ") +
                                         hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

int logit_loglik_grad_dev(bbx_logit* c, const double* d_beta, double* loglik,
                          double* d_grad) {
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

int logit_hessian_dev(bbx_logit* c, const double* d_v, double* d_out) {
  if (!c->have_location)
    return fail(BBX_ERR_STATE, "bbx_logit_set_location has not succeeded");
  bbx_design* h = c->h;
  BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
  BBX_TRY(launch_rows<LM_HESS>(c, c->eta.as<const double>(),
                               c->tmp.as<double>(), nullptr));
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, d_out);
}

}  // namespace

extern "C" {

int bbx_logit_create(bbx_design* design, const double* n_success,
                     const double* n_trial, bbx_logit** out) {
  return no_throw(
      [&] { return logit_create_impl(design, n_success, n_trial, out); });
}

int bbx_logit_destroy(bbx_logit* c) {
  if (!c) return BBX_OK;
  if (design_alive(c->h)) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->h->stream);
  }
  ham::free_pinned(c);
  delete c;
  return BBX_OK;
}

int bbx_logit_loglik_grad_dev(bbx_logit* c, const double* d_beta,
                              double* loglik, double* d_grad) {
  BBX_TRY(logit_check(c));
  if (!d_beta || !loglik) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw(
      [&] { return logit_loglik_grad_dev(c, d_beta, loglik, d_grad); });
}

int bbx_logit_loglik_grad(bbx_logit* c, const double* beta, double* loglik,
                          double* grad) {
  BBX_TRY(logit_check(c));
  if (!beta || !loglik) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    double ll = 0.;
    BBX_TRY(with_p_stage(c, beta, grad, [&](const double* d_in, double* d_out) {
      return logit_loglik_grad_dev(c, d_in, &ll, d_out);
    }));
    *loglik = ll;
    return BBX_OK;
  });
}

int bbx_logit_set_location(bbx_logit* c, const double* beta) {
  BBX_TRY(logit_check(c));
  if (!beta) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    bbx_design* h = c->h;
    c->have_location = false;
    double* d_in = h->stage_P.as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(launch_rows<LM_LOC>(c, c->eta.as<const double>(),
                                c->d_loc.as<double>(), nullptr));
    BBX_HIP(hipStreamSynchronize(h->stream));   // beta is free again
    c->have_location = true;
    return BBX_OK;
  });
}

int bbx_logit_hessian_matvec_dev(bbx_logit* c, const double* d_v,
                                 double* d_out) {
  BBX_TRY(logit_check(c));
  if (!d_v || !d_out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return logit_hessian_dev(c, d_v, d_out); });
}

int bbx_logit_hessian_matvec(bbx_logit* c, const double* v, double* out) {
  BBX_TRY(logit_check(c));
  if (!v || !out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return with_p_stage(c, v, out, [&](const double* d_in, double* d_out) {
      return logit_hessian_dev(c, d_in, d_out);
    });
  });
}

int bbx_logit_hmc_trajectory(bbx_logit* c, double dt, int n_step,
                             const double* precond_scale,
                             const double* prior_prec, const double* q0,
                             const double* p0, double logp0,
                             const double* grad0, double hamiltonian_tol,
                             double* q, double* p, double* logp, double* grad,
                             int* n_grad_evals, int* instability,
                             double* hamiltonian) {
  BBX_TRY(logit_check(c));
  if (!precond_scale || !prior_prec || !q0 || !p0 || !grad0)
    return fail(BBX_ERR_INVALID, "NULL argument");
  if (n_step < 0) return fail(BBX_ERR_INVALID, "n_step < 0");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    LogitLik lik{c};
    return ham::trajectory_impl(c, lik, dt, n_step, precond_scale, prior_prec,
                                q0, p0, logp0, grad0, hamiltonian_tol, q, p,
                                logp, grad, n_grad_evals, instability,
                                hamiltonian);
  });
}

int bbx_logit_nuts_begin(bbx_logit* c, const double* precond_scale,
                         const double* prior_prec, const double* q0,
                         const double* p0, double logp0, const double* grad0,
                         double joint_logp0, double joint_logp_threshold,
                         double hamiltonian_tol) {
  BBX_TRY(logit_check(c));
  if (!precond_scale || !prior_prec || !q0 || !p0 || !grad0)
    return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return ham::nuts_begin_impl(c, precond_scale, prior_prec, q0, p0, logp0,
                                grad0, joint_logp0, joint_logp_threshold,
                                hamiltonian_tol);
  });
}

int bbx_logit_nuts_doubling(bbx_logit* c, double dt, int direction, int height,
                            const double* uniforms, int* n_uniform_used,
                            int* n_steps, int* flags, int* tree,
                            double* averages) {
  BBX_TRY(logit_check(c));
  BBX_TRY(ham::nuts_doubling_args(c, "bbx_logit", uniforms, direction, height));
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    LogitLik lik{c};
    BBX_TRY(ham::nuts_doubling_impl(c, lik, dt, direction, height, uniforms));
    ham::nuts_doubling_out(c, n_uniform_used, n_steps, flags, tree, averages);
    return BBX_OK;
  });
}

int bbx_logit_nuts_sample(bbx_logit* c, double* q, double* logp,
                          double* grad) {
  BBX_TRY(logit_check(c));
  if (!c->nuts_begun)
    return fail(BBX_ERR_STATE, "bbx_logit_nuts_begin has not succeeded");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return ham::nuts_sample_impl(c, q, logp, grad); });
}

}  // extern "C"
