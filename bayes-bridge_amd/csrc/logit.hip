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
  const size_t d8 = sizeof(double);
  int st = ham::init_core(c, h, "logit");
  if (st == BBX_OK) st = c->d_loc.alloc(d8 * n);
  if (st == BBX_OK) st = c->ym.alloc(d8 * 2 * n);
  if (st != BBX_OK) return ham::discard(c, st);
  hipError_t e = hipMemcpyAsync(c->ym.ptr, ym.data(), d8 * 2 * n,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("logit upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

struct LogitFamily {
  static constexpr const char* name = "logit";
  using Lik = LogitLik;
  static int locate(bbx_logit* c, const double* d_in) {
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(launch_rows<LM_LOC>(c, c->eta.as<const double>(),
                                c->d_loc.as<double>(), nullptr));
    BBX_HIP(hipStreamSynchronize(c->h->stream));   // beta is free again
    return BBX_OK;
  }
  static int hessian_from_v(bbx_logit* c, const double* d_v, double* d_out) {
    bbx_design* h = c->h;
    BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
    BBX_TRY(launch_rows<LM_HESS>(c, c->eta.as<const double>(),
                                 c->tmp.as<double>(), nullptr));
    TdotEpilogue ep;
    return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, d_out);
  }
};

}  // namespace

extern "C" int bbx_logit_create(bbx_design* design, const double* n_success,
                                const double* n_trial, bbx_logit** out) {
  return no_throw(
      [&] { return logit_create_impl(design, n_success, n_trial, out); });
}

BBX_HAM_ENTRY_POINTS(logit, LogitFamily)
