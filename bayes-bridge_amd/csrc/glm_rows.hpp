// What the row-wise GLM likelihood handles share (logit.hip, poisson.hip,
// negbin.hip, ordinal.hip, weibull.hip): the handle base, the one row kernel,
// its launch, the likelihood block, the family that hamiltonian.hpp's entry
// points take and the body of `create`; and, for the families with an
// auxiliary parameter (negbin.hip's dispersion, weibull.hip's shape,
// ordinal.hip's cutpoints), the one candidate kernel, its host driver and the
// C ABI's front.  A row holds a pair (s, t) -- (n_success, n_trial), or (y, log
// exposure) -- and every per-row value is a function of the row's linear
// predictor and its pair alone.  A handle states a policy V, passed to the
// kernel by value (empty, or the few numbers the expressions need):
//
//   device side (the per-row expressions; everything else is written once)
//     loc(x, s, t)            the Hessian's location value d_i at eta_i = x
//     grad(x, s, t, w, l)     gradient mode: w_i and ll_i; returns the
//                             family's own test for raising CoxTraj::zero and
//                             skip (read only where `raises`)
//     raises                  static constexpr bool: false compiles the
//                             kernel without any flag code
//   host side
//     Handle, name            the C ABI's struct and "logit", "poisson", ...
//     make(c)                 the policy of handle c
//
// The Hessian mode is -(d_i u_i) for every family and is written in the
// kernel.  A policy method is the expression of its handle's file header, with
// that association and rounding order; the kernel only loads, adds, reduces
// and stores.  Policies live in the unnamed namespace of their file and the
// kernel is static: no two translation units instantiate it with the same
// arguments, and no handle type's name reaches an exported symbol.
//
// The contract of the row kernel:
//  - Its reductions (sum ll, sum w) are block sums in a fixed order into NPART
//    partials over a FIXED partition -- row i belongs to workgroup
//    (i / VEC_BLOCK) % NPART, as in cox_weight_kernel -- re-added in a fixed
//    order by their consumers: no float atomics, the same inputs give the same
//    bits on every run.
//  - A thread keeps GLM_ROW_U rows of consecutive laps in flight (their loads
//    are issued before the first exp), and a row's pair is stored interleaved
//    so that it is one 16-byte load; the rows are still added in lap order, so
//    the partials do not depend on GLM_ROW_U.
//  - Where a family's test fires, the gradient mode raises CoxTraj::zero (and
//    skip), as the Cox scan does for an empty risk-set sum: the log-likelihood
//    reads -inf whatever the other rows hold, the trajectory's instability
//    rule fires at this step and a half-tree ends here, with no step taken
//    from a gradient that does not exist.  `skip` points at st->skip: a
//    workgroup that starts after this store returns at entry and leaves its
//    partials stale.  They are never read: every consumer (cox_loglik_kernel,
//    post_b, the leaf kernel) looks at st->zero first, as after
//    cox_scan_sum_kernel<SM_INVH>.  A NaN raises no flag: it comes out of the
//    sums as a NaN.
//
// The candidate sums: L(candidate j), j < K <= MAXC, of an auxiliary parameter
// in one pass over the rows, at the coefficients given or on the linear
// predictor the previous call left in the handle.  A family states a policy C:
//
//   device side
//     MAXC, TAB               candidates per call; doubles per candidate's
//                             table
//     struct Row              what a thread keeps of a row
//     row(eta, pair)          ... from the row's linear predictor and pair
//     term(row, tab)          the row's term for the candidate of table `tab`
//   host side
//     Handle, family          the C ABI's struct (a GlmCandCore) and "negbin"
//     who, count, arg, must   the words of the front's messages
//     stride(c)               doubles per candidate in the caller's array
//     valid(c, v)             the front's test of one candidate
//     fill(c, v, tab)         one candidate's table from the caller's array
//     Sum                     the type the NPART partials are re-added in
//
// The candidate kernel stands under the row kernel's contract: its partition,
// GLM_ROW_U rows in flight, a thread's rows added in lap order, one block sum
// per candidate and K x NPART candidate-major partials, re-added on the host
// in index order.  A row's term for candidate j is a function of the row and
// table j alone, and every candidate has its own accumulator: the sum of a
// candidate depends neither on K nor on its place among the K.
//
// The fp-contract pragma below is file-scope and meant to hold to the end of
// the including translation unit: it binds where a template is written, not
// where it is instantiated, so the kernel needs it here, and every file that
// is included after this one states the same pragma itself.
#pragma once
#include <math.h>

#include <cmath>
#include <string>
#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

static_assert(SCAN_G == NPART, "the row kernel writes one loglik partial per "
                               "workgroup into HamCore::llpart");

constexpr int GLM_ROW_U = 4;   // rows in flight per thread

enum GlmRowMode {
  GLM_GRAD = 0,   // w, partials of sum ll and of sum w
  GLM_LOC = 1,    // d, the location value
  GLM_HESS = 2    // w = -(d u), partials of sum w
};

// The buffers of every row-wise handle (the design is borrowed: it must
// outlive the handle)
struct GlmRowsCore : HamCore {
  DevMem pair;   // 2 n: (s_i, t_i)
  DevMem loc;    // n: the Hessian's location
};

// ... and of every handle with candidate sums
struct GlmCandCore : GlmRowsCore {
  DevMem eta_cand;    // n: eta of the last candidate call with coefficients
  DevMem cand_part;   // MAXC x NPART partials of the candidate sums
  DevMem cand_tab;    // MAXC x TAB: the call's tables
  bool have_eta_cand = false;
};

// `a`: eta (GLM_GRAD, GLM_LOC) or u = X~ v (GLM_HESS); `pair`: (s_i, t_i)
// (GLM_GRAD, GLM_LOC); `d`: the location's d (GLM_HESS); `out`: w or d.
template <class V, int MODE>
static __global__ __launch_bounds__(VEC_BLOCK) void glm_row_kernel(
    int64_t n, const double* __restrict__ a, const double2* __restrict__ pair,
    const double* __restrict__ d, double* __restrict__ out, V v_,
    double* __restrict__ llpart, double* __restrict__ sumw_part, CoxTraj* st,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  double acc = 0., ll = 0.;
  bool over = false;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += GLM_ROW_U * lap) {
    double x[GLM_ROW_U], s[GLM_ROW_U], t[GLM_ROW_U];
#pragma unroll
    for (int k = 0; k < GLM_ROW_U; ++k) {
      const int64_t i = i0 + k * lap;
      x[k] = s[k] = t[k] = 0.;
      if (i < n) {
        x[k] = a[i];
        if (MODE == GLM_HESS) {
          s[k] = d[i];
        } else {
          const double2 c = pair[i];
          s[k] = c.x;
          t[k] = c.y;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < GLM_ROW_U; ++k) {
      const int64_t i = i0 + k * lap;
      if (i >= n) break;
      double v;
      if (MODE == GLM_HESS) {
        v = -(s[k] * x[k]);
      } else if (MODE == GLM_LOC) {
        v = v_.loc(x[k], s[k], t[k]);
      } else {
        double l;
        const bool raise = v_.grad(x[k], s[k], t[k], v, l);
        ll += l;
        if (V::raises) over |= raise;
      }
      out[i] = v;
      acc += v;
    }
  }
  if (MODE == GLM_LOC) return;
  acc = block_sum<VEC_BLOCK>(acc);
  if (MODE == GLM_GRAD) {
    ll = block_sum<VEC_BLOCK>(ll);
    if (V::raises && over) {
      st->zero = 1;
      st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    sumw_part[blockIdx.x] = acc;
    if (MODE == GLM_GRAD) llpart[blockIdx.x] = ll;
  }
}

// K sums over the rows in one pass, on the row kernel's partition and in its
// order of addition.  `tabs`: K tables, C::TAB doubles apart; `part`:
// K x NPART partials, candidate-major.  The K running sums of a thread live in
// LDS (one column per thread: no bank conflict, no barrier), so that the loop
// over j is a loop and K a number: the K = 8 body unrolled holds more
// wave-uniform values (the tables and the polynomial coefficients of exp,
// log1p and log) than there are scalar registers, and more live values than
// the register budget of the row kernels.
template <class C>
static __global__ __launch_bounds__(VEC_BLOCK) void glm_cand_kernel(
    int64_t n, int K, const double* __restrict__ eta,
    const double2* __restrict__ pair, const double* __restrict__ tabs,
    double* __restrict__ part) {
  __shared__ double s_acc[C::MAXC][VEC_BLOCK];
  for (int j = 0; j < K; ++j) s_acc[j][threadIdx.x] = 0.;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += GLM_ROW_U * lap) {
    typename C::Row row[GLM_ROW_U] = {};
#pragma unroll
    for (int u = 0; u < GLM_ROW_U; ++u) {
      const int64_t i = i0 + u * lap;
      if (i < n) row[u] = C::row(eta[i], pair[i]);
    }
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
      const double* tab = tabs + j * C::TAB;
      double acc = s_acc[j][threadIdx.x];
#pragma unroll
      for (int u = 0; u < GLM_ROW_U; ++u) {
        if (i0 + u * lap >= n) break;
        acc += C::term(row[u], tab);
      }
      s_acc[j][threadIdx.x] = acc;
    }
  }
  for (int j = 0; j < K; ++j) {
    const double sum = block_sum<VEC_BLOCK>(s_acc[j][threadIdx.x]);
    if (threadIdx.x == 0) part[j * NPART + blockIdx.x] = sum;
  }
}

namespace {  // host side: internal, as the handle types appear in the names

using ham::cst;
using ham::eta_of;

template <class V, int MODE>
int launch_rows(typename V::Handle* c, const double* a, double* out,
                const int* skip) {
  bbx_design* h = c->h;
  BBX_LAUNCH((glm_row_kernel<V, MODE>), dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, a, c->pair.template as<const double2>(),
             c->loc.template as<const double>(), out, V::make(c),
             c->llpart.template as<double>(), part_slot(h, PS_SUMW), cst(c),
             skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// From eta (in c->eta, complete in stream order): w, the loglik partials and
// (grad != null) grad = X~^T w.
template <class V>
int likelihood_from_eta(typename V::Handle* c, double* grad) {
  bbx_design* h = c->h;
  BBX_TRY((launch_rows<V, GLM_GRAD>(c, c->eta.template as<const double>(),
                                    c->tmp.template as<double>(),
                                    &cst(c)->skip)));
  if (!grad) return BBX_OK;
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.template as<double>(), part_slot(h, PS_SUMW),
                     ep, grad);
}

// The policy hamiltonian.hpp's entry points take
template <class V>
struct GlmFamilyT {
  using H = typename V::Handle;
  static constexpr const char* name = V::name;
  // The family's block of a leapfrog step
  struct Lik {
    H* c;
    int operator()(double* grad) const {
      return likelihood_from_eta<V>(c, grad);
    }
  };
  static int locate(H* c, const double* d_in) {
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY((launch_rows<V, GLM_LOC>(c, c->eta.template as<const double>(),
                                     c->loc.template as<double>(), nullptr)));
    BBX_HIP(hipStreamSynchronize(c->h->stream));   // beta is free again
    return BBX_OK;
  }
  static int hessian_from_v(H* c, const double* d_v, double* d_out) {
    bbx_design* h = c->h;
    BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
    BBX_TRY((launch_rows<V, GLM_HESS>(c, c->eta.template as<const double>(),
                                      c->tmp.template as<double>(), nullptr)));
    TdotEpilogue ep;
    return launch_tdot(h, c->tmp.template as<double>(), part_slot(h, PS_SUMW),
                       ep, d_out);
  }
};

// The candidate buffers of a fresh handle (a `more` of glm_create_rows)
template <class C>
int alloc_cand(typename C::Handle* c) {
  const size_t d8 = sizeof(double);
  BBX_TRY(c->eta_cand.alloc(d8 * c->h->n));
  BBX_TRY(c->cand_part.alloc(d8 * C::MAXC * NPART));
  return c->cand_tab.alloc(d8 * C::MAXC * C::TAB);
}

// L(candidate j), j < K, at beta (null: the eta of the previous call): the
// product into eta_cand, the candidates' tables up, one launch, the K x NPART
// partials back in one copy and re-added on the host in index order in
// C::Sum, rounded once.
template <class C>
int cand_loglik_impl(typename C::Handle* c, const double* beta, int K,
                     const double* v, double* out) {
  bbx_design* h = c->h;
  if (beta) {
    c->have_eta_cand = false;
    double* d_in = h->stage_P.template as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(launch_prep_v(h, d_in, nullptr, nullptr, part_slot(h, PS_C)));
    BBX_TRY(launch_dot(h, d_in, nullptr, c->eta_cand.template as<double>(),
                       nullptr));
  }
  double tab[C::MAXC * C::TAB] = {};
  for (int j = 0; j < K; ++j)
    C::fill(c, v + (size_t)j * C::stride(c), tab + j * C::TAB);
  // (tab outlives the copy: this function synchronises before it returns)
  BBX_HIP(hipMemcpyAsync(c->cand_tab.ptr, tab, sizeof(double) * K * C::TAB,
                         hipMemcpyHostToDevice, h->stream));
  BBX_LAUNCH(glm_cand_kernel<C>, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->n, K, c->eta_cand.template as<const double>(),
             c->pair.template as<const double2>(),
             c->cand_tab.template as<const double>(),
             c->cand_part.template as<double>());
  BBX_HIP(hipGetLastError());
  std::vector<double> part((size_t)K * NPART);
  BBX_HIP(hipMemcpyAsync(part.data(), c->cand_part.ptr,
                         sizeof(double) * part.size(), hipMemcpyDeviceToHost,
                         h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));   // the one synchronisation
  if (beta) c->have_eta_cand = true;
  for (int j = 0; j < K; ++j) {
    typename C::Sum sum = 0.;
    for (int b = 0; b < NPART; ++b) sum += part[(size_t)j * NPART + b];
    out[j] = (double)sum;
  }
  return BBX_OK;
}

// The C ABI's front of the candidate sums
template <class C>
int cand_loglik(typename C::Handle* c, const double* beta, int K,
                const double* v, double* out) {
  const std::string who = C::who;
  BBX_TRY(ham::check(c, C::family));
  if (!v || !out) return fail(BBX_ERR_INVALID, who + "NULL argument");
  if (K < 1 || K > C::MAXC)
    return fail(BBX_ERR_INVALID, who + C::count + " outside [1, " +
                                     std::to_string(C::MAXC) + "]");
  for (int j = 0; j < K; ++j) {
    if (!C::valid(c, v + (size_t)j * C::stride(c)))
      return fail(BBX_ERR_INVALID, who + C::arg + "[" + std::to_string(j) +
                                       "] is not finite and " + C::must);
  }
  if (!beta && !c->have_eta_cand)
    return fail(BBX_ERR_STATE, who + "no linear predictor is cached: the "
                                     "first call on a handle needs beta");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return cand_loglik_impl<C>(c, beta, K, v, out); });
}

inline bool finite_positive(double x) { return std::isfinite(x) && x > 0.; }

// The shared head of a `create`; `counts`: every array the family needs is
// given.
template <class H>
int glm_create_head(bbx_design* h, bool counts, H** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!counts) return fail(BBX_ERR_INVALID, "NULL count array");
  return BBX_OK;
}

// The rest of it: the pairs (s[i], t ? t[i] : 0) interleaved, each passed by
// `row(i, s_i, t_i)` (BBX_OK, or the failure), a fresh handle with HamCore's
// buffers and GlmRowsCore's, `more(c)` for the family's own, and the upload.
template <class H, class Row, class More>
int glm_create_rows(bbx_design* h, const char* family, const double* s,
                    const double* t, Row&& row, More&& more, H** out) {
  const int64_t n = h->n;
  std::vector<double> pair((size_t)2 * n);
  for (int64_t i = 0; i < n; ++i) {
    const double si = s[i], ti = t ? t[i] : 0.;
    BBX_TRY(row(i, si, ti));
    pair[2 * i] = si;
    pair[2 * i + 1] = ti;
  }
  H* c = new H;
  const size_t d8 = sizeof(double);
  int st = ham::init_core(c, h, family);
  if (st == BBX_OK) st = c->loc.alloc(d8 * n);
  if (st == BBX_OK) st = more(c);
  if (st == BBX_OK) st = c->pair.alloc(d8 * 2 * n);
  if (st != BBX_OK) return ham::discard(c, st);
  hipError_t e = hipMemcpyAsync(c->pair.ptr, pair.data(), d8 * 2 * n,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string(family) +
                                                 " upload: " +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

// ... for a family without buffers of its own
template <class H, class Row>
int glm_create_rows(bbx_design* h, const char* family, const double* s,
                    const double* t, Row&& row, H** out) {
  return glm_create_rows(h, family, s, t, row, [](H*) { return BBX_OK; }, out);
}

// A row of the count families: a count and a log exposure
int glm_count_row(int64_t i, double yi, double oi) {
  if (!std::isfinite(yi))
    return fail(BBX_ERR_INVALID, "y[" + std::to_string(i) + "] is not finite");
  if (yi < 0.)
    return fail(BBX_ERR_INVALID, "y[" + std::to_string(i) + "] is negative");
  if (!std::isfinite(oi))
    return fail(BBX_ERR_INVALID,
                "log_exposure[" + std::to_string(i) + "] is not finite");
  return BBX_OK;
}

}  // namespace
}  // namespace bbx
