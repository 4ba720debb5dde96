// Weibull proportional-hazards likelihood of right-censored times for the
// Hamiltonian coefficient samplers: its gradient, its Hessian-vector product
// at a fixed location, the trajectory / No-U-Turn drivers of hamiltonian.hpp
// with this family's block between "eta is complete" and "grad_loglik is
// complete", and the reduction the shape's own update needs.
//
// Rows (d_i, lt_i): d = 1 for an event at t, 0 for a row censored at t, and
// lt = log t.  With eta = X~ beta and the shape k > 0 the hazard is
// h(t | x) = k t^(k - 1) exp(eta), and per row, with every product rounded
// before the sum it enters (fp-contract off):
//   m_i  = exp(eta_i + (k * lt_i))
//   ll_i = (d_i * eta_i) - m_i     (d (log k + (k - 1) lt) is constant in
//                                   beta: dropped here)
//   w_i  = d_i - m_i,  grad = X~^T w
// Hessian-vector product at a fixed location: the location's value is m_i,
// u = X~ v, out = X~^T (-(m u)).
// Shape: L(k) = sum_i (d_i * ((log k + ((k - 1) * lt_i)) + eta_i)) - m_i, the
// whole log density, for up to WEIBULL_MAXK values of k in one pass over the
// rows (weibull_terms.hpp states the term).
//
// At k = 1 the product k * lt is lt, so m, ll, w and the location are the
// Poisson handle's on rows (y = d, o = lt), bit for bit.
//
// Overflow, as in poisson.hip: where eta + k lt is past exp's range, m = inf
// and ll_i = -inf (NaN where eta itself is +inf and d = 1).  The test that
// raises CoxTraj::zero (and skip) is m == inf, not ll_i == -inf.  In the shape
// sums such a row's term is d times a finite number minus inf = -inf, and the
// sum for that k is exactly -inf for finite eta: no inf - inf is formed.
//
// The row kernel, its contract and the host side are glm_rows.hpp's; this
// file states the expressions above on rows (d_i, lt_i), with the handle's k
// in the policy, and adds the shape sums: a sibling kernel under the same
// contract, in which each of the K values has its own accumulator, block sum
// and NPART partials, and a row's term for k_j is computed from (eta, d, lt,
// k_j, log k_j) alone: the sum for a given k depends neither on K nor on its
// place among the K values.
#include <math.h>

#include <cmath>
#include <vector>

#include "common.hpp"
#include "glm_rows.hpp"
#include "hamiltonian.hpp"
#include "weibull_terms.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr int WEIBULL_MAXK = 8;   // values of k per shape call

// K sums of the whole log density in one pass over the rows, on the row
// kernel's partition and in its order of addition.  `tab`: (k_j, log k_j)
// pairs; `part`: K x NPART partials, value-major.  The K running sums of a
// thread live in LDS (one column per thread: no bank conflict, no barrier),
// as negbin_disp_kernel's do, so that the loop over j is a loop and K a
// number.  A row's term for k_j is a function of (eta, d, lt) and pair j
// alone.
static __global__ __launch_bounds__(VEC_BLOCK) void weibull_shape_kernel(
    int64_t n, int K, const double* __restrict__ eta,
    const double2* __restrict__ dlt, const double2* __restrict__ tab,
    double* __restrict__ part) {
  __shared__ double s_acc[WEIBULL_MAXK][VEC_BLOCK];
  for (int j = 0; j < K; ++j) s_acc[j][threadIdx.x] = 0.;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += GLM_ROW_U * lap) {
    double x[GLM_ROW_U], d[GLM_ROW_U], lt[GLM_ROW_U];
#pragma unroll
    for (int u = 0; u < GLM_ROW_U; ++u) {
      const int64_t i = i0 + u * lap;
      x[u] = d[u] = lt[u] = 0.;
      if (i < n) {
        const double2 c = dlt[i];
        d[u] = c.x;
        lt[u] = c.y;
        x[u] = eta[i];
      }
    }
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
      const double2 kk = tab[j];
      double acc = s_acc[j][threadIdx.x];
#pragma unroll
      for (int u = 0; u < GLM_ROW_U; ++u) {
        if (i0 + u * lap >= n) break;
        acc += weibull_full(x[u], d[u], lt[u], kk.x, kk.y);
      }
      s_acc[j][threadIdx.x] = acc;
    }
  }
  for (int j = 0; j < K; ++j) {
    const double sum = block_sum<VEC_BLOCK>(s_acc[j][threadIdx.x]);
    if (threadIdx.x == 0) part[j * NPART + blockIdx.x] = sum;
  }
}

}  // namespace bbx

using namespace bbx;

// One Weibull likelihood on a design: rows (d_i, log t_i)
struct bbx_weibull : GlmRowsCore {
  DevMem eta_shape;    // n: eta of the last shape call with coefficients
  DevMem shape_part;   // WEIBULL_MAXK x NPART partials of the shape sums
  DevMem shape_tab;    // WEIBULL_MAXK pairs (k, log k) of the call
  double k = 1., logk = 0.;
  bool have_eta_shape = false;
};

namespace {

// the handle's k and log k, by value in the kernel's arguments (the
// beta-dependent part reads k alone: log k belongs to the whole density)
struct WeibullRows {
  using Handle = bbx_weibull;
  static constexpr const char* name = "weibull";
  static constexpr bool raises = true;
  double k, logk;
  static WeibullRows make(const bbx_weibull* c) {
    return WeibullRows{c->k, c->logk};
  }
  __device__ double loc(double x, double, double lt) const {
    return exp(weibull_arg(x, k, lt));
  }
  __device__ bool grad(double x, double d, double lt, double& w,
                       double& l) const {
    const double m = exp(weibull_arg(x, k, lt));
    w = d - m;
    l = d * x - m;
    return m == INFINITY;
  }
};

bool finite_positive(double k) { return std::isfinite(k) && k > 0.; }

int weibull_row(int64_t i, double di, double lti) {
  if (!(di == 0. || di == 1.))
    return fail(BBX_ERR_INVALID,
                "event[" + std::to_string(i) + "] is not 0 or 1");
  if (!std::isfinite(lti))
    return fail(BBX_ERR_INVALID,
                "log_time[" + std::to_string(i) + "] is not finite");
  return BBX_OK;
}

int weibull_create_impl(bbx_design* h, const double* event,
                        const double* log_time, double shape,
                        bbx_weibull** out) {
  BBX_TRY(glm_create_head(h, true, out));
  if (!event) return fail(BBX_ERR_INVALID, "NULL event array");
  if (!log_time) return fail(BBX_ERR_INVALID, "NULL log_time array");
  if (!finite_positive(shape))
    return fail(BBX_ERR_INVALID, "the shape is not finite and positive");
  return glm_create_rows(
      h, "weibull", event, log_time, weibull_row,
      [&](bbx_weibull* c) {
        c->k = shape;
        c->logk = log(shape);
        const size_t d8 = sizeof(double);
        BBX_TRY(c->eta_shape.alloc(d8 * h->n));
        BBX_TRY(c->shape_part.alloc(d8 * WEIBULL_MAXK * NPART));
        return c->shape_tab.alloc(d8 * WEIBULL_MAXK * 2);
      },
      out);
}

// L(k_j), j < n_k, at beta (null: the eta of the previous call): the product
// into eta_shape, the pairs (k, log k) up, one launch of the shape kernel,
// the K x NPART partials back in one copy and re-added on the host in index
// order, in long double and rounded once: NPART partials of one size added in
// double one after the other lose several ulps, which the slice sampler would
// not notice but the tests' bound (4 float64 roundings) does.
int shape_loglik_impl(bbx_weibull* c, const double* beta, int n_k,
                      const double* k, double* out) {
  bbx_design* h = c->h;
  if (beta) {
    c->have_eta_shape = false;
    double* d_in = h->stage_P.as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(launch_prep_v(h, d_in, nullptr, nullptr, part_slot(h, PS_C)));
    BBX_TRY(launch_dot(h, d_in, nullptr, c->eta_shape.as<double>(), nullptr));
  }
  double tab[WEIBULL_MAXK * 2];
  for (int j = 0; j < n_k; ++j) {
    tab[2 * j] = k[j];
    tab[2 * j + 1] = log(k[j]);
  }
  // (tab outlives the copy: this function synchronises before it returns)
  BBX_HIP(hipMemcpyAsync(c->shape_tab.ptr, tab, sizeof(double) * 2 * n_k,
                         hipMemcpyHostToDevice, h->stream));
  BBX_LAUNCH(weibull_shape_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->n, n_k, c->eta_shape.as<const double>(),
             c->pair.as<const double2>(), c->shape_tab.as<const double2>(),
             c->shape_part.as<double>());
  BBX_HIP(hipGetLastError());
  std::vector<double> part((size_t)n_k * NPART);
  BBX_HIP(hipMemcpyAsync(part.data(), c->shape_part.ptr,
                         sizeof(double) * part.size(), hipMemcpyDeviceToHost,
                         h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));   // the one synchronisation
  if (beta) c->have_eta_shape = true;
  for (int j = 0; j < n_k; ++j) {
    long double sum = 0.;
    for (int b = 0; b < NPART; ++b) sum += part[(size_t)j * NPART + b];
    out[j] = (double)sum;
  }
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_weibull_create(bbx_design* design, const double* event,
                                  const double* log_time, double shape,
                                  bbx_weibull** out) {
  return no_throw([&] {
    return weibull_create_impl(design, event, log_time, shape, out);
  });
}

extern "C" int bbx_weibull_set_shape(bbx_weibull* c, double k) {
  BBX_TRY(ham::check(c, "weibull"));
  if (!finite_positive(k))
    return fail(BBX_ERR_INVALID,
                "bbx_weibull_set_shape: the shape is not finite and positive");
  if (c->nuts_open)
    return fail(BBX_ERR_STATE,
                "bbx_weibull_set_shape: a No-U-Turn tree is installed on the "
                "handle (bbx_weibull_nuts_begin); take its sample "
                "(bbx_weibull_nuts_sample) first");
  c->k = k;
  c->logk = log(k);
  c->have_location = false;   // m was formed with the previous k
  return BBX_OK;
}

extern "C" int bbx_weibull_shape_loglik(bbx_weibull* c, const double* beta,
                                        int n_k, const double* k,
                                        double* out) {
  const char* who = "bbx_weibull_shape_loglik: ";
  BBX_TRY(ham::check(c, "weibull"));
  if (!k || !out) return fail(BBX_ERR_INVALID, std::string(who) + "NULL argument");
  if (n_k < 1 || n_k > WEIBULL_MAXK)
    return fail(BBX_ERR_INVALID, std::string(who) + "n_k outside [1, " +
                                     std::to_string(WEIBULL_MAXK) + "]");
  for (int j = 0; j < n_k; ++j) {
    if (!finite_positive(k[j]))
      return fail(BBX_ERR_INVALID, std::string(who) + "k[" +
                                       std::to_string(j) +
                                       "] is not finite and positive");
  }
  if (!beta && !c->have_eta_shape)
    return fail(BBX_ERR_STATE, std::string(who) +
                                   "no linear predictor is cached: the first "
                                   "call on a handle needs beta");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return shape_loglik_impl(c, beta, n_k, k, out); });
}

BBX_HAM_ENTRY_POINTS(weibull, GlmFamilyT<WeibullRows>)
