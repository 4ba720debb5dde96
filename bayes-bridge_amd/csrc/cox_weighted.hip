// Cox partial likelihood with case weights (Breslow ties), on the plain
// handle's row order and launch count (cox.hip).  The preconditioned
// trajectory and the No-U-Turn tree are hamiltonian.hpp's.
//
// Rows are ordered as cox.hip orders them: events first by increasing time,
// then censored observations by decreasing censoring time.  Risk set k
// (k < ne) is [start_k, end_k]; n_app[i] counts the risk sets that contain i.
// With weights a_i > 0, eta = X~ beta, m = max eta (of eta alone, not of
// eta + log a) and g_i = a_i exp(eta_i - m), the product rounded once:
//   scan_i = sum_{j=i}^{ne-1} g_j  (i < ne: suffix over the events)
//          = sum_{j=ne}^{i}   g_j  (i >= ne: prefix over the censored)
//   H_k    = scan[start_k] + (end_k >= ne ? scan[end_k] : 0)
//   loglik = sum_k a_k ((eta_k - m) - log H_k)      (-inf if some H_k == 0)
//   q_k    = a_k (1/H_k),  c = cumsum q
//   w_i    = [i < ne] a_i - c[n_app_i - 1] g_i,  grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v, S = segsum(g u),
//   z_k = a_k ((1/H_k) ((1/H_k) S_k)), cz = cumsum z,
//   r_i = (c[n_app_i - 1] g_i) u_i - g_i cz[n_app_i - 1],  out = X~^T (-r).
// With integer weights this is the plain likelihood of the data with row i
// written a_i times (the copies of an event share one risk set); with all
// weights 1 every product by a is exact and the bits are the plain handle's.
//
// Rounding order.  1/H_k is rounded first and multiplied by a_k (q_k is not
// a_k / H_k); z_k is formed innermost first: t = (1/H_k) S_k, t = (1/H_k) t,
// z_k = a_k t, each rounded.  The location keeps g, c and 1/H_k itself (the
// event pass A stores it beside a/H in the same launch).  Doubling
// every weight multiplies every intermediate by a power of two, so gradient
// and Hessian product double bit for bit.
//
// H_k == 0 is an empty risk set: CoxTraj::zero and skip are raised as the
// plain handle raises them.  A NaN stays a NaN.
//
// The kernels, their partition and reductions, the six launches and the
// family are cox_family.hpp's; this file states the formulae above as its
// policy (CoxWeighted), the index checks and the C entry points.
//
// Scans: the fixed partition and pass B of cox_scan.hpp.  Launches per
// likelihood, as the plain handle's: max, g pass A / B, a/H pass A / B,
// weights.  The event pass reads a_k from the row vector (events are rows
// 0 .. ne - 1).  No float atomics: the same inputs give the same bits on every
// run.
#include <math.h>

#include <string>

#include "common.hpp"
#include "cox_family.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One weighted Cox likelihood on a design (borrowed: the design must outlive
// it).  CoxCore's h buffers hold g, inv holds a/H (or z) and inv_loc 1/H.
struct bbx_coxw : CoxCore {
  DevMem start, end, napp;               // int32: ne, ne, n
  DevMem wt;                             // n: the case weights
  // out of line, as it has been since the handle was added: libbbx.so's
  // dynamic symbols name it
  __attribute__((noinline)) ~bbx_coxw() {}
};

namespace {

// The header's formulae as cox_family.hpp's kernels ask for them
struct CoxWeighted {
  using Handle = bbx_coxw;
  static constexpr const char* name = "coxw";
  static constexpr int halves = 1;
  static constexpr bool keeps_inv = true;  // the location's 1/H beside a/H
  const int32_t* start;
  const int32_t* end;
  const int32_t* napp;
  const double* a;                       // the weights, in row order
  int64_t ne;
  static CoxWeighted make(const bbx_coxw* c) {
    return {c->start.as<const int32_t>(), c->end.as<const int32_t>(),
            c->napp.as<const int32_t>(), c->wt.as<const double>(), c->ne};
  }
  // the events reversed (suffix sums), the censored rows forward
  static void risk_layout(const bbx_coxw* c, int* nseg, int64_t* len,
                          int* rev) {
    *nseg = 2;
    len[0] = c->ne, rev[0] = 1;
    len[1] = c->n - c->ne, rev[1] = 0;
  }
  static double* hu(bbx_coxw* c) { return c->tmp.as<double>(); }
  __device__ int64_t row(int, int64_t i) const { return i; }
  __device__ double h_of(int64_t r, double e) const { return a[r] * e; }
  __device__ double risk_term(int, int64_t, double x) const { return x; }
  // a_k from the row vector: events are rows 0 .. ne - 1
  __device__ double H(const double* scan, int64_t k, double& ak) const {
    const int32_t e = end[k];
    double H = scan[start[k]];
    if (e >= ne) H += scan[e];
    ak = a[k];
    return H;
  }
  __device__ bool empty(double H) const { return H == 0.; }
  __device__ int64_t event_row(int64_t k) const { return k; }
  __device__ double scaled(double x, double ak) const { return ak * x; }
  template <bool HESS>
  __device__ void AZ(const double* c, const double* cz, int64_t i, double& A,
                     double& Z) const {
    const int32_t k = napp[i] - 1;
    A = c[k];
    if (HESS) Z = cz[k];
  }
  __device__ double indicator(int64_t i) const { return i < ne ? a[i] : 0.; }
};

int coxw_create_impl(bbx_design* h, int64_t n_event, const int32_t* start,
                     const int32_t* end, const int32_t* n_app,
                     const double* weights, bbx_coxw** out) {
  BBX_TRY(cox_create_head(h, n_event,
                          !start || !end || !n_app ? "NULL index array"
                          : !weights               ? "NULL weights"
                                                   : nullptr,
                          out));
  const int64_t n = h->n;
  // the kernels index scan[start], scan[end] and c[n_app - 1]: check them all
  for (int64_t k = 0; k < n_event; ++k) {
    if (start[k] < 0 || start[k] > k || end[k] < n_event - 1 || end[k] >= n)
      return fail(BBX_ERR_INVALID, "risk set " + std::to_string(k) +
                                       " out of range");
  }
  for (int64_t i = 0; i < n; ++i) {
    if (n_app[i] < 1 || n_app[i] > n_event)
      return fail(BBX_ERR_INVALID, "n_app[" + std::to_string(i) +
                                       "] outside [1, n_event]");
  }
  for (int64_t i = 0; i < n; ++i) {
    // !(x > 0) is true of a NaN too
    if (!(weights[i] > 0.) || isinf(weights[i]))
      return fail(BBX_ERR_INVALID, "weights[" + std::to_string(i) +
                                       "] is not a finite positive number");
  }

  bbx_coxw* c = new bbx_coxw;
  const char* fam = CoxWeighted::name;
  int st = cox_alloc(c, h, fam, n_event, n, n_event);
  if (st == BBX_OK) st = cox_upload(c, fam, c->start, start, n_event);
  if (st == BBX_OK) st = cox_upload(c, fam, c->end, end, n_event);
  if (st == BBX_OK) st = cox_upload(c, fam, c->napp, n_app, n);
  if (st == BBX_OK) st = cox_upload(c, fam, c->wt, weights, n);
  if (st == BBX_OK) st = cox_uploaded(c, fam);
  if (st != BBX_OK) return ham::discard(c, st);
  *out = c;
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_coxw_create(bbx_design* design, int64_t n_event,
                               const int32_t* start, const int32_t* end,
                               const int32_t* n_app, const double* weights,
                               bbx_coxw** out) {
  return no_throw([&] {
    return coxw_create_impl(design, n_event, start, end, n_app, weights, out);
  });
}

BBX_HAM_ENTRY_POINTS(coxw, CoxFamilyT<CoxWeighted>)
BBX_COX_PREDICT_ENTRY_POINTS(coxw, CoxFamilyT<CoxWeighted>)
