// Cox partial likelihood with Efron's approximation for tied event times, on
// the plain handle's row order and launch count (cox.hip).  The preconditioned
// trajectory and the No-U-Turn tree are hamiltonian.hpp's.
//
// Rows are ordered as cox.hip orders them: events first by increasing time,
// then censored observations by decreasing censoring time.  Event k belongs to
// a tie group of rows s .. s+d-1 (s = start_k); its position in the group is
// l = k - s and a_k = 1 - l/d.  With eta = X~ beta, m = max eta,
// h_i = exp(eta_i - m), E the suffix sum of h over the events (E[ne] = 0) and
// C the prefix sum of h over the censored rows:
//   R_g    = E[s+d] + (end_k >= ne ? C[end_k] : 0)   at risk, not in the group
//   T_g    = E[s] - E[s+d]                           the tie group
//   phi_k  = R_g + a_k T_g                  (Breslow: R_g + T_g for every k)
//   loglik = sum_k (eta_k - m) - log phi_k  (-inf if some phi_k <= 0)
//   inv_k  = 1/phi_k,  c = cumsum inv,  cb = cumsum (l/d) inv    (cb[-1] = 0)
//   A_i    = c[n_app_i - 1] - [i < ne] (cb[s_i + d_i - 1] - cb[s_i - 1])
//   w_i    = [i < ne] - h_i A_i,  grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v, S_k = SR_g + a_k ST_g
// from the same scans of h u, z_k = inv_k (inv_k S_k), cz and czb as c and cb,
// Z_i as A_i from them, r_i = (h_i A_i) u_i - h_i Z_i, out = X~^T (-r).
//
// Cancellation.  phi is formed as R + a T, not as (R + T) - (l/d) T: an error
// delta in T (|delta| <~ eps (R + T), the rounding of E[s]) moves phi by
// a delta, at most eps a (R + T) / (R + a T) <= eps relative to phi, whatever
// d is.  For the last tie group E[s+d] is the exact 0 and nothing is
// subtracted.  cb <= c term by term, so cb[s+d-1] - cb[s-1] is bounded by the
// rounding of c[n_app - 1] itself.  phi_k <= 0 is treated as the plain handle
// treats H_k == 0: CoxTraj::zero and skip are raised.
//
// The kernels, their partition and reductions, the six launches and the
// family are cox_family.hpp's; this file states the formulae above as its
// policy (CoxEfron), the index checks and the C entry points.
//
// Scans: the fixed partition and pass B of cox_scan.hpp.  inv and (l/d) inv
// are elements k and ne + k of one buffer of 2 ne values: the event pass A
// gathers once per event and leaves the chunk sums of both halves, and one
// pass B over two segments gives c and cb.  Launches per likelihood, as the
// plain handle's: max, h pass A / B, 1/phi pass A / B, weights.  No float
// atomics: the same inputs give the same bits on every run.
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_family.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One Cox likelihood with Efron ties on a design (borrowed: the design must
// outlive it).  The event-length buffers of CoxCore hold 2 ne values: (1/phi,
// l/d 1/phi) or z, and their cumsums (c, cb).
struct bbx_coxef : CoxCore {
  DevMem grp, end, napp;                 // int2 ne, int32 ne, int32 n
  // out of line, as it has been since the handle was added: libbbx.so's
  // dynamic symbols name it
  __attribute__((noinline)) ~bbx_coxef() {}
};

namespace {

// The header's formulae as cox_family.hpp's kernels ask for them
struct CoxEfron {
  using Handle = bbx_coxef;
  static constexpr const char* name = "coxef";
  static constexpr int halves = 2;       // inv and (l/d) inv; c and cb
  static constexpr int half_rev = 0;     // cb forward, as c
  static constexpr bool keeps_inv = false;
  const int2* grp;                       // (s - 1, s + d - 1) of every event
  const int32_t* end;
  const int32_t* napp;
  int64_t ne;
  static CoxEfron make(const bbx_coxef* c) {
    return {c->grp.as<const int2>(), c->end.as<const int32_t>(),
            c->napp.as<const int32_t>(), c->ne};
  }
  // E: the events reversed; C: the censored rows forward
  static void risk_layout(const bbx_coxef* c, int* nseg, int64_t* len,
                          int* rev) {
    *nseg = 2;
    len[0] = c->ne, rev[0] = 1;
    len[1] = c->n - c->ne, rev[1] = 0;
  }
  static double* hu(bbx_coxef* c) { return c->tmp.as<double>(); }
  __device__ int64_t row(int, int64_t i) const { return i; }
  __device__ double h_of(int64_t, double e) const { return e; }
  __device__ double risk_term(int, int64_t, double x) const { return x; }
  // phi_k = R_g + a_k T_g from one gather; lf = l/d
  __device__ double H(const double* scan, int64_t k, double& lf) const {
    const int2 g = grp[k];
    const int32_t e = end[k];
    const int64_t s = (int64_t)g.x + 1, next = (int64_t)g.y + 1;
    const double En = next < ne ? scan[next] : 0.;
    const double T = scan[s] - En;
    double R = En;
    if (e >= ne) R += scan[e];
    lf = (double)(k - s) / (double)(next - s);
    return R + (1. - lf) * T;
  }
  __device__ bool empty(double phi) const { return phi <= 0.; }
  __device__ int64_t event_row(int64_t k) const { return k; }
  __device__ double scaled(double x, double) const { return x; }
  // c in cum[0, ne) and cb in cum[ne, 2 ne)
  template <bool HESS>
  __device__ void AZ(const double* c, const double* cz, int64_t i, double& A,
                     double& Z) const {
    const int32_t k = napp[i] - 1;
    A = c[k];
    if (HESS) Z = cz[k];
    if (i < ne) {
      const int2 g = grp[i];
      A = A - (c[ne + g.y] - (g.x >= 0 ? c[ne + g.x] : 0.));
      if (HESS) Z = Z - (cz[ne + g.y] - (g.x >= 0 ? cz[ne + g.x] : 0.));
    }
  }
  __device__ double indicator(int64_t i) const { return i < ne ? 1. : 0.; }
};

std::string at(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

int coxef_create_impl(bbx_design* h, int64_t n_event, const int32_t* start,
                      const int32_t* end, const int32_t* n_app,
                      bbx_coxef** out) {
  BBX_TRY(cox_create_head(
      h, n_event, start && end && n_app ? nullptr : "NULL index array", out));
  const int64_t n = h->n;
  const int64_t ne = n_event;
  // the kernels index scan[s], scan[s + d], scan[end], c[n_app - 1],
  // cb[s - 1] and cb[s + d - 1]: check what is given, derive the tie groups
  // (events k and k' are tied iff start[k] == start[k'])
  for (int64_t k = 0; k < ne; ++k) {
    if (start[k] < 0 || start[k] > k)
      return fail(BBX_ERR_INVALID, at("start", k) + " outside [0, k]");
    if (k > 0 && start[k] < start[k - 1])
      return fail(BBX_ERR_INVALID, at("start", k) + " is decreasing");
    if (start[k] != k && start[k] != start[k - 1])
      return fail(BBX_ERR_INVALID, at("start", k) + " is not the first row "
                                       "of a contiguous tie group");
    if (end[k] < ne - 1 || end[k] >= n)
      return fail(BBX_ERR_INVALID, at("end", k) + " outside [n_event - 1, n)");
    if (k > 0 && end[k] > end[k - 1])
      return fail(BBX_ERR_INVALID, at("end", k) + " is increasing");
  }
  for (int64_t i = 0; i < n; ++i) {
    if (n_app[i] < 1 || n_app[i] > ne)
      return fail(BBX_ERR_INVALID, at("n_app", i) + " outside [1, n_event]");
    if (n_app[i] < ne && start[n_app[i]] != n_app[i])
      return fail(BBX_ERR_INVALID, at("n_app", i) + " does not end on a "
                                       "tie-group boundary");
  }
  std::vector<int32_t> grp((size_t)2 * ne);
  for (int64_t k = ne - 1, next = ne; k >= 0; --k) {
    grp[2 * k] = start[k] - 1;
    grp[2 * k + 1] = (int32_t)(next - 1);
    if (start[k] == k) next = k;
  }

  bbx_coxef* c = new bbx_coxef;
  const char* fam = CoxEfron::name;
  int st = cox_alloc(c, h, fam, ne, n, 2 * ne);
  if (st == BBX_OK)
    st = cox_upload(c, fam, c->grp, (const int2*)grp.data(), ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->end, end, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->napp, n_app, n);
  if (st == BBX_OK) st = cox_uploaded(c, fam);
  if (st != BBX_OK) return ham::discard(c, st);
  *out = c;
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_coxef_create(bbx_design* design, int64_t n_event,
                                const int32_t* start, const int32_t* end,
                                const int32_t* n_app, bbx_coxef** out) {
  return no_throw([&] {
    return coxef_create_impl(design, n_event, start, end, n_app, out);
  });
}

BBX_HAM_ENTRY_POINTS(coxef, CoxFamilyT<CoxEfron>)
BBX_COX_PREDICT_ENTRY_POINTS(coxef, CoxFamilyT<CoxEfron>)
