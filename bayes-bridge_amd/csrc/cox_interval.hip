// Cox partial likelihood in counting-process form: every row is at risk on
// (entry_i, exit_i], so a subject may enter late (left truncation) or be
// written as several (start, stop] rows with covariates that change.  The
// preconditioned trajectory and the No-U-Turn tree are hamiltonian.hpp's.
//
// Rows are sorted by exit time x ascending, events before censored rows at an
// equal exit.  Event k (k < ne, in time order) is row evrow[k]; row i is in
// its risk set iff e_i < t_k <= x_i (Breslow ties: tied events share a set).
// Index arrays (host-built, checked by the create call):
//   entry_perm[j]  the rows in ascending entry order
//   a_k            the first row with x >= t_k
//   b_k            the first position in entry order with e >= t_k (may be n)
//   p_i, q_i       #{k : t_k <= x_i}, #{k : t_k <= e_i}   (q_i < p_i)
// With eta = X~ beta, m = max eta, h_i = exp(eta_i - m):
//   E[i]   = sum_{r >= i} h_r                  suffix sum in row order
//   F[j]   = sum_{l >= j} h_{entry_perm[l]}    suffix sum in entry order
//   H_k    = E[a_k] - (b_k < n ? F[b_k] : 0)
//   loglik = sum_k (eta_k - m) - log H_k       (-inf if some H_k <= 0)
//   c      = cumsum_k 1/H_k
//   w_i    = delta_i - h_i (c[p_i - 1] - c[q_i - 1])   (c[-1] = 0), grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v, S_k from the same two
// scans of h u, z_k = (1/H_k) ((1/H_k) S_k), cz = cumsum z,
//   r_i = (h_i (c[p_i-1] - c[q_i-1])) u_i - h_i (cz[p_i-1] - cz[q_i-1]),
//   out = X~^T (-r).
//
// Cancellation.  Every row with e >= t_k has x > t_k, so F[b_k] sums a subset
// of E[a_k]'s rows and H_k > 0 in exact arithmetic; in floating point the
// relative error of H_k is about eps E / H.  H_k <= 0 is treated as the plain
// handle treats an empty risk-set sum: CoxTraj::zero and skip are raised.
// Where no row enters late (b_k = n for every k) nothing is subtracted, the
// entry-order segment is not launched and H_k is the plain suffix sum.
//
// The kernels, their partition and reductions, the six launches and the
// family are cox_family.hpp's; this file states the formulae above as its
// policy (CoxEntry), the index checks and the C entry points.
//
// Scans: the fixed partition and pass B of cox_scan.hpp; E and F are the two
// segments of one blocked scan over a buffer of 2 n values (row order, then
// entry order: pass A gathers the second copy through entry_perm).  Launches
// per likelihood, as the plain handle's: max, h pass A / B, 1/H pass A / B,
// weights.  No float atomics: the same inputs give the same bits on every run.
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_family.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One counting-process Cox likelihood on a design (borrowed: the design must
// outlive it).  The row-length buffers of CoxCore hold nseg n values.
struct bbx_coxcp : CoxCore {
  int nseg = 1;                          // 2 where some row enters late
  DevMem evrow, a, b;                    // int32: ne
  DevMem perm, pq, delta;                // int32 n, int2 n, uint8 n
  DevMem hu;                             // nseg n: h u
};

namespace {

// The header's formulae as cox_family.hpp's kernels ask for them
struct CoxEntry {
  using Handle = bbx_coxcp;
  static constexpr const char* name = "coxcp";
  static constexpr int halves = 1;
  static constexpr bool keeps_inv = false;
  const int32_t* perm;
  const int32_t* evrow;
  const int32_t* a;
  const int32_t* b;
  const int2* pq;                        // (p_i, q_i) pairs, one 8-byte load
  const uint8_t* delta;
  int64_t n;
  static CoxEntry make(const bbx_coxcp* c) {
    return {c->perm.as<const int32_t>(), c->evrow.as<const int32_t>(),
            c->a.as<const int32_t>(),    c->b.as<const int32_t>(),
            c->pq.as<const int2>(),      c->delta.as<const uint8_t>(), c->n};
  }
  // E: the rows reversed; F: the entry order reversed (elements n .. 2n - 1),
  // launched only where some row enters late
  static void risk_layout(const bbx_coxcp* c, int* nseg, int64_t* len,
                          int* rev) {
    *nseg = c->nseg;
    len[0] = c->n, rev[0] = 1;
    len[1] = c->nseg == 2 ? c->n : 0, rev[1] = 1;
  }
  static double* hu(bbx_coxcp* c) { return c->hu.as<double>(); }
  // element i < n is row i, element n + j is row entry_perm[j]
  __device__ int64_t row(int s, int64_t i) const {
    return s == 0 ? i : (int64_t)perm[i - n];
  }
  __device__ double h_of(int64_t, double e) const { return e; }
  __device__ double risk_term(int, int64_t, double x) const { return x; }
  __device__ double H(const double* scan, int64_t k, double&) const {
    const int32_t bk = b[k];
    double H = scan[a[k]];
    if (bk < n) H = H - scan[n + bk];
    return H;
  }
  __device__ bool empty(double H) const { return H <= 0.; }
  __device__ int64_t event_row(int64_t k) const { return evrow[k]; }
  __device__ double scaled(double x, double) const { return x; }
  template <bool HESS>
  __device__ void AZ(const double* c, const double* cz, int64_t i, double& A,
                     double& Z) const {
    const int2 k = pq[i];
    const int32_t p = k.x - 1, q = k.y - 1;
    A = c[p] - (q >= 0 ? c[q] : 0.);
    if (HESS) Z = cz[p] - (q >= 0 ? cz[q] : 0.);
  }
  __device__ double indicator(int64_t i) const { return delta[i] ? 1. : 0.; }
};

std::string at(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

int coxcp_create_impl(bbx_design* h, int64_t n_event, const int32_t* evrow,
                      const int32_t* a, const int32_t* b, const int32_t* p,
                      const int32_t* q, const int32_t* entry_perm,
                      bbx_coxcp** out) {
  BBX_TRY(cox_create_head(h, n_event,
                          evrow && a && b && p && q && entry_perm
                              ? nullptr
                              : "NULL index array",
                          out));
  const int64_t n = h->n;
  const int64_t ne = n_event;
  // the kernels index eta[evrow], scan[a], scan[n + b], eta[entry_perm],
  // c[p - 1] and c[q - 1]: check them all
  bool delayed = false;
  for (int64_t k = 0; k < ne; ++k) {
    if (evrow[k] < 0 || evrow[k] >= n)
      return fail(BBX_ERR_INVALID, at("evrow", k) + " outside [0, n)");
    if (k > 0 && evrow[k] <= evrow[k - 1])
      return fail(BBX_ERR_INVALID, at("evrow", k) + " is not increasing");
    if (a[k] < 0 || a[k] > evrow[k])
      return fail(BBX_ERR_INVALID, at("a", k) + " outside [0, evrow[k]]");
    if (b[k] < 0 || b[k] > n)
      return fail(BBX_ERR_INVALID, at("b", k) + " outside [0, n]");
    if (k > 0 && a[k] < a[k - 1])
      return fail(BBX_ERR_INVALID, at("a", k) + " is decreasing");
    if (k > 0 && b[k] < b[k - 1])
      return fail(BBX_ERR_INVALID, at("b", k) + " is decreasing");
    if (a[k] >= b[k])
      return fail(BBX_ERR_INVALID, "risk set " + std::to_string(k) +
                                       " is empty (a[k] >= b[k])");
    delayed |= b[k] < n;
  }
  std::vector<uint8_t> seen(n, 0), delta(n, 0);
  for (int64_t j = 0; j < n; ++j) {
    const int32_t r = entry_perm[j];
    if (r < 0 || r >= n || seen[r])
      return fail(BBX_ERR_INVALID, "entry_perm is not a permutation (" +
                                       at("entry_perm", j) + ")");
    seen[r] = 1;
  }
  std::vector<int32_t> pq((size_t)2 * n);
  for (int64_t i = 0; i < n; ++i) {
    if (p[i] < 1 || p[i] > ne)
      return fail(BBX_ERR_INVALID, at("p", i) + " outside [1, n_event]");
    if (i > 0 && p[i] < p[i - 1])
      return fail(BBX_ERR_INVALID, at("p", i) + " is decreasing");
    if (q[i] < 0 || q[i] >= p[i])
      return fail(BBX_ERR_INVALID, at("q", i) + " outside [0, p[i])");
    pq[2 * i] = p[i];
    pq[2 * i + 1] = q[i];
  }
  for (int64_t j = 1; j < n; ++j) {
    if (q[entry_perm[j]] < q[entry_perm[j - 1]])
      return fail(BBX_ERR_INVALID, "q[" + at("entry_perm", j) +
                                       "] is decreasing in entry order");
  }
  for (int64_t k = 0; k < ne; ++k) delta[evrow[k]] = 1;

  bbx_coxcp* c = new bbx_coxcp;
  c->nseg = delayed ? 2 : 1;
  const char* fam = CoxEntry::name;
  int st = cox_alloc(c, h, fam, ne, n * c->nseg, ne);
  if (st == BBX_OK) st = c->hu.alloc(sizeof(double) * n * c->nseg);
  if (st == BBX_OK) st = cox_upload(c, fam, c->evrow, evrow, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->a, a, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->b, b, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->perm, entry_perm, n);
  if (st == BBX_OK) st = cox_upload(c, fam, c->pq, pq.data(), 2 * n);
  if (st == BBX_OK) st = cox_upload(c, fam, c->delta, delta.data(), n);
  if (st == BBX_OK) st = cox_uploaded(c, fam);
  if (st != BBX_OK) return ham::discard(c, st);
  *out = c;
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_coxcp_create(bbx_design* design, int64_t n_event,
                                const int32_t* evrow, const int32_t* a,
                                const int32_t* b, const int32_t* p,
                                const int32_t* q, const int32_t* entry_perm,
                                bbx_coxcp** out) {
  return no_throw([&] {
    return coxcp_create_impl(design, n_event, evrow, a, b, p, q, entry_perm,
                             out);
  });
}

BBX_HAM_ENTRY_POINTS(coxcp, CoxFamilyT<CoxEntry>)
BBX_COX_PREDICT_ENTRY_POINTS(coxcp, CoxFamilyT<CoxEntry>)
