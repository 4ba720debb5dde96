// Fine-Gray subdistribution-hazard likelihood (competing risks), on the
// counting-process handle's row order and the plain handle's launch count.
// The preconditioned trajectory and the No-U-Turn tree are hamiltonian.hpp's.
//
// Every row has an observed time T and one of three statuses: event of
// interest, competing event, censored.  Rows are sorted by T ascending, at an
// equal T events, then competing, then censored rows.  Event k (k < ne, in
// time order) is row evrow[k].  Row i is in its risk set with weight 1 iff
// T_i >= t_k (whatever its status), and with weight G(t_k-) / G(T_i-) iff it
// had a competing event at T_i < t_k; G(s-) is the Kaplan-Meier estimate of the
// censoring survivor function from the left, formed by the caller on all its
// rows (Breslow ties: tied events share a set).  Arrays (host-built, checked
// by the create call):
//   a_k          the first row with T >= t_k
//   comp_row[j]  the competing rows, ascending; r_j = 1 / G(T-) of the j-th
//   b_k          the number of competing rows before row a_k
//   g_k          G(t_k-)
//   p_i          #{k : t_k <= T_i}  (0: a competing row before the first event)
// With eta = X~ beta, m = max eta, h_i = exp(eta_i - m):
//   E[i]   = sum_{l >= i} h_l                      suffix sum in row order
//   F[j]   = sum_{l <= j} h_{comp_row[l]} r_l      prefix sum, competing rows
//   H_k    = E[a_k] + (b_k > 0 ? g_k F[b_k - 1] : 0)
//   loglik = sum_k (eta_{evrow k} - m) - log H_k   (-inf if some H_k == 0)
//   inv_k  = 1/H_k,  c = cumsum inv,  sg[j] = sum_{k >= j} g_k inv_k (sg[ne] = 0)
//   A_i    = (p_i > 0 ? c[p_i - 1] : 0) + [i = comp_row[j]] r_j sg[p_i]
//   w_i    = [i is an event] - h_i A_i,  grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v, S_k as H_k from the
// same two scans of h u and (h u) r, z_k = inv_k (inv_k S_k), cz and sz as c
// and sg from z and g z, Z_i as A_i from them,
//   r_i = (h_i A_i) u_i - h_i Z_i,  out = X~^T (-r).
//
// No cancellation.  Every sum of the likelihood and the gradient is a sum of
// positive terms: sg is scanned as a suffix sum (the second event half
// reversed), never formed as cg[ne - 1] - cg[p - 1].  H_k == 0 is an empty
// risk-set sum: CoxTraj::zero and skip are raised as the plain handle raises
// them.  A NaN stays a NaN.
//
// Rounding order.  h r is one product of the rounded h; (h u) r is formed in
// that order.  g_k F is rounded, then added to E.  1/H_k is rounded first and
// multiplied by g_k (not g_k / H_k); z_k is formed innermost first and then
// multiplied by g_k.  r_j sg[p_i] is rounded, then added to c[p_i - 1].
// Without competing rows nothing is multiplied and H_k and c are the
// counting-process handle's without late entries.
//
// The kernels, their partition and reductions, the six launches and the
// family are cox_family.hpp's; this file states the formulae above as its
// policy (CoxFineGray), the index checks and the C entry points.
//
// Scans: the fixed partition and pass B of cox_scan.hpp.  E and F are the two
// segments of one blocked scan over a buffer of n + nc values (row order
// reversed, then the competing rows forward: pass A gathers the second
// through comp_row; it is not launched where nc = 0).  inv and g inv are
// elements k and ne + k of one buffer of 2 ne values: the event pass A
// gathers once per event and leaves the chunk sums of both halves, and one
// pass B gives c forward and sg as a suffix sum over the same chunks.
// Launches per likelihood, as the plain handle's: max, h pass A / B, 1/H pass
// A / B, weights.  No float atomics: the same inputs give the same bits on
// every run.
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_family.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

// One Fine-Gray likelihood on a design (borrowed: the design must outlive
// it).  The row-length buffers of CoxCore hold n + nc values, the event-length
// ones 2 ne: (1/H, g/H) or (z, g z), and their sums (c, sg).
struct bbx_coxfg : CoxCore {
  int64_t nc = 0;                        // competing rows
  DevMem evrow, a, b;                    // int32: ne
  DevMem crow, pc;                       // int32 nc, int2 n
  DevMem g, r;                           // double: ne, nc
  DevMem hu;                             // n + nc: h u
};

namespace {

// pc[i].y of a row that is no competing row
constexpr int32_t FG_CENSORED = -1, FG_EVENT = -2;

// The header's formulae as cox_family.hpp's kernels ask for them
struct CoxFineGray {
  using Handle = bbx_coxfg;
  static constexpr const char* name = "coxfg";
  static constexpr int halves = 2;       // inv and g inv; c and sg
  static constexpr int half_rev = 2;     // sg is a suffix sum
  static constexpr bool keeps_inv = false;
  const int32_t* evrow;
  const int32_t* a;
  const int32_t* b;
  const int32_t* crow;
  const int2* pc;                        // (p_i, j or FG_*), one 8-byte load
  const double* g;
  const double* r;
  int64_t n, ne;
  static CoxFineGray make(const bbx_coxfg* c) {
    return {c->evrow.as<const int32_t>(), c->a.as<const int32_t>(),
            c->b.as<const int32_t>(),     c->crow.as<const int32_t>(),
            c->pc.as<const int2>(),       c->g.as<const double>(),
            c->r.as<const double>(),      c->n, c->ne};
  }
  // E: the rows reversed; F: the competing rows forward (elements n ..
  // n + nc - 1), launched only where there are some
  static void risk_layout(const bbx_coxfg* c, int* nseg, int64_t* len,
                          int* rev) {
    *nseg = c->nc > 0 ? 2 : 1;
    len[0] = c->n, rev[0] = 1;
    len[1] = c->nc, rev[1] = 0;
  }
  static double* hu(bbx_coxfg* c) { return c->hu.as<double>(); }
  // element i < n is row i, element n + j is row comp_row[j]
  __device__ int64_t row(int s, int64_t i) const {
    return s == 0 ? i : (int64_t)crow[i - n];
  }
  __device__ double h_of(int64_t, double e) const { return e; }
  __device__ double risk_term(int s, int64_t i, double x) const {
    return s == 0 ? x : x * r[i - n];
  }
  __device__ double H(const double* scan, int64_t k, double& gk) const {
    const int32_t bk = b[k];
    gk = g[k];
    double H = scan[a[k]];
    if (bk > 0) H = H + gk * scan[n + bk - 1];
    return H;
  }
  __device__ bool empty(double H) const { return H == 0.; }
  __device__ int64_t event_row(int64_t k) const { return evrow[k]; }
  __device__ double scaled(double x, double) const { return x; }
  // c in cum[0, ne) and sg in cum[ne, 2 ne)
  template <bool HESS>
  __device__ void AZ(const double* c, const double* cz, int64_t i, double& A,
                     double& Z) const {
    const int2 k = pc[i];
    const int32_t p = k.x;
    A = p > 0 ? c[p - 1] : 0.;
    if (HESS) Z = p > 0 ? cz[p - 1] : 0.;
    if (k.y >= 0 && p < ne) {
      const double rj = r[k.y];
      A = A + rj * c[ne + p];
      if (HESS) Z = Z + rj * cz[ne + p];
    }
  }
  __device__ double indicator(int64_t i) const {
    return pc[i].y == FG_EVENT ? 1. : 0.;
  }
};

std::string at(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

int coxfg_create_impl(bbx_design* h, int64_t n_event, const int32_t* evrow,
                      const int32_t* a, const int32_t* b, const int32_t* p,
                      int64_t n_comp, const int32_t* comp_row,
                      const double* event_g, const double* comp_rinv,
                      bbx_coxfg** out) {
  BBX_TRY(cox_create_head(
      h, n_event,
      !evrow || !a || !b || !p || (n_comp > 0 && !comp_row)
          ? "NULL index array"
          : !event_g || (n_comp > 0 && !comp_rinv) ? "NULL factor array"
                                                   : nullptr,
      out));
  const int64_t n = h->n;
  const int64_t ne = n_event, nc = n_comp;
  if (nc < 0 || nc > n - ne)
    return fail(BBX_ERR_INVALID, "n_comp must be in [0, n - n_event]");
  // the kernels index eta[evrow], scan[a], scan[n + b - 1], eta[comp_row],
  // c[p - 1], sg[p], g[k] and r[j]: check them all
  // code[i]: FG_EVENT, FG_CENSORED or the number of competing row i
  std::vector<int32_t> code(n, FG_CENSORED);
  for (int64_t k = 0; k < ne; ++k) {
    if (evrow[k] < 0 || evrow[k] >= n)
      return fail(BBX_ERR_INVALID, at("evrow", k) + " outside [0, n)");
    if (k > 0 && evrow[k] <= evrow[k - 1])
      return fail(BBX_ERR_INVALID, at("evrow", k) + " is not increasing");
    if (a[k] < 0 || a[k] > evrow[k])
      return fail(BBX_ERR_INVALID, at("a", k) + " outside [0, evrow[k]]");
    if (k > 0 && a[k] < a[k - 1])
      return fail(BBX_ERR_INVALID, at("a", k) + " is decreasing");
    code[evrow[k]] = FG_EVENT;
  }
  for (int64_t j = 0; j < nc; ++j) {
    if (comp_row[j] < 0 || comp_row[j] >= n)
      return fail(BBX_ERR_INVALID, at("comp_row", j) + " outside [0, n)");
    if (j > 0 && comp_row[j] <= comp_row[j - 1])
      return fail(BBX_ERR_INVALID, at("comp_row", j) + " is not increasing");
    if (code[comp_row[j]] == FG_EVENT)
      return fail(BBX_ERR_INVALID, at("comp_row", j) + " is an event row");
    code[comp_row[j]] = (int32_t)j;
  }
  for (int64_t k = 0, j = 0; k < ne; ++k) {
    while (j < nc && comp_row[j] < a[k]) ++j;
    if (b[k] != j)
      return fail(BBX_ERR_INVALID, at("b", k) + " is not the number of "
                                       "competing rows before a[k]");
  }
  std::vector<int32_t> pc((size_t)2 * n);
  for (int64_t i = 0; i < n; ++i) {
    if (p[i] < (code[i] >= 0 ? 0 : 1) || p[i] > ne)
      return fail(BBX_ERR_INVALID,
                  at("p", i) + (code[i] >= 0 ? " outside [0, n_event]"
                                             : " outside [1, n_event]"));
    if (i > 0 && p[i] < p[i - 1])
      return fail(BBX_ERR_INVALID, at("p", i) + " is decreasing");
    pc[2 * i] = p[i];
    pc[2 * i + 1] = code[i];
  }
  for (int64_t k = 0; k < ne; ++k) {
    // !(x > 0) is true of a NaN too
    if (!(event_g[k] > 0.) || !(event_g[k] <= 1.))
      return fail(BBX_ERR_INVALID, at("event_g", k) + " is not in (0, 1]");
  }
  for (int64_t j = 0; j < nc; ++j) {
    if (!(comp_rinv[j] >= 1.) || isinf(comp_rinv[j]))
      return fail(BBX_ERR_INVALID, at("comp_rinv", j) +
                                       " is not a finite number >= 1");
  }

  bbx_coxfg* c = new bbx_coxfg;
  c->nc = nc;
  const char* fam = CoxFineGray::name;
  int st = cox_alloc(c, h, fam, ne, n + nc, 2 * ne);
  if (st == BBX_OK) st = c->hu.alloc(sizeof(double) * (n + nc));
  if (st == BBX_OK) st = cox_upload(c, fam, c->evrow, evrow, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->a, a, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->b, b, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->g, event_g, ne);
  if (st == BBX_OK) st = cox_upload(c, fam, c->pc, pc.data(), 2 * n);
  if (nc > 0) {
    if (st == BBX_OK) st = cox_upload(c, fam, c->crow, comp_row, nc);
    if (st == BBX_OK) st = cox_upload(c, fam, c->r, comp_rinv, nc);
  }
  if (st == BBX_OK) st = cox_uploaded(c, fam);
  if (st != BBX_OK) return ham::discard(c, st);
  *out = c;
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_coxfg_create(bbx_design* design, int64_t n_event,
                                const int32_t* evrow, const int32_t* a,
                                const int32_t* b, const int32_t* p,
                                int64_t n_comp, const int32_t* comp_row,
                                const double* event_g, const double* comp_rinv,
                                bbx_coxfg** out) {
  return no_throw([&] {
    return coxfg_create_impl(design, n_event, evrow, a, b, p, n_comp, comp_row,
                             event_g, comp_rinv, out);
  });
}

BBX_HAM_ENTRY_POINTS(coxfg, CoxFamilyT<CoxFineGray>)
BBX_COX_PREDICT_ENTRY_POINTS(coxfg, CoxFamilyT<CoxFineGray>)
