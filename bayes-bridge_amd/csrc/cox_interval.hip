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
// Scans: the fixed partition and pass B of cox_scan.hpp; E and F are the two
// segments of one blocked scan over a buffer of 2 n values (row order, then
// entry order: pass A gathers the second copy through entry_perm).  Launches
// per likelihood, as the plain handle's: max, h pass A / B, 1/H pass A / B,
// weights.  No float atomics: the same inputs give the same bits on every run.
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_scan.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

enum CpMode {
  CP_H = 0,     // h = exp(eta - m)                  (row order, entry order)
  CP_HU = 1,    // h u                               (row order, entry order)
  CP_INVH = 2,  // 1 / H_k, and the loglik partials  (events, forward)
  CP_WU = 3     // (1/H_k) ((1/H_k) S_k)             (events, forward)
};

struct CpArgs {
  const double* eta = nullptr;     // CP_H, CP_INVH
  const double* maxp = nullptr;    // NPART partials of max eta
  const double* h = nullptr;       // CP_HU
  const double* u = nullptr;       // CP_HU
  const double* scan = nullptr;    // CP_INVH, CP_WU: E in [0, n), F in [n, 2n)
  const double* inv = nullptr;     // CP_WU: 1 / H at the location
  const int32_t* perm = nullptr;   // CP_H, CP_HU: entry_perm
  const int32_t* evrow = nullptr;  // CP_INVH
  const int32_t* a = nullptr;
  const int32_t* b = nullptr;
  int64_t n = 0;
  double* val = nullptr;           // the per-element value, stored
  double* llpart = nullptr;        // CP_INVH: SCAN_G loglik partials
  CoxTraj* st = nullptr;           // CP_INVH: zero / skip flags
};

// Pass A: the value of every element of every chunk (stored in a.val) and one
// sum per chunk.  CP_H / CP_HU: element i < n is row i, element n + j is row
// entry_perm[j].
template <int MODE>
__global__ __launch_bounds__(SCAN_BLOCK) void coxcp_scan_sum_kernel(
    Segs sg, CpArgs a, double* __restrict__ csum,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int s = blockIdx.x / SCAN_G, b = blockIdx.x % SCAN_G;
  const int64_t len = sg.len[s];
  const int64_t L = (len + SCAN_G - 1) / SCAN_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < len ? t0 + L : len;
  double m = 0.;
  if (MODE == CP_H || MODE == CP_INVH) m = part_max(a.maxp);
  double acc = 0., ll = 0.;
  bool zero = false;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += SCAN_BLOCK) {
    const int64_t i = seg_elem(sg, s, t);
    double v;
    if (MODE == CP_H || MODE == CP_HU) {
      const int64_t r = s == 0 ? i : (int64_t)a.perm[i - a.n];
      v = MODE == CP_H ? exp(a.eta[r] - m) : a.h[r] * a.u[r];
    } else {
      const int32_t bk = a.b[i];
      double H = a.scan[a.a[i]];
      if (bk < a.n) H = H - a.scan[a.n + bk];
      if (MODE == CP_INVH) {
        zero |= (H <= 0.);
        v = 1. / H;
        ll += (a.eta[a.evrow[i]] - m) - log(H);
      } else {
        const double iv = a.inv[i];
        v = iv * (iv * H);
      }
    }
    a.val[i] = v;
    acc += v;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (MODE == CP_INVH) {
    ll = block_sum<SCAN_BLOCK>(ll);
    if (zero) {
      a.st->zero = 1;
      a.st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    csum[blockIdx.x] = acc;
    if (MODE == CP_INVH) a.llpart[b] = ll;
  }
}

// w = delta_i - h_i (c[p_i - 1] - c[q_i - 1])                (HESS = false)
// w = -((h_i (c[p_i-1] - c[q_i-1])) u_i - h_i (cz[p_i-1] - cz[q_i-1]))
// and the NPART partials of sum(w).  pq: (p_i, q_i) pairs, one 8-byte load.
template <bool HESS>
__global__ __launch_bounds__(VEC_BLOCK) void coxcp_weight_kernel(
    int64_t n, const double* __restrict__ h, const double* __restrict__ c,
    const int2* __restrict__ pq, const uint8_t* __restrict__ delta,
    const double* __restrict__ u, const double* __restrict__ cz,
    double* __restrict__ w, double* __restrict__ part,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK) {
    const int2 k = pq[i];
    const int32_t p = k.x - 1, q = k.y - 1;
    const double hi = h[i];
    const double rs = hi * (c[p] - (q >= 0 ? c[q] : 0.));
    double v;
    if (HESS) {
      v = -(rs * u[i] - hi * (cz[p] - (q >= 0 ? cz[q] : 0.)));
    } else {
      v = (delta[i] ? 1. : 0.) - rs;
    }
    w[i] = v;
    acc += v;
  }
  acc = block_sum<VEC_BLOCK>(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

}  // namespace bbx

using namespace bbx;

// One counting-process Cox likelihood on a design (borrowed: the design must
// outlive it).
struct bbx_coxcp : HamCore {
  int64_t ne = 0;
  int nseg = 1;                          // 2 where some row enters late
  DevMem evrow, a, b;                    // int32: ne
  DevMem perm, pq, delta;                // int32 n, int2 n, uint8 n
  DevMem hz, scan, hu;                   // nseg n: h, (E, F), h u
  DevMem inv, cs;                        // ne: 1/H (or z), cumsum
  DevMem h_loc, inv_loc, c_loc;          // the Hessian's location: nseg n, ne, ne
  DevMem csum, maxp;                     // 2 SCAN_G, NPART
};

namespace {

using ham::cst;
using ham::eta_of;
using ham::read_state;

// E: the rows reversed; F: the entry order reversed (elements n .. 2n - 1)
Segs risk_segs(const bbx_coxcp* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->n;
  sg.rev[0] = 1;
  sg.base[1] = c->n;
  sg.len[1] = c->nseg == 2 ? c->n : 0;
  sg.rev[1] = 1;
  return sg;
}

Segs event_segs(const bbx_coxcp* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 0;
  sg.base[1] = 0;
  sg.len[1] = 0;
  sg.rev[1] = 0;
  return sg;
}

template <int MODE>
int launch_scan_sum(bbx_coxcp* c, const Segs& sg, int nseg, const CpArgs& a,
                    const int* skip) {
  BBX_LAUNCH(coxcp_scan_sum_kernel<MODE>, dim3(nseg * SCAN_G),
             dim3(SCAN_BLOCK), 0, c->h->stream, sg, a, c->csum.as<double>(),
             skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

int launch_scan_out(bbx_coxcp* c, const Segs& sg, int nseg, const double* val,
                    double* out, const int* skip) {
  BBX_LAUNCH(cox_scan_out_kernel, dim3(nseg * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, val, out, c->csum.as<const double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

CpArgs event_args(const bbx_coxcp* c) {
  CpArgs b;
  b.scan = c->scan.as<double>();
  b.evrow = c->evrow.as<int32_t>();
  b.a = c->a.as<int32_t>();
  b.b = c->b.as<int32_t>();
  b.n = c->n;
  return b;
}

// From eta (already in c->eta, complete in stream order): h, H, the loglik
// partials, 1/H into `inv` and c = cumsum(1/H) into `cum`, then (grad != null)
// w and grad = X~^T w.  `h_out`: where h goes (c->hz or the location's).
int likelihood_from_eta(bbx_coxcp* c, double* h_out, double* inv, double* cum,
                        double* grad) {
  bbx_design* h = c->h;
  const int* skip = &cst(c)->skip;
  BBX_LAUNCH(cox_max_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream, c->n,
             c->eta.as<const double>(), c->maxp.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  const Segs rs = risk_segs(c), es = event_segs(c);
  CpArgs a;
  a.eta = c->eta.as<double>();
  a.maxp = c->maxp.as<double>();
  a.perm = c->perm.as<int32_t>();
  a.n = c->n;
  a.val = h_out;
  BBX_TRY(launch_scan_sum<CP_H>(c, rs, c->nseg, a, skip));
  BBX_TRY(launch_scan_out(c, rs, c->nseg, h_out, c->scan.as<double>(), skip));
  CpArgs b = event_args(c);
  b.eta = c->eta.as<double>();
  b.maxp = c->maxp.as<double>();
  b.val = inv;
  b.llpart = c->llpart.as<double>();
  b.st = cst(c);
  BBX_TRY(launch_scan_sum<CP_INVH>(c, es, 1, b, skip));
  BBX_TRY(launch_scan_out(c, es, 1, inv, cum, skip));
  if (!grad) return BBX_OK;
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxcp_weight_kernel<false>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, h_out, cum, c->pq.as<const int2>(),
             c->delta.as<const uint8_t>(), nullptr, nullptr,
             c->tmp.as<double>(), sumw, skip);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, grad);
}

std::string at(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

int coxcp_create_impl(bbx_design* h, int64_t n_event, const int32_t* evrow,
                      const int32_t* a, const int32_t* b, const int32_t* p,
                      const int32_t* q, const int32_t* entry_perm,
                      bbx_coxcp** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!evrow || !a || !b || !p || !q || !entry_perm)
    return fail(BBX_ERR_INVALID, "NULL index array");
  const int64_t n = h->n;
  if (n >= (int64_t(1) << 31))
    return fail(BBX_ERR_INVALID, "the Cox model needs fewer than 2^31 rows");
  if (n_event < 1 || n_event > n)
    return fail(BBX_ERR_INVALID, "n_event must be in [1, n]");
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
  c->ne = ne;
  c->nseg = delayed ? 2 : 1;
  const size_t d8 = sizeof(double), i4 = sizeof(int32_t);
  int st = ham::init_core(c, h, "coxcp");
  DevMem* nvec[] = {&c->hz, &c->scan, &c->hu, &c->h_loc};
  for (DevMem* m : nvec)
    if (st == BBX_OK) st = m->alloc(d8 * n * c->nseg);
  DevMem* evec[] = {&c->inv, &c->cs, &c->inv_loc, &c->c_loc};
  for (DevMem* m : evec)
    if (st == BBX_OK) st = m->alloc(d8 * ne);
  DevMem* eidx[] = {&c->evrow, &c->a, &c->b};
  for (DevMem* m : eidx)
    if (st == BBX_OK) st = m->alloc(i4 * ne);
  if (st == BBX_OK) st = c->perm.alloc(i4 * n);
  if (st == BBX_OK) st = c->pq.alloc(i4 * 2 * n);
  if (st == BBX_OK) st = c->delta.alloc(n);
  if (st == BBX_OK) st = c->csum.alloc(d8 * 2 * SCAN_G);
  if (st == BBX_OK) st = c->maxp.alloc(d8 * NPART);
  if (st != BBX_OK) return ham::discard(c, st);
  const hipMemcpyKind H2D = hipMemcpyHostToDevice;
  hipError_t e = hipMemcpyAsync(c->evrow.ptr, evrow, i4 * ne, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->a.ptr, a, i4 * ne, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->b.ptr, b, i4 * ne, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->perm.ptr, entry_perm, i4 * n, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->pq.ptr, pq.data(), i4 * 2 * n, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->delta.ptr, delta.data(), n, H2D, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("coxcp upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

// The Cox block of a leapfrog step: everything from eta to X~^T w
struct CoxCpLik {
  bbx_coxcp* c;
  int operator()(double* grad) const {
    return likelihood_from_eta(c, c->hz.as<double>(), c->inv.as<double>(),
                               c->cs.as<double>(), grad);
  }
};

struct CoxCpFamily {
  static constexpr const char* name = "coxcp";
  using Lik = CoxCpLik;
  static int locate(bbx_coxcp* c, const double* d_in) {
    BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, c->h->stream, cst(c));
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(likelihood_from_eta(c, c->h_loc.as<double>(),
                                c->inv_loc.as<double>(), c->c_loc.as<double>(),
                                nullptr));
    BBX_TRY(read_state(c));
    if (c->host_st->zero)
      return fail(BBX_ERR_NUMERIC,
                  "Hessian location: a risk-set sum of relative hazards is 0");
    return BBX_OK;
  }
  static int hessian_from_v(bbx_coxcp* c, const double* d_v, double* d_out);
};

int CoxCpFamily::hessian_from_v(bbx_coxcp* c, const double* d_v,
                                double* d_out) {
  bbx_design* h = c->h;
  BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
  BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
  const Segs rs = risk_segs(c), es = event_segs(c);
  CpArgs a;
  a.h = c->h_loc.as<double>();
  a.u = c->eta.as<double>();
  a.perm = c->perm.as<int32_t>();
  a.n = c->n;
  a.val = c->hu.as<double>();
  BBX_TRY(launch_scan_sum<CP_HU>(c, rs, c->nseg, a, nullptr));
  BBX_TRY(launch_scan_out(c, rs, c->nseg, c->hu.as<double>(),
                          c->scan.as<double>(), nullptr));
  CpArgs b = event_args(c);
  b.inv = c->inv_loc.as<double>();
  b.val = c->inv.as<double>();
  BBX_TRY(launch_scan_sum<CP_WU>(c, es, 1, b, nullptr));
  BBX_TRY(launch_scan_out(c, es, 1, c->inv.as<double>(), c->cs.as<double>(),
                          nullptr));
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxcp_weight_kernel<true>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->h_loc.as<const double>(),
             c->c_loc.as<const double>(), c->pq.as<const int2>(),
             c->delta.as<const uint8_t>(), c->eta.as<const double>(),
             c->cs.as<const double>(), c->tmp.as<double>(), sumw, nullptr);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, d_out);
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

BBX_HAM_ENTRY_POINTS(coxcp, CoxCpFamily)
