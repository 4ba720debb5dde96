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
#include "cox_scan.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// Pass A over the risk segments: h = exp(eta - m) (HU = false) or h u, stored
// in val, and one sum per chunk.
template <bool HU>
__global__ __launch_bounds__(SCAN_BLOCK) void coxef_risk_sum_kernel(
    Segs sg, const double* __restrict__ eta, const double* __restrict__ maxp,
    const double* __restrict__ h, const double* __restrict__ u,
    double* __restrict__ val, double* __restrict__ csum,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int s = blockIdx.x / SCAN_G, b = blockIdx.x % SCAN_G;
  const int64_t len = sg.len[s];
  const int64_t L = (len + SCAN_G - 1) / SCAN_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < len ? t0 + L : len;
  double m = 0.;
  if (!HU) m = part_max(maxp);
  double acc = 0.;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += SCAN_BLOCK) {
    const int64_t i = seg_elem(sg, s, t);
    const double v = HU ? h[i] * u[i] : exp(eta[i] - m);
    val[i] = v;
    acc += v;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (threadIdx.x == 0) csum[blockIdx.x] = acc;
}

struct EfArgs {
  const double* eta = nullptr;    // likelihood mode
  const double* maxp = nullptr;   // NPART partials of max eta
  const double* scan = nullptr;   // E in [0, ne), C in [ne, n)
  const double* inv = nullptr;    // Hessian mode: 1 / phi at the location
  const int2* grp = nullptr;      // (s - 1, s + d - 1) of every event
  const int32_t* end = nullptr;
  int64_t ne = 0;
  double* val = nullptr;          // 2 ne: the value, (l/d) times the value
  double* llpart = nullptr;       // likelihood mode: SCAN_G loglik partials
  CoxTraj* st = nullptr;          // likelihood mode: zero / skip flags
};

// Pass A over the events, SCAN_G blocks: phi_k = R_g + a_k T_g from one
// gather, 1/phi_k (HESS: inv_k (inv_k S_k)) into element k and l/d times it
// into element ne + k, and the chunk sums of both halves.
template <bool HESS>
__global__ __launch_bounds__(SCAN_BLOCK) void coxef_event_sum_kernel(
    EfArgs a, double* __restrict__ csum, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int b = blockIdx.x;
  const int64_t len = a.ne;
  const int64_t L = (len + SCAN_G - 1) / SCAN_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < len ? t0 + L : len;
  double m = 0.;
  if (!HESS) m = part_max(a.maxp);
  double acc = 0., accb = 0., ll = 0.;
  bool zero = false;
  for (int64_t k = t0 + threadIdx.x; k < t1; k += SCAN_BLOCK) {
    const int2 g = a.grp[k];
    const int32_t e = a.end[k];
    const int64_t s = (int64_t)g.x + 1, next = (int64_t)g.y + 1;
    const double En = next < a.ne ? a.scan[next] : 0.;
    const double T = a.scan[s] - En;
    double R = En;
    if (e >= a.ne) R += a.scan[e];
    const double lf = (double)(k - s) / (double)(next - s);
    const double phi = R + (1. - lf) * T;
    double v;
    if (!HESS) {
      zero |= (phi <= 0.);
      v = 1. / phi;
      ll += (a.eta[k] - m) - log(phi);
    } else {
      const double iv = a.inv[k];
      v = iv * (iv * phi);
    }
    const double vb = lf * v;
    a.val[k] = v;
    a.val[a.ne + k] = vb;
    acc += v;
    accb += vb;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  accb = block_sum<SCAN_BLOCK>(accb);
  if (!HESS) {
    ll = block_sum<SCAN_BLOCK>(ll);
    if (zero) {
      a.st->zero = 1;
      a.st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    csum[b] = acc;
    csum[SCAN_G + b] = accb;
    if (!HESS) a.llpart[b] = ll;
  }
}

// A_i = c[n_app_i - 1] - [i < ne] (cb[s_i + d_i - 1] - cb[s_i - 1]), c in
// cum[0, ne) and cb in cum[ne, 2 ne):
// w = [i < ne] - h_i A_i                              (HESS = false: gradient)
// w = -((h_i A_i) u_i - h_i Z_i), Z as A from cz      (HESS = true)
// and the NPART partials of sum(w).  grp: (s - 1, s + d - 1), one 8-byte load.
template <bool HESS>
__global__ __launch_bounds__(VEC_BLOCK) void coxef_weight_kernel(
    int64_t n, int64_t ne, const double* __restrict__ h,
    const double* __restrict__ c, const int32_t* __restrict__ napp,
    const int2* __restrict__ grp, const double* __restrict__ u,
    const double* __restrict__ cz, double* __restrict__ w,
    double* __restrict__ part, const int* __restrict__ skip) {
  if (skip && *skip) return;
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK) {
    const int32_t k = napp[i] - 1;
    const double hi = h[i];
    double A = c[k], Z = HESS ? cz[k] : 0.;
    if (i < ne) {
      const int2 g = grp[i];
      A = A - (c[ne + g.y] - (g.x >= 0 ? c[ne + g.x] : 0.));
      if (HESS) Z = Z - (cz[ne + g.y] - (g.x >= 0 ? cz[ne + g.x] : 0.));
    }
    const double rs = hi * A;
    double v;
    if (HESS) {
      v = -(rs * u[i] - hi * Z);
    } else {
      v = (i < ne ? 1. : 0.) - rs;
    }
    w[i] = v;
    acc += v;
  }
  acc = block_sum<VEC_BLOCK>(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

}  // namespace bbx

using namespace bbx;

// One Cox likelihood with Efron ties on a design (borrowed: the design must
// outlive it).
struct bbx_coxef : HamCore {
  int64_t ne = 0;
  DevMem grp, end, napp;                 // int2 ne, int32 ne, int32 n
  DevMem hz, scan;                       // n: h, risk scan (tmp: w / h u)
  DevMem inv, cs;                        // 2 ne: (1/phi, l/d 1/phi) or z; cumsums
  DevMem h_loc, inv_loc, c_loc;          // the Hessian's location: n, 2 ne, 2 ne
  DevMem csum, maxp;                     // 2 SCAN_G, NPART
};

namespace {

using ham::cst;
using ham::eta_of;
using ham::read_state;

// E: the events reversed; C: the censored rows forward
Segs risk_segs(const bbx_coxef* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 1;
  sg.base[1] = c->ne;
  sg.len[1] = c->n - c->ne;
  sg.rev[1] = 0;
  return sg;
}

// c: elements 0 .. ne - 1; cb: elements ne .. 2 ne - 1, both forward
Segs event_segs(const bbx_coxef* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 0;
  sg.base[1] = c->ne;
  sg.len[1] = c->ne;
  sg.rev[1] = 0;
  return sg;
}

template <bool HU>
int launch_risk_sum(bbx_coxef* c, const Segs& sg, const double* eta,
                    const double* h, const double* u, double* val,
                    const int* skip) {
  BBX_LAUNCH(coxef_risk_sum_kernel<HU>, dim3(2 * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, eta, c->maxp.as<const double>(), h, u, val,
             c->csum.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <bool HESS>
int launch_event_sum(bbx_coxef* c, const EfArgs& a, const int* skip) {
  BBX_LAUNCH(coxef_event_sum_kernel<HESS>, dim3(SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, a, c->csum.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

int launch_scan_out(bbx_coxef* c, const Segs& sg, const double* val,
                    double* out, const int* skip) {
  BBX_LAUNCH(cox_scan_out_kernel, dim3(2 * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, val, out, c->csum.as<const double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

EfArgs event_args(const bbx_coxef* c) {
  EfArgs b;
  b.scan = c->scan.as<double>();
  b.grp = c->grp.as<int2>();
  b.end = c->end.as<int32_t>();
  b.ne = c->ne;
  return b;
}

// From eta (already in c->eta, complete in stream order): h, phi, the loglik
// partials, (1/phi, l/d 1/phi) into `inv` and their cumsums (c, cb) into
// `cum`, then (grad != null) w and grad = X~^T w.  `h_out`: where h goes
// (c->hz or the location's).
int likelihood_from_eta(bbx_coxef* c, double* h_out, double* inv, double* cum,
                        double* grad) {
  bbx_design* h = c->h;
  const int* skip = &cst(c)->skip;
  BBX_LAUNCH(cox_max_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream, c->n,
             c->eta.as<const double>(), c->maxp.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  const Segs rs = risk_segs(c), es = event_segs(c);
  BBX_TRY(launch_risk_sum<false>(c, rs, c->eta.as<const double>(), nullptr,
                                 nullptr, h_out, skip));
  BBX_TRY(launch_scan_out(c, rs, h_out, c->scan.as<double>(), skip));
  EfArgs b = event_args(c);
  b.eta = c->eta.as<double>();
  b.maxp = c->maxp.as<double>();
  b.val = inv;
  b.llpart = c->llpart.as<double>();
  b.st = cst(c);
  BBX_TRY(launch_event_sum<false>(c, b, skip));
  BBX_TRY(launch_scan_out(c, es, inv, cum, skip));
  if (!grad) return BBX_OK;
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxef_weight_kernel<false>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->ne, h_out, cum, c->napp.as<const int32_t>(),
             c->grp.as<const int2>(), nullptr, nullptr, c->tmp.as<double>(),
             sumw, skip);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, grad);
}

std::string at(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

int coxef_create_impl(bbx_design* h, int64_t n_event, const int32_t* start,
                      const int32_t* end, const int32_t* n_app,
                      bbx_coxef** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!start || !end || !n_app)
    return fail(BBX_ERR_INVALID, "NULL index array");
  const int64_t n = h->n;
  if (n >= (int64_t(1) << 31))
    return fail(BBX_ERR_INVALID, "the Cox model needs fewer than 2^31 rows");
  if (n_event < 1 || n_event > n)
    return fail(BBX_ERR_INVALID, "n_event must be in [1, n]");
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
  c->ne = ne;
  const size_t d8 = sizeof(double), i4 = sizeof(int32_t);
  int st = ham::init_core(c, h, "coxef");
  DevMem* nvec[] = {&c->hz, &c->scan, &c->h_loc};
  for (DevMem* m : nvec)
    if (st == BBX_OK) st = m->alloc(d8 * n);
  DevMem* evec[] = {&c->inv, &c->cs, &c->inv_loc, &c->c_loc};
  for (DevMem* m : evec)
    if (st == BBX_OK) st = m->alloc(d8 * 2 * ne);
  if (st == BBX_OK) st = c->grp.alloc(i4 * 2 * ne);
  if (st == BBX_OK) st = c->end.alloc(i4 * ne);
  if (st == BBX_OK) st = c->napp.alloc(i4 * n);
  if (st == BBX_OK) st = c->csum.alloc(d8 * 2 * SCAN_G);
  if (st == BBX_OK) st = c->maxp.alloc(d8 * NPART);
  if (st != BBX_OK) return ham::discard(c, st);
  const hipMemcpyKind H2D = hipMemcpyHostToDevice;
  hipError_t e = hipMemcpyAsync(c->grp.ptr, grp.data(), i4 * 2 * ne, H2D,
                                h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->end.ptr, end, i4 * ne, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->napp.ptr, n_app, i4 * n, H2D, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("coxef upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

// The Cox block of a leapfrog step: everything from eta to X~^T w
struct CoxEfLik {
  bbx_coxef* c;
  int operator()(double* grad) const {
    return likelihood_from_eta(c, c->hz.as<double>(), c->inv.as<double>(),
                               c->cs.as<double>(), grad);
  }
};

struct CoxEfFamily {
  static constexpr const char* name = "coxef";
  using Lik = CoxEfLik;
  static int locate(bbx_coxef* c, const double* d_in) {
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
  static int hessian_from_v(bbx_coxef* c, const double* d_v, double* d_out);
};

int CoxEfFamily::hessian_from_v(bbx_coxef* c, const double* d_v,
                                double* d_out) {
  bbx_design* h = c->h;
  BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
  BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
  const Segs rs = risk_segs(c), es = event_segs(c);
  BBX_TRY(launch_risk_sum<true>(c, rs, nullptr, c->h_loc.as<const double>(),
                                c->eta.as<const double>(), c->tmp.as<double>(),
                                nullptr));
  BBX_TRY(launch_scan_out(c, rs, c->tmp.as<double>(), c->scan.as<double>(),
                          nullptr));
  EfArgs b = event_args(c);
  b.inv = c->inv_loc.as<double>();
  b.val = c->inv.as<double>();
  BBX_TRY(launch_event_sum<true>(c, b, nullptr));
  BBX_TRY(launch_scan_out(c, es, c->inv.as<double>(), c->cs.as<double>(),
                          nullptr));
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxef_weight_kernel<true>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->ne, c->h_loc.as<const double>(),
             c->c_loc.as<const double>(), c->napp.as<const int32_t>(),
             c->grp.as<const int2>(), c->eta.as<const double>(),
             c->cs.as<const double>(), c->tmp.as<double>(), sumw, nullptr);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, d_out);
}

}  // namespace

extern "C" int bbx_coxef_create(bbx_design* design, int64_t n_event,
                                const int32_t* start, const int32_t* end,
                                const int32_t* n_app, bbx_coxef** out) {
  return no_throw([&] {
    return coxef_create_impl(design, n_event, start, end, n_app, out);
  });
}

BBX_HAM_ENTRY_POINTS(coxef, CoxEfFamily)
