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
// Scans: the fixed partition and pass B of cox_scan.hpp.  Launches per
// likelihood, as the plain handle's: max, g pass A / B, a/H pass A / B,
// weights.  The event pass reads a_k from the row vector (events are rows
// 0 .. ne - 1).  No float atomics: the same inputs give the same bits on every
// run.
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_scan.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// Pass A over the risk segments: g = a exp(eta - m) (HU = false) or g u,
// stored in val, and one sum per chunk.
template <bool HU>
__global__ __launch_bounds__(SCAN_BLOCK) void coxw_risk_sum_kernel(
    Segs sg, const double* __restrict__ eta, const double* __restrict__ maxp,
    const double* __restrict__ a, const double* __restrict__ g,
    const double* __restrict__ u, double* __restrict__ val,
    double* __restrict__ csum, const int* __restrict__ skip) {
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
    const double v = HU ? g[i] * u[i] : a[i] * exp(eta[i] - m);
    val[i] = v;
    acc += v;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (threadIdx.x == 0) csum[blockIdx.x] = acc;
}

struct CoxwArgs {
  const double* eta = nullptr;    // likelihood mode
  const double* maxp = nullptr;   // NPART partials of max eta
  const double* a = nullptr;      // the weights, in row order
  const double* scan = nullptr;   // risk-segment scan
  const double* inv = nullptr;    // Hessian mode: 1 / H at the location
  const int32_t* start = nullptr;
  const int32_t* end = nullptr;
  int64_t ne = 0;
  double* val = nullptr;          // a / H (Hessian mode: z), stored
  double* inv_out = nullptr;      // likelihood mode, optional: 1 / H, stored
  double* llpart = nullptr;       // likelihood mode: SCAN_G loglik partials
  CoxTraj* st = nullptr;          // likelihood mode: zero / skip flags
};

// Pass A over the events, SCAN_G blocks: H_k (HESS: S_k) from the risk scan,
// q_k = a_k (1/H_k) (HESS: z_k = a_k (inv_k (inv_k S_k))) stored in val, and
// one sum per chunk.
template <bool HESS>
__global__ __launch_bounds__(SCAN_BLOCK) void coxw_event_sum_kernel(
    CoxwArgs a, double* __restrict__ csum, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int b = blockIdx.x;
  const int64_t len = a.ne;
  const int64_t L = (len + SCAN_G - 1) / SCAN_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < len ? t0 + L : len;
  double m = 0.;
  if (!HESS) m = part_max(a.maxp);
  double acc = 0., ll = 0.;
  bool zero = false;
  for (int64_t k = t0 + threadIdx.x; k < t1; k += SCAN_BLOCK) {
    const int32_t e = a.end[k];
    double H = a.scan[a.start[k]];
    if (e >= a.ne) H += a.scan[e];
    const double ak = a.a[k];
    double v;
    if (!HESS) {
      zero |= (H == 0.);
      const double iv = 1. / H;
      if (a.inv_out) a.inv_out[k] = iv;
      v = ak * iv;
      ll += ak * ((a.eta[k] - m) - log(H));
    } else {
      const double iv = a.inv[k];
      v = ak * (iv * (iv * H));
    }
    a.val[k] = v;
    acc += v;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (!HESS) {
    ll = block_sum<SCAN_BLOCK>(ll);
    if (zero) {
      a.st->zero = 1;
      a.st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    csum[b] = acc;
    if (!HESS) a.llpart[b] = ll;
  }
}

// w = [i < ne] a_i - c[n_app_i - 1] g_i              (HESS = false: gradient)
// w = -((c[n_app_i - 1] g_i) u_i - g_i cz[n_app_i - 1])   (HESS = true)
// and the NPART partials of sum(w) (the Tdot's intercept / centring term).
template <bool HESS>
__global__ __launch_bounds__(VEC_BLOCK) void coxw_weight_kernel(
    int64_t n, int64_t ne, const double* __restrict__ a,
    const double* __restrict__ g, const double* __restrict__ c,
    const int32_t* __restrict__ napp, const double* __restrict__ u,
    const double* __restrict__ cz, double* __restrict__ w,
    double* __restrict__ part, const int* __restrict__ skip) {
  if (skip && *skip) return;
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK) {
    const int32_t k = napp[i] - 1;
    const double rs = c[k] * g[i];
    double v;
    if (HESS) {
      v = -(rs * u[i] - g[i] * cz[k]);
    } else {
      v = (i < ne ? a[i] : 0.) - rs;
    }
    w[i] = v;
    acc += v;
  }
  acc = block_sum<VEC_BLOCK>(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

}  // namespace bbx

using namespace bbx;

// One weighted Cox likelihood on a design (borrowed: the design must outlive
// it).
struct bbx_coxw : HamCore {
  int64_t ne = 0;
  DevMem start, end, napp;               // int32: ne, ne, n
  DevMem wt;                             // n: the case weights
  DevMem gz, scan;                       // n: g, risk scan (tmp: w / g u)
  DevMem inv, cs;                        // ne: a/H (or z), cumsum
  DevMem g_loc, inv_loc, c_loc;          // the Hessian's location: n, ne (1/H), ne
  DevMem csum, maxp;                     // 2 SCAN_G, NPART
};

namespace {

using ham::cst;
using ham::eta_of;
using ham::read_state;

Segs risk_segs(const bbx_coxw* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 1;
  sg.base[1] = c->ne;
  sg.len[1] = c->n - c->ne;
  sg.rev[1] = 0;
  return sg;
}

Segs event_segs(const bbx_coxw* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 0;
  sg.base[1] = 0;
  sg.len[1] = 0;
  sg.rev[1] = 0;
  return sg;
}

template <bool HU>
int launch_risk_sum(bbx_coxw* c, const Segs& sg, const double* eta,
                    const double* g, const double* u, double* val,
                    const int* skip) {
  BBX_LAUNCH(coxw_risk_sum_kernel<HU>, dim3(2 * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, eta, c->maxp.as<const double>(),
             c->wt.as<const double>(), g, u, val, c->csum.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <bool HESS>
int launch_event_sum(bbx_coxw* c, const CoxwArgs& a, const int* skip) {
  BBX_LAUNCH(coxw_event_sum_kernel<HESS>, dim3(SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, a, c->csum.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

int launch_scan_out(bbx_coxw* c, const Segs& sg, int nseg, const double* val,
                    double* out, const int* skip) {
  BBX_LAUNCH(cox_scan_out_kernel, dim3(nseg * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, val, out, c->csum.as<const double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

CoxwArgs event_args(const bbx_coxw* c) {
  CoxwArgs b;
  b.a = c->wt.as<double>();
  b.scan = c->scan.as<double>();
  b.start = c->start.as<int32_t>();
  b.end = c->end.as<int32_t>();
  b.ne = c->ne;
  return b;
}

// From eta (already in c->eta, complete in stream order): g, H, the loglik
// partials, a/H into `q` (and 1/H into `inv1` where given) and c = cumsum(a/H)
// into `cum`, then (grad != null) w and grad = X~^T w.  `g_out`: where g goes
// (c->gz or the location's).
int likelihood_from_eta(bbx_coxw* c, double* g_out, double* q, double* inv1,
                        double* cum, double* grad) {
  bbx_design* h = c->h;
  const int* skip = &cst(c)->skip;
  BBX_LAUNCH(cox_max_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream, c->n,
             c->eta.as<const double>(), c->maxp.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  const Segs rs = risk_segs(c), es = event_segs(c);
  BBX_TRY(launch_risk_sum<false>(c, rs, c->eta.as<const double>(), nullptr,
                                 nullptr, g_out, skip));
  BBX_TRY(launch_scan_out(c, rs, 2, g_out, c->scan.as<double>(), skip));
  CoxwArgs b = event_args(c);
  b.eta = c->eta.as<double>();
  b.maxp = c->maxp.as<double>();
  b.val = q;
  b.inv_out = inv1;
  b.llpart = c->llpart.as<double>();
  b.st = cst(c);
  BBX_TRY(launch_event_sum<false>(c, b, skip));
  BBX_TRY(launch_scan_out(c, es, 1, q, cum, skip));
  if (!grad) return BBX_OK;
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxw_weight_kernel<false>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->ne, c->wt.as<const double>(), g_out, cum,
             c->napp.as<const int32_t>(), nullptr, nullptr,
             c->tmp.as<double>(), sumw, skip);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, grad);
}

int coxw_create_impl(bbx_design* h, int64_t n_event, const int32_t* start,
                     const int32_t* end, const int32_t* n_app,
                     const double* weights, bbx_coxw** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!start || !end || !n_app) return fail(BBX_ERR_INVALID, "NULL index array");
  if (!weights) return fail(BBX_ERR_INVALID, "NULL weights");
  const int64_t n = h->n;
  if (n >= (int64_t(1) << 31))
    return fail(BBX_ERR_INVALID, "the Cox model needs fewer than 2^31 rows");
  if (n_event < 1 || n_event > n)
    return fail(BBX_ERR_INVALID, "n_event must be in [1, n]");
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
  c->ne = n_event;
  const size_t d8 = sizeof(double), i4 = sizeof(int32_t);
  int st = ham::init_core(c, h, "coxw");
  DevMem* nvec[] = {&c->wt, &c->gz, &c->scan, &c->g_loc};
  for (DevMem* m : nvec)
    if (st == BBX_OK) st = m->alloc(d8 * n);
  DevMem* evec[] = {&c->inv, &c->cs, &c->inv_loc, &c->c_loc};
  for (DevMem* m : evec)
    if (st == BBX_OK) st = m->alloc(d8 * n_event);
  if (st == BBX_OK) st = c->start.alloc(i4 * n_event);
  if (st == BBX_OK) st = c->end.alloc(i4 * n_event);
  if (st == BBX_OK) st = c->napp.alloc(i4 * n);
  if (st == BBX_OK) st = c->csum.alloc(d8 * 2 * SCAN_G);
  if (st == BBX_OK) st = c->maxp.alloc(d8 * NPART);
  if (st != BBX_OK) return ham::discard(c, st);
  const hipMemcpyKind H2D = hipMemcpyHostToDevice;
  hipError_t e = hipMemcpyAsync(c->start.ptr, start, i4 * n_event, H2D,
                                h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->end.ptr, end, i4 * n_event, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->napp.ptr, n_app, i4 * n, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->wt.ptr, weights, d8 * n, H2D, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("coxw upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

// The Cox block of a leapfrog step: everything from eta to X~^T w
struct CoxwLik {
  bbx_coxw* c;
  int operator()(double* grad) const {
    return likelihood_from_eta(c, c->gz.as<double>(), c->inv.as<double>(),
                               nullptr, c->cs.as<double>(), grad);
  }
};

struct CoxwFamily {
  static constexpr const char* name = "coxw";
  using Lik = CoxwLik;
  static int locate(bbx_coxw* c, const double* d_in) {
    BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, c->h->stream, cst(c));
    BBX_TRY(eta_of(c, d_in));
    // a/H is only the scan's input: it goes to the scratch c->inv
    BBX_TRY(likelihood_from_eta(c, c->g_loc.as<double>(), c->inv.as<double>(),
                                c->inv_loc.as<double>(), c->c_loc.as<double>(),
                                nullptr));
    BBX_TRY(read_state(c));
    if (c->host_st->zero)
      return fail(BBX_ERR_NUMERIC,
                  "Hessian location: a risk-set sum of relative hazards is 0");
    return BBX_OK;
  }
  static int hessian_from_v(bbx_coxw* c, const double* d_v, double* d_out);
};

int CoxwFamily::hessian_from_v(bbx_coxw* c, const double* d_v,
                               double* d_out) {
  bbx_design* h = c->h;
  BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
  BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
  const Segs rs = risk_segs(c), es = event_segs(c);
  BBX_TRY(launch_risk_sum<true>(c, rs, nullptr, c->g_loc.as<const double>(),
                                c->eta.as<const double>(), c->tmp.as<double>(),
                                nullptr));
  BBX_TRY(launch_scan_out(c, rs, 2, c->tmp.as<double>(), c->scan.as<double>(),
                          nullptr));
  CoxwArgs b = event_args(c);
  b.inv = c->inv_loc.as<double>();
  b.val = c->inv.as<double>();
  BBX_TRY(launch_event_sum<true>(c, b, nullptr));
  BBX_TRY(launch_scan_out(c, es, 1, c->inv.as<double>(), c->cs.as<double>(),
                          nullptr));
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxw_weight_kernel<true>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->ne, c->wt.as<const double>(),
             c->g_loc.as<const double>(), c->c_loc.as<const double>(),
             c->napp.as<const int32_t>(), c->eta.as<const double>(),
             c->cs.as<const double>(), c->tmp.as<double>(), sumw, nullptr);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, d_out);
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

BBX_HAM_ENTRY_POINTS(coxw, CoxwFamily)
