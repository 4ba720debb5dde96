// Cox proportional-hazards likelihood (model/cox_model.py:180-273) and the
// preconditioned HMC trajectory that uses it (hmc.py:137-174, dynamics.py).
//
// Observations are ordered as the reference orders them (cox_model.py:70-121):
// events first by increasing time, then censored observations by decreasing
// censoring time.  Risk set k (k < ne) is [start_k, end_k]; n_app[i] counts the
// risk sets that contain i.  With eta = X~ beta:
//
//   m      = max eta,  h_i = exp(eta_i - m)              max_kernel, scan pass A
//   scan_i = sum_{j=i}^{ne-1} h_j  (i < ne: suffix over the events)
//          = sum_{j=ne}^{i}   h_j  (i >= ne: prefix over the censored)
//   H_k    = scan[start_k] + (end_k >= ne ? scan[end_k] : 0)
// A late risk set is never a difference of two large prefix sums (the
// reference's structure, cox_model.py:219-233): no cancellation.
//   loglik = sum_k (eta_k - m) - log H_k      (-inf if some H_k == 0)
//   c      = cumsum_k 1/H_k,  w_i = [i < ne] - c[n_app_i - 1] h_i,  grad = X~^T w
// Hessian-vector product at a fixed location (cox_model.py:251-273): u = X~ v,
//   S = segsum(h u), z_k = (1/H_k) ((1/H_k) S_k), cz = cumsum z,
//   r = (c[n_app - 1] h) u - h cz[n_app - 1],  out = X~^T (-r).
//
// Scans.  Every scan is a blocked two-pass scan over a FIXED partition: each
// segment is cut into SCAN_G chunks; pass A writes one sum per chunk (block
// reduction in a fixed order), pass B re-adds the sums of the chunks before its
// own (fixed order) and scans its chunk in tiles of SCAN_BLOCK x SCAN_E.  No
// float atomics anywhere: the same inputs give the same bits on every run.
//
// Trajectory.  The leapfrog kernels, the No-U-Turn tree and their drivers are
// shared with the logit family (hamiltonian.hpp); likelihood_from_eta below
// is the block they call between "eta is complete" and "grad_loglik is
// complete".
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"
#include "cox_scan.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// SCAN_G, SCAN_BLOCK, SCAN_E, Segs, cox_max_kernel and pass B
// (cox_scan_out_kernel): cox_scan.hpp

enum ScanMode {
  SM_H = 0,     // h_i = exp(eta_i - m)                    (risk segments)
  SM_HU = 1,    // h_i u_i                                 (risk segments)
  SM_INVH = 2,  // 1 / H_k, and the loglik partials         (events, forward)
  SM_WU = 3     // (1/H_k) ((1/H_k) S_k)                   (events, forward)
};

struct ScanArgs {
  const double* eta = nullptr;    // SM_H, SM_INVH
  const double* maxp = nullptr;   // NPART partials of max eta
  const double* h = nullptr;      // SM_HU
  const double* u = nullptr;      // SM_HU
  const double* scan = nullptr;   // SM_INVH, SM_WU: risk-segment scan
  const double* inv = nullptr;    // SM_WU: 1 / H at the location
  const int32_t* start = nullptr;
  const int32_t* end = nullptr;
  int64_t ne = 0;
  double* val = nullptr;          // the per-element value, stored
  double* llpart = nullptr;       // SM_INVH: SCAN_G loglik partials
  CoxTraj* st = nullptr;          // SM_INVH: zero / skip flags
};

// Pass A: the value of every element of every chunk (stored in a.val) and one
// sum per chunk.
template <int MODE>
__global__ __launch_bounds__(SCAN_BLOCK) void cox_scan_sum_kernel(
    Segs sg, ScanArgs a, double* __restrict__ csum,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int s = blockIdx.x / SCAN_G, b = blockIdx.x % SCAN_G;
  const int64_t len = sg.len[s];
  const int64_t L = (len + SCAN_G - 1) / SCAN_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < len ? t0 + L : len;
  double m = 0.;
  if (MODE == SM_H || MODE == SM_INVH) m = part_max(a.maxp);
  double acc = 0., ll = 0.;
  bool zero = false;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += SCAN_BLOCK) {
    const int64_t i = seg_elem(sg, s, t);
    double v;
    if (MODE == SM_H) {
      v = exp(a.eta[i] - m);
    } else if (MODE == SM_HU) {
      v = a.h[i] * a.u[i];
    } else {
      const int32_t e = a.end[i];
      double H = a.scan[a.start[i]];
      if (e >= a.ne) H += a.scan[e];
      if (MODE == SM_INVH) {
        zero |= (H == 0.);
        v = 1. / H;
        ll += (a.eta[i] - m) - log(H);
      } else {
        const double iv = a.inv[i];
        v = iv * (iv * H);
      }
    }
    a.val[i] = v;
    acc += v;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (MODE == SM_INVH) {
    ll = block_sum<SCAN_BLOCK>(ll);
    if (zero) {
      a.st->zero = 1;
      a.st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    csum[blockIdx.x] = acc;
    if (MODE == SM_INVH) a.llpart[b] = ll;
  }
}


// w = [i < ne] - c[n_app_i - 1] h_i                 (HESS = false: gradient)
// w = -((c[n_app_i - 1] h_i) u_i - h_i cz[n_app_i - 1])   (HESS = true)
// and the NPART partials of sum(w) (the Tdot's intercept / centring term).
template <bool HESS>
__global__ __launch_bounds__(VEC_BLOCK) void cox_weight_kernel(
    int64_t n, int64_t ne, const double* __restrict__ h,
    const double* __restrict__ c, const int32_t* __restrict__ napp,
    const double* __restrict__ u, const double* __restrict__ cz,
    double* __restrict__ w, double* __restrict__ part,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK) {
    const int32_t k = napp[i] - 1;
    const double rs = c[k] * h[i];
    double v;
    if (HESS) {
      v = -(rs * u[i] - h[i] * cz[k]);
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

#include "cox_strat.hpp"   // the kernels of a stratified handle

using namespace bbx;

// One Cox likelihood on a design (borrowed: the design must outlive it).
struct bbx_cox : HamCore {
  int64_t ne = 0;
  DevMem start, end, napp;               // int32: ne, ne, n
  DevMem hz, scan;                       // n: h, risk scan (tmp: w / h u)
  DevMem inv, cs;                        // ne: 1/H (or z), cumsum
  DevMem h_loc, inv_loc, c_loc;          // the Hessian's location: n, ne, ne
  DevMem csum, maxp;                     // 2 SCAN_G, NPART
  // bbx_cox_create_stratified (cox_strat.hpp): ne counts the events of all
  // strata, `end` holds -1 where a risk set ends at an event, `napp` holds
  // last_set
  bool strat = false;
  int64_t ns = 0;
  DevMem rflag, eflag;                   // uint8: n RowFlag, ne EF_HEAD
  DevMem sid, evrow;                     // int32: n stratum, ne row of an event
  DevMem ms, aggf;                       // ns max eta; int 2 SCAN_G
};

namespace {

Segs risk_segs(const bbx_cox* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 1;
  sg.base[1] = c->ne;
  sg.len[1] = c->n - c->ne;
  sg.rev[1] = 0;
  return sg;
}

Segs event_segs(const bbx_cox* c) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = c->ne;
  sg.rev[0] = 0;
  sg.base[1] = 0;
  sg.len[1] = 0;
  sg.rev[1] = 0;
  return sg;
}

using ham::cst;
using ham::eta_of;
using ham::read_state;

template <int MODE>
int launch_scan_sum(bbx_cox* c, const Segs& sg, int nseg, const ScanArgs& a,
                    const int* skip) {
  BBX_LAUNCH(cox_scan_sum_kernel<MODE>, dim3(nseg * SCAN_G), dim3(SCAN_BLOCK),
             0, c->h->stream, sg, a, c->csum.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

int launch_scan_out(bbx_cox* c, const Segs& sg, int nseg, const double* val,
                    double* out, const int* skip) {
  BBX_LAUNCH(cox_scan_out_kernel, dim3(nseg * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, val, out, c->csum.as<const double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <int MODE>
int launch_strat_agg(bbx_cox* c, int ndir, StratArgs& a, const int* skip) {
  a.aggv = c->csum.as<double>();
  a.aggf = c->aggf.as<int>();
  BBX_LAUNCH(coxs_agg_kernel<MODE>, dim3(ndir * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, a, skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <int OUT>
int launch_strat_out(bbx_cox* c, int ndir, const StratArgs& a,
                     const double* val, double* out, const int* skip) {
  BBX_LAUNCH(coxs_out_kernel<OUT>, dim3(ndir * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, a.len, a.flag, c->sid.as<const int32_t>(), val, out,
             c->csum.as<const double>(), c->aggf.as<const int>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

StratArgs row_args(const bbx_cox* c) {
  StratArgs a;
  a.len = c->n;
  a.flag = c->rflag.as<const uint8_t>();
  a.sid = c->sid.as<const int32_t>();
  return a;
}

StratArgs event_args(const bbx_cox* c) {
  StratArgs a;
  a.len = c->ne;
  a.flag = c->eflag.as<const uint8_t>();
  a.sid = c->sid.as<const int32_t>();
  a.evrow = c->evrow.as<const int32_t>();
  a.start = c->start.as<const int32_t>();
  a.endc = c->end.as<const int32_t>();
  a.scan = c->scan.as<const double>();
  return a;
}

// likelihood_from_eta of a stratified handle: eight launches whatever the
// strata are (max A / B, h A / B, 1/H A / B, w, X~^T w)
int strat_likelihood_from_eta(bbx_cox* c, double* h_out, double* inv,
                              double* cum, double* grad) {
  bbx_design* h = c->h;
  const int* skip = &cst(c)->skip;
  StratArgs m = row_args(c);
  m.eta = c->eta.as<const double>();
  BBX_TRY(launch_strat_agg<SS_MAX>(c, 1, m, skip));
  BBX_TRY(launch_strat_out<SO_MAX>(c, 1, m, m.eta, c->ms.as<double>(), skip));
  StratArgs a = row_args(c);
  a.eta = c->eta.as<const double>();
  a.ms = c->ms.as<const double>();
  a.val = h_out;
  BBX_TRY(launch_strat_agg<SS_H>(c, 2, a, skip));
  BBX_TRY(launch_strat_out<SO_RISK>(c, 2, a, h_out, c->scan.as<double>(), skip));
  StratArgs b = event_args(c);
  b.eta = c->eta.as<const double>();
  b.ms = c->ms.as<const double>();
  b.val = inv;
  b.llpart = c->llpart.as<double>();
  b.st = cst(c);
  BBX_TRY(launch_strat_agg<SS_INVH>(c, 1, b, skip));
  BBX_TRY(launch_strat_out<SO_ALL>(c, 1, b, inv, cum, skip));
  if (!grad) return BBX_OK;
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxs_weight_kernel<false>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->rflag.as<const uint8_t>(), h_out, cum,
             c->napp.as<const int32_t>(), nullptr, nullptr,
             c->tmp.as<double>(), sumw, skip);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, grad);
}

// cox_hessian_dev of a stratified handle, after u = X~ v is in c->eta
int strat_hessian_from_u(bbx_cox* c, double* d_out) {
  bbx_design* h = c->h;
  StratArgs a = row_args(c);
  a.h = c->h_loc.as<const double>();
  a.u = c->eta.as<const double>();
  a.val = c->tmp.as<double>();
  BBX_TRY(launch_strat_agg<SS_HU>(c, 2, a, nullptr));
  BBX_TRY(launch_strat_out<SO_RISK>(c, 2, a, c->tmp.as<double>(),
                                    c->scan.as<double>(), nullptr));
  StratArgs b = event_args(c);
  b.inv = c->inv_loc.as<const double>();
  b.val = c->inv.as<double>();
  BBX_TRY(launch_strat_agg<SS_WU>(c, 1, b, nullptr));
  BBX_TRY(launch_strat_out<SO_ALL>(c, 1, b, c->inv.as<double>(),
                                   c->cs.as<double>(), nullptr));
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(coxs_weight_kernel<true>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->rflag.as<const uint8_t>(),
             c->h_loc.as<const double>(), c->c_loc.as<const double>(),
             c->napp.as<const int32_t>(), c->eta.as<const double>(),
             c->cs.as<const double>(), c->tmp.as<double>(), sumw, nullptr);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, d_out);
}

// From eta (already in c->eta, complete in stream order): h, H, the loglik
// partials, 1/H into `inv` and c = cumsum(1/H) into `cum`, then (grad != null)
// w and grad = X~^T w.  `h_out`: where h goes (c->hz or the location's).
int likelihood_from_eta(bbx_cox* c, double* h_out, double* inv, double* cum,
                        double* grad) {
  if (c->strat) return strat_likelihood_from_eta(c, h_out, inv, cum, grad);
  bbx_design* h = c->h;
  const int* skip = &cst(c)->skip;
  BBX_LAUNCH(cox_max_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream, c->n,
             c->eta.as<const double>(), c->maxp.as<double>(), skip);
  BBX_HIP(hipGetLastError());
  const Segs rs = risk_segs(c), es = event_segs(c);
  ScanArgs a;
  a.eta = c->eta.as<double>();
  a.maxp = c->maxp.as<double>();
  a.val = h_out;
  BBX_TRY(launch_scan_sum<SM_H>(c, rs, 2, a, skip));
  BBX_TRY(launch_scan_out(c, rs, 2, h_out, c->scan.as<double>(), skip));
  ScanArgs b;
  b.eta = c->eta.as<double>();
  b.maxp = c->maxp.as<double>();
  b.scan = c->scan.as<double>();
  b.start = c->start.as<int32_t>();
  b.end = c->end.as<int32_t>();
  b.ne = c->ne;
  b.val = inv;
  b.llpart = c->llpart.as<double>();
  b.st = cst(c);
  BBX_TRY(launch_scan_sum<SM_INVH>(c, es, 1, b, skip));
  BBX_TRY(launch_scan_out(c, es, 1, inv, cum, skip));
  if (!grad) return BBX_OK;
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(cox_weight_kernel<false>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->ne, h_out, cum, c->napp.as<const int32_t>(),
             nullptr, nullptr, c->tmp.as<double>(), sumw, skip);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, grad);
}

// A handle with every buffer both kinds of handle use, the three index arrays
// uploaded (n_event, n_event and n int32) and the device state zeroed; the
// uploads are complete on return.
int cox_new(bbx_design* h, int64_t n_event, const int32_t* start,
            const int32_t* end, const int32_t* n_app, bbx_cox** out) {
  const int64_t n = h->n;
  bbx_cox* c = new bbx_cox;
  c->ne = n_event;
  const size_t d8 = sizeof(double), i4 = sizeof(int32_t);
  int st = ham::init_core(c, h, "cox");
  DevMem* nvec[] = {&c->hz, &c->scan, &c->h_loc};
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
  hipError_t e = hipMemcpyAsync(c->start.ptr, start, i4 * n_event,
                                hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->end.ptr, end, i4 * n_event, hipMemcpyHostToDevice,
                       h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->napp.ptr, n_app, i4 * n, hipMemcpyHostToDevice,
                       h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("cox upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

int cox_create_impl(bbx_design* h, int64_t n_event, const int32_t* start,
                    const int32_t* end, const int32_t* n_app, bbx_cox** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!start || !end || !n_app) return fail(BBX_ERR_INVALID, "NULL index array");
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
  return cox_new(h, n_event, start, end, n_app, out);
}

int cox_create_strat_impl(bbx_design* h, int64_t ns, const int64_t* sptr,
                          const int32_t* sne, const int32_t* start,
                          const int32_t* end, const int32_t* last_set,
                          bbx_cox** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!sptr || !sne || !start || !end || !last_set)
    return fail(BBX_ERR_INVALID, "NULL index array");
  const int64_t n = h->n;
  if (n >= (int64_t(1) << 31))
    return fail(BBX_ERR_INVALID, "the Cox model needs fewer than 2^31 rows");
  if (ns < 1 || ns > n)
    return fail(BBX_ERR_INVALID, "n_strata must be in [1, n]");
  if (sptr[0] != 0)
    return fail(BBX_ERR_INVALID, "stratum_ptr[0] must be 0");
  int64_t ne = 0;
  for (int64_t s = 0; s < ns; ++s) {
    // in this order: a bad stratum_ptr must not be used as a bound below
    if (sptr[s + 1] <= sptr[s] || sptr[s + 1] > n)
      return fail(BBX_ERR_INVALID, "stratum " + std::to_string(s) +
                                       ": stratum_ptr is not increasing "
                                       "within [0, n]");
    if (sne[s] < 1 || sne[s] > sptr[s + 1] - sptr[s])
      return fail(BBX_ERR_INVALID, "stratum " + std::to_string(s) +
                                       ": stratum_n_event outside [1, rows "
                                       "of the stratum]");
    ne += sne[s];
  }
  if (sptr[ns] != n)
    return fail(BBX_ERR_INVALID, "stratum_ptr[n_strata] must be n");
  // the kernels index scan[start], scan[end], c[last_set], ms[sid] and
  // eta[evrow]: check what is given, build the rest here
  std::vector<uint8_t> rflag(n, 0), eflag(ne, 0);
  std::vector<int32_t> sid(n), evrow(ne), endc(ne);
  int64_t e0 = 0;
  for (int64_t s = 0; s < ns; ++s) {
    const int64_t r0 = sptr[s], r1 = sptr[s + 1], c0 = r0 + sne[s];
    for (int64_t j = 0; j < sne[s]; ++j) {
      const int64_t k = e0 + j, r = r0 + j;
      if (start[k] < r0 || start[k] > r || end[k] < c0 - 1 || end[k] >= r1)
        return fail(BBX_ERR_INVALID, "risk set " + std::to_string(k) +
                                         " (stratum " + std::to_string(s) +
                                         ") leaves its stratum");
      evrow[k] = (int32_t)r;
      endc[k] = end[k] >= c0 ? end[k] : -1;
      rflag[r] |= RF_EVENT;
    }
    for (int64_t r = r0; r < r1; ++r) {
      if (last_set[r] < e0 || last_set[r] >= e0 + sne[s])
        return fail(BBX_ERR_INVALID, "last_set[" + std::to_string(r) +
                                         "] is no event of stratum " +
                                         std::to_string(s));
      sid[r] = (int32_t)s;
    }
    eflag[e0] = EF_HEAD;
    rflag[r0] |= RF_FWD | RF_SHEAD;
    if (c0 < r1) rflag[c0] |= RF_FWD;
    rflag[c0 - 1] |= RF_BWD;
    rflag[r1 - 1] |= RF_BWD | RF_SLAST;
    e0 += sne[s];
  }
  bbx_cox* c = nullptr;
  BBX_TRY(cox_new(h, ne, start, endc.data(), last_set, &c));
  c->strat = true;
  c->ns = ns;
  const size_t d8 = sizeof(double), i4 = sizeof(int32_t);
  int st = c->rflag.alloc(n);
  if (st == BBX_OK) st = c->eflag.alloc(ne);
  if (st == BBX_OK) st = c->sid.alloc(i4 * n);
  if (st == BBX_OK) st = c->evrow.alloc(i4 * ne);
  if (st == BBX_OK) st = c->ms.alloc(d8 * ns);
  if (st == BBX_OK) st = c->aggf.alloc(sizeof(int) * 2 * SCAN_G);
  if (st == BBX_OK) {
    hipError_t e = hipMemcpyAsync(c->rflag.ptr, rflag.data(), n,
                                  hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->eflag.ptr, eflag.data(), ne, hipMemcpyHostToDevice,
                         h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->sid.ptr, sid.data(), i4 * n, hipMemcpyHostToDevice,
                         h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->evrow.ptr, evrow.data(), i4 * ne,
                         hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
      st = fail(BBX_ERR_HIP, std::string("stratified cox upload: ") +
                                 hipGetErrorString(e));
  }
  if (st != BBX_OK) return ham::discard(c, st);
  *out = c;
  return BBX_OK;
}

// The Cox block of a leapfrog step: everything from eta to X~^T w
struct CoxLik {
  bbx_cox* c;
  int operator()(double* grad) const {
    return likelihood_from_eta(c, c->hz.as<double>(), c->inv.as<double>(),
                               c->cs.as<double>(), grad);
  }
};

struct CoxFamily {
  static constexpr const char* name = "cox";
  using Lik = CoxLik;
  static int locate(bbx_cox* c, const double* d_in) {
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
  static int hessian_from_v(bbx_cox* c, const double* d_v, double* d_out);
};

int CoxFamily::hessian_from_v(bbx_cox* c, const double* d_v,
                              double* d_out) {
  bbx_design* h = c->h;
  BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
  BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
  if (c->strat) return strat_hessian_from_u(c, d_out);
  const Segs rs = risk_segs(c), es = event_segs(c);
  ScanArgs a;
  a.h = c->h_loc.as<double>();
  a.u = c->eta.as<double>();
  a.val = c->tmp.as<double>();
  BBX_TRY(launch_scan_sum<SM_HU>(c, rs, 2, a, nullptr));
  BBX_TRY(launch_scan_out(c, rs, 2, c->tmp.as<double>(), c->scan.as<double>(),
                          nullptr));
  ScanArgs b;
  b.scan = c->scan.as<double>();
  b.inv = c->inv_loc.as<double>();
  b.start = c->start.as<int32_t>();
  b.end = c->end.as<int32_t>();
  b.ne = c->ne;
  b.val = c->inv.as<double>();
  BBX_TRY(launch_scan_sum<SM_WU>(c, es, 1, b, nullptr));
  BBX_TRY(launch_scan_out(c, es, 1, c->inv.as<double>(), c->cs.as<double>(),
                          nullptr));
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH(cox_weight_kernel<true>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->n, c->ne, c->h_loc.as<const double>(),
             c->c_loc.as<const double>(), c->napp.as<const int32_t>(),
             c->eta.as<const double>(), c->cs.as<const double>(),
             c->tmp.as<double>(), sumw, nullptr);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), sumw, ep, d_out);
}

}  // namespace

extern "C" {

int bbx_cox_create(bbx_design* design, int64_t n_event, const int32_t* start,
                   const int32_t* end, const int32_t* n_app, bbx_cox** out) {
  return no_throw([&] {
    return cox_create_impl(design, n_event, start, end, n_app, out);
  });
}

int bbx_cox_create_stratified(bbx_design* design, int64_t n_strata,
                              const int64_t* stratum_ptr,
                              const int32_t* stratum_n_event,
                              const int32_t* start, const int32_t* end,
                              const int32_t* last_set, bbx_cox** out) {
  return no_throw([&] {
    return cox_create_strat_impl(design, n_strata, stratum_ptr,
                                 stratum_n_event, start, end, last_set, out);
  });
}

}  // extern "C"

BBX_HAM_ENTRY_POINTS(cox, CoxFamily)
