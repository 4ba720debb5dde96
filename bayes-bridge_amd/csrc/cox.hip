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
// shared with the logit family (hamiltonian.hpp); likelihood_from_eta is the
// block they call between "eta is complete" and "grad_loglik is complete".
//
// The kernels and that block are cox_family.hpp's, under the policy CoxPlain
// below; a stratified handle runs cox_strat.hpp's kernels instead.
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_family.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

#include "cox_strat.hpp"   // the kernels of a stratified handle

using namespace bbx;

// One Cox likelihood on a design (borrowed: the design must outlive it).
struct bbx_cox : CoxCore {
  DevMem start, end, napp;               // int32: ne, ne, n
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

// The header's formulae as cox_family.hpp's kernels ask for them
struct CoxPlain {
  using Handle = bbx_cox;
  static constexpr const char* name = "cox";
  static constexpr int halves = 1;
  static constexpr bool keeps_inv = false;
  const int32_t* start;
  const int32_t* end;
  const int32_t* napp;
  int64_t ne;
  static CoxPlain make(const bbx_cox* c) {
    return {c->start.as<const int32_t>(), c->end.as<const int32_t>(),
            c->napp.as<const int32_t>(), c->ne};
  }
  // the events reversed (suffix sums), the censored rows forward
  static void risk_layout(const bbx_cox* c, int* nseg, int64_t* len, int* rev) {
    *nseg = 2;
    len[0] = c->ne, rev[0] = 1;
    len[1] = c->n - c->ne, rev[1] = 0;
  }
  static double* hu(bbx_cox* c) { return c->tmp.as<double>(); }
  __device__ int64_t row(int, int64_t i) const { return i; }
  __device__ double h_of(int64_t, double e) const { return e; }
  __device__ double risk_term(int, int64_t, double x) const { return x; }
  __device__ double H(const double* scan, int64_t k, double&) const {
    const int32_t e = end[k];
    double H = scan[start[k]];
    if (e >= ne) H += scan[e];
    return H;
  }
  __device__ bool empty(double H) const { return H == 0.; }
  __device__ int64_t event_row(int64_t k) const { return k; }
  __device__ double scaled(double x, double) const { return x; }
  template <bool HESS>
  __device__ void AZ(const double* c, const double* cz, int64_t i, double& A,
                     double& Z) const {
    const int32_t k = napp[i] - 1;
    A = c[k];
    if (HESS) Z = cz[k];
  }
  __device__ double indicator(int64_t i) const { return i < ne ? 1. : 0.; }
};

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

// The two blocks of cox_family.hpp, or a stratified handle's own
struct CoxDriver {
  static int likelihood(bbx_cox* c, double* h_out, double* inv, double* inv1,
                        double* cum, double* grad) {
    if (c->strat) return strat_likelihood_from_eta(c, h_out, inv, cum, grad);
    return likelihood_from_eta<CoxPlain>(c, h_out, inv, inv1, cum, grad);
  }
  static int hessian(bbx_cox* c, double* d_out) {
    if (c->strat) return strat_hessian_from_u(c, d_out);
    return hessian_from_u<CoxPlain>(c, d_out);
  }
  // the shift of an event: max eta, or the max of the event's stratum
  static CoxShift shift(const bbx_cox* c) {
    CoxShift sh = CoxDriverT<CoxPlain>::shift(c);
    if (c->strat) {
      sh.ms = c->ms.as<const double>();
      sh.sid = c->sid.as<const int32_t>();
      sh.evrow = c->evrow.as<const int32_t>();
    }
    return sh;
  }
};

using CoxFamily = CoxFamilyT<CoxPlain, CoxDriver>;

// A handle with every buffer both kinds of handle use, the three index arrays
// uploaded (n_event, n_event and n int32) and the device state zeroed; the
// uploads are complete on return.
int cox_new(bbx_design* h, int64_t n_event, const int32_t* start,
            const int32_t* end, const int32_t* n_app, bbx_cox** out) {
  bbx_cox* c = new bbx_cox;
  int st = cox_alloc(c, h, "cox", n_event, h->n, n_event);
  if (st == BBX_OK) st = cox_upload(c, "cox", c->start, start, n_event);
  if (st == BBX_OK) st = cox_upload(c, "cox", c->end, end, n_event);
  if (st == BBX_OK) st = cox_upload(c, "cox", c->napp, n_app, h->n);
  if (st == BBX_OK) st = cox_uploaded(c, "cox");
  if (st != BBX_OK) return ham::discard(c, st);
  *out = c;
  return BBX_OK;
}

int cox_create_impl(bbx_design* h, int64_t n_event, const int32_t* start,
                    const int32_t* end, const int32_t* n_app, bbx_cox** out) {
  BBX_TRY(cox_create_head(
      h, n_event, start && end && n_app ? nullptr : "NULL index array", out));
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
BBX_COX_PREDICT_ENTRY_POINTS(cox, CoxFamily)
