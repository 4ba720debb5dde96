// What the Cox likelihood handles share (cox.hip, cox_interval.hip,
// cox_efron.hip, cox_weighted.hip, cox_finegray.hip): the handle base, the
// three kernels that form values, the six-launch driver, the family that
// hamiltonian.hpp's entry points take and the prediction calls (the baseline
// hazard read off the likelihood's cumulative sum, the residuals; at the end
// of the file).  A handle states a policy V, a small
// struct of device pointers that is passed to the kernels by value:
//
//   device side (the per-element expressions; everything else is written once)
//     row(s, i)         the row behind element i of risk segment s
//     h_of(r, e)        the relative hazard of row r from e = exp(eta_r - m)
//     risk_term(s, i, x)   what element i of risk segment s adds to its scan:
//                       x (h, or h u), or x times a factor of the element
//     H(scan, k, f)     the risk-set sum of event k from the risk scan; f: a
//                       factor of event k the policy wants back (weight, l/d)
//     empty(H)          the test that raises CoxTraj::zero and skip
//     event_row(k)      the row of event k
//     scaled(x, f)      x, or x times the event's weight
//     AZ<HESS>(c, cz, i, A, Z)   A_i of row i from the cumulative sum c and,
//                       HESS, Z_i from cz the same way (one walk of the row's
//                       indices serves both)
//     indicator(i)      the event indicator (or event weight) of row i
//     halves            1, or 2: f times the value goes to element ne + k and
//                       its chunk sums to csum[SCAN_G + b]
//     half_rev          halves == 2: 0, the second half's cumulative sum runs
//                       forward as the first one's, or 2, it is a suffix sum
//                       (cox_scan.hpp: over the same chunks)
//     keeps_inv         1/H is stored beside the (scaled) value
//   host side
//     Handle, name      the C ABI's struct and "cox", "coxcp", ...
//     make(c)           the policy of handle c
//     risk_layout(c, nseg, len, rev)   the risk segments: how many are
//                       launched, their lengths and directions (segment 1
//                       starts where segment 0 ends)
//     hu(c)             where the Hessian's h u goes
//
// A policy method is the expression of its handle's file header, with that
// association and rounding order; the kernels below only add, reduce and
// store.  Policies live in the unnamed namespace of their file: no two
// translation units instantiate a kernel with the same arguments, and no
// handle type's name reaches an exported symbol.
#pragma once
#include <math.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "cox_scan.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// The buffers of every Cox handle.  "n" below is the handle's row length (n,
// or nseg n of the interval handle), "ne" its event length (ne, or 2 ne of
// the Efron handle).
struct CoxCore : HamCore {
  int64_t ne = 0;
  DevMem hz, scan;                       // n: h, risk scan
  DevMem inv, cs;                        // ne: 1/H (or z), cumsum
  DevMem h_loc, inv_loc, c_loc;          // the Hessian's location: n, ne, ne
  DevMem csum, maxp;                     // 2 SCAN_G, NPART
};

// Pass A over the risk segments: h (HU = false) or h u, stored in val, and
// one sum per chunk.
template <class V, bool HU>
__global__ __launch_bounds__(SCAN_BLOCK) void cox_risk_sum_kernel(
    Segs sg, V v, const double* __restrict__ eta,
    const double* __restrict__ maxp, const double* __restrict__ h,
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
    const int64_t r = v.row(s, i);
    const double x =
        v.risk_term(s, i, HU ? h[r] * u[r] : v.h_of(r, exp(eta[r] - m)));
    val[i] = x;
    acc += x;
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (threadIdx.x == 0) csum[blockIdx.x] = acc;
}

struct CoxEventArgs {
  const double* eta = nullptr;    // likelihood mode
  const double* maxp = nullptr;   // likelihood mode: NPART partials of max eta
  const double* scan = nullptr;   // the risk scan
  const double* inv = nullptr;    // Hessian mode: 1 / H at the location
  int64_t ne = 0;
  double* val = nullptr;          // the value (halves == 2: and f times it)
  double* inv_out = nullptr;      // keeps_inv, optional: 1 / H
  double* llpart = nullptr;       // likelihood mode: SCAN_G loglik partials
  CoxTraj* st = nullptr;          // likelihood mode: zero / skip flags
};

// Pass A over the events, SCAN_G blocks: H_k (HESS: S_k) from the risk scan,
// 1/H_k (HESS: inv_k (inv_k S_k)), scaled, stored in val, and one sum per
// chunk and half.
template <class V, bool HESS>
__global__ __launch_bounds__(SCAN_BLOCK) void cox_event_sum_kernel(
    V v, CoxEventArgs a, double* __restrict__ csum,
    const int* __restrict__ skip) {
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
    double f;
    const double H = v.H(a.scan, k, f);
    double x;
    if (!HESS) {
      zero |= v.empty(H);
      const double iv = 1. / H;
      if (V::keeps_inv && a.inv_out) a.inv_out[k] = iv;
      x = v.scaled(iv, f);
      ll += v.scaled((a.eta[v.event_row(k)] - m) - log(H), f);
    } else {
      const double iv = a.inv[k];
      x = v.scaled(iv * (iv * H), f);
    }
    a.val[k] = x;
    acc += x;
    if (V::halves == 2) {
      const double xb = f * x;
      a.val[a.ne + k] = xb;
      accb += xb;
    }
  }
  acc = block_sum<SCAN_BLOCK>(acc);
  if (V::halves == 2) accb = block_sum<SCAN_BLOCK>(accb);
  if (!HESS) {
    ll = block_sum<SCAN_BLOCK>(ll);
    if (zero) {
      a.st->zero = 1;
      a.st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    csum[b] = acc;
    if (V::halves == 2) csum[SCAN_G + b] = accb;
    if (!HESS) a.llpart[b] = ll;
  }
}

// w = indicator_i - h_i A_i                           (HESS = false: gradient)
// w = -((h_i A_i) u_i - h_i Z_i), Z as A from cz      (HESS = true)
// and the NPART partials of sum(w) (the Tdot's intercept / centring term).
template <class V, bool HESS>
__global__ __launch_bounds__(VEC_BLOCK) void cox_row_weight_kernel(
    V v, int64_t n, const double* __restrict__ h, const double* __restrict__ c,
    const double* __restrict__ u, const double* __restrict__ cz,
    double* __restrict__ w, double* __restrict__ part,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK) {
    const double hi = h[i];
    double A, Z = 0.;
    v.template AZ<HESS>(c, cz, i, A, Z);
    const double rs = hi * A;
    double x;
    if (HESS) {
      x = -(rs * u[i] - hi * Z);
    } else {
      x = v.indicator(i) - rs;
    }
    w[i] = x;
    acc += x;
  }
  acc = block_sum<VEC_BLOCK>(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// Where the shift m of an event comes from: the NPART partials of max eta, or
// (a stratified handle) the stratum's own max through the row of the event
struct CoxShift {
  const double* maxp = nullptr;
  const double* ms = nullptr;      // per stratum; null: one shift, from maxp
  const int32_t* sid = nullptr;    // stratum of a row
  const int32_t* evrow = nullptr;  // row of an event
};

// log Lambda0 on a grid: out[j] = log(c[k_j]) - m, k_j = grid_event[j]; -inf
// where k_j is -1 (no event at or before the grid point).  c is the first
// event half of the likelihood's cumulative sum, complete in stream order.  A
// draw whose likelihood raised skip (an empty risk-set sum) writes nothing
// but its flag.  Static, as the scan kernels are: one copy per handle file.
static __global__ __launch_bounds__(VEC_BLOCK) void cox_hazard_grid_kernel(
    CoxShift sh, int64_t n_grid, const int32_t* __restrict__ grid_event,
    const double* __restrict__ c, double* __restrict__ out,
    int* __restrict__ bad, const CoxTraj* __restrict__ st) {
  if (st->skip) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 1;
    return;
  }
  double m = 0.;
  if (!sh.ms) m = part_max(sh.maxp);
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < n_grid;
       j += (int64_t)gridDim.x * VEC_BLOCK) {
    const int32_t k = grid_event[j];
    double v = -INFINITY;
    if (k >= 0) {
      if (sh.ms) m = sh.ms[sh.sid[sh.evrow[k]]];
      v = log(c[k]) - m;
    }
    out[j] = v;
  }
}

namespace {  // host side: internal, as the handle types appear in the names

using ham::cst;
using ham::eta_of;
using ham::read_state;

// The shared head of a `create`.  `missing`: the message for the first NULL
// array argument, or null where every array is given.
template <class H>
int cox_create_head(bbx_design* h, int64_t n_event, const char* missing,
                    H** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (missing) return fail(BBX_ERR_INVALID, missing);
  if (h->n >= (int64_t(1) << 31))
    return fail(BBX_ERR_INVALID, "the Cox model needs fewer than 2^31 rows");
  if (n_event < 1 || n_event > h->n)
    return fail(BBX_ERR_INVALID, "n_event must be in [1, n]");
  return BBX_OK;
}

// HamCore's part of a fresh handle and the buffers of CoxCore: `rows` doubles
// in each row-length buffer, `events` in each event-length one.
int cox_alloc(CoxCore* c, bbx_design* h, const char* family, int64_t n_event,
              int64_t rows, int64_t events) {
  c->ne = n_event;
  const size_t d8 = sizeof(double);
  BBX_TRY(ham::init_core(c, h, family));
  for (DevMem* m : {&c->hz, &c->scan, &c->h_loc}) BBX_TRY(m->alloc(d8 * rows));
  for (DevMem* m : {&c->inv, &c->cs, &c->inv_loc, &c->c_loc})
    BBX_TRY(m->alloc(d8 * events));
  BBX_TRY(c->csum.alloc(d8 * 2 * SCAN_G));
  return c->maxp.alloc(d8 * NPART);
}

int cox_upload_failed(const char* family, hipError_t e) {
  return fail(BBX_ERR_HIP, std::string(family) + " upload: " +
                               hipGetErrorString(e));
}

// Allocates `m` for `count` values and queues their upload from the host
template <class T>
int cox_upload(CoxCore* c, const char* family, DevMem& m, const T* src,
               size_t count) {
  BBX_TRY(m.alloc(sizeof(T) * count));
  const hipError_t e = hipMemcpyAsync(m.ptr, src, sizeof(T) * count,
                                      hipMemcpyHostToDevice, c->h->stream);
  return e == hipSuccess ? BBX_OK : cox_upload_failed(family, e);
}

// The end of a `create`: the uploads are complete on return
int cox_uploaded(CoxCore* c, const char* family) {
  const hipError_t e = hipStreamSynchronize(c->h->stream);
  return e == hipSuccess ? BBX_OK : cox_upload_failed(family, e);
}

// Two segments, the second after the first
Segs cox_segs(int64_t len0, int rev0, int64_t len1, int rev1) {
  Segs sg;
  sg.base[0] = 0;
  sg.len[0] = len0;
  sg.rev[0] = rev0;
  sg.base[1] = len0;
  sg.len[1] = len1;
  sg.rev[1] = rev1;
  return sg;
}

template <class V>
Segs risk_segs(const typename V::Handle* c, int* nseg) {
  int64_t len[2];
  int rev[2];
  V::risk_layout(c, nseg, len, rev);
  return cox_segs(len[0], rev[0], len[1], rev[1]);
}

// The cumulative sums over the events, one per half: the first forward, the
// second as the policy says
template <class V>
Segs event_segs(const typename V::Handle* c) {
  if constexpr (V::halves == 2) {
    return cox_segs(c->ne, 0, c->ne, V::half_rev);
  } else {
    return cox_segs(c->ne, 0, 0, 0);
  }
}

int launch_scan_out(CoxCore* c, const Segs& sg, int nseg, const double* val,
                    double* out, const int* skip) {
  BBX_LAUNCH(cox_scan_out_kernel, dim3(nseg * SCAN_G), dim3(SCAN_BLOCK), 0,
             c->h->stream, sg, val, out, c->csum.as<const double>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// Risk pass A / B: the values into `val`, their scan into c->scan
template <class V, bool HU>
int launch_risk(typename V::Handle* c, const double* h, double* val,
                const int* skip) {
  int nseg;
  const Segs rs = risk_segs<V>(c, &nseg);
  BBX_LAUNCH((cox_risk_sum_kernel<V, HU>), dim3(nseg * SCAN_G),
             dim3(SCAN_BLOCK), 0, c->h->stream, rs, V::make(c),
             c->eta.template as<const double>(),
             c->maxp.template as<const double>(), h,
             c->eta.template as<const double>(), val,
             c->csum.template as<double>(), skip);
  BBX_HIP(hipGetLastError());
  return launch_scan_out(c, rs, nseg, val, c->scan.template as<double>(),
                         skip);
}

// Event pass A / B: the values into a.val, their cumsums into `cum`
template <class V, bool HESS>
int launch_event(typename V::Handle* c, CoxEventArgs a, double* cum,
                 const int* skip) {
  a.scan = c->scan.template as<const double>();
  a.ne = c->ne;
  BBX_LAUNCH((cox_event_sum_kernel<V, HESS>), dim3(SCAN_G), dim3(SCAN_BLOCK),
             0, c->h->stream, V::make(c), a, c->csum.template as<double>(),
             skip);
  BBX_HIP(hipGetLastError());
  return launch_scan_out(c, event_segs<V>(c), V::halves, a.val, cum, skip);
}

// Row pass and X~^T w into `out`
template <class V, bool HESS>
int launch_rows(typename V::Handle* c, const double* h_at, const double* cum,
                const double* cz, double* out, const int* skip) {
  bbx_design* h = c->h;
  double* w = c->tmp.template as<double>();
  double* sumw = part_slot(h, PS_SUMW);
  BBX_LAUNCH((cox_row_weight_kernel<V, HESS>), dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, V::make(c), c->n, h_at, cum,
             HESS ? c->eta.template as<const double>() : nullptr, cz, w, sumw,
             skip);
  BBX_HIP(hipGetLastError());
  TdotEpilogue ep;
  return launch_tdot(h, w, sumw, ep, out);
}

// From eta (already in c->eta, complete in stream order): h, H, the loglik
// partials, the event values into `inv` (keeps_inv: and 1/H into `inv1` where
// given) and their cumsums into `cum`, then (grad != null) w and
// grad = X~^T w.  `h_out`: where h goes (c->hz or the location's).  Six
// launches: max, risk pass A / B, event pass A / B, rows.
template <class V>
int likelihood_from_eta(typename V::Handle* c, double* h_out, double* inv,
                        double* inv1, double* cum, double* grad) {
  const int* skip = &cst(c)->skip;
  BBX_LAUNCH(cox_max_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, c->h->stream,
             c->n, c->eta.template as<const double>(),
             c->maxp.template as<double>(), skip);
  BBX_HIP(hipGetLastError());
  BBX_TRY((launch_risk<V, false>(c, nullptr, h_out, skip)));
  CoxEventArgs b;
  b.eta = c->eta.template as<const double>();
  b.maxp = c->maxp.template as<const double>();
  b.val = inv;
  b.inv_out = inv1;
  b.llpart = c->llpart.template as<double>();
  b.st = cst(c);
  BBX_TRY((launch_event<V, false>(c, b, cum, skip)));
  if (!grad) return BBX_OK;
  return launch_rows<V, false>(c, h_out, cum, nullptr, grad, skip);
}

// The Hessian matvec at the location, after u = X~ v is in c->eta
template <class V>
int hessian_from_u(typename V::Handle* c, double* d_out) {
  const double* h_loc = c->h_loc.template as<const double>();
  BBX_TRY((launch_risk<V, true>(c, h_loc, V::hu(c), nullptr)));
  CoxEventArgs b;
  b.inv = c->inv_loc.template as<const double>();
  b.val = c->inv.template as<double>();
  BBX_TRY((launch_event<V, true>(c, b, c->cs.template as<double>(), nullptr)));
  return launch_rows<V, true>(c, h_loc, c->c_loc.template as<const double>(),
                              c->cs.template as<const double>(), d_out,
                              nullptr);
}

// The two blocks above as a family calls them; cox.hip states its own, which
// sends a stratified handle to its own algorithm
template <class V>
struct CoxDriverT {
  using H = typename V::Handle;
  static int likelihood(H* c, double* h_out, double* inv, double* inv1,
                        double* cum, double* grad) {
    return likelihood_from_eta<V>(c, h_out, inv, inv1, cum, grad);
  }
  static int hessian(H* c, double* d_out) { return hessian_from_u<V>(c, d_out); }
  static CoxShift shift(const H* c) {
    CoxShift sh;
    sh.maxp = c->maxp.template as<const double>();
    return sh;
  }
};

// The policy hamiltonian.hpp's entry points take
template <class V, class D = CoxDriverT<V>>
struct CoxFamilyT {
  using H = typename V::Handle;
  static constexpr const char* name = V::name;
  // The Cox block of a leapfrog step: everything from eta to X~^T w
  struct Lik {
    H* c;
    int operator()(double* grad) const {
      return D::likelihood(c, c->hz.template as<double>(),
                           c->inv.template as<double>(), nullptr,
                           c->cs.template as<double>(), grad);
    }
  };
  static int locate(H* c, const double* d_in) {
    BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, c->h->stream, cst(c));
    BBX_TRY(eta_of(c, d_in));
    // keeps_inv: the location keeps 1/H itself; the scaled value is only the
    // scan's input and goes to the scratch c->inv
    double* inv_loc = c->inv_loc.template as<double>();
    BBX_TRY(D::likelihood(c, c->h_loc.template as<double>(),
                          V::keeps_inv ? c->inv.template as<double>() : inv_loc,
                          V::keeps_inv ? inv_loc : nullptr,
                          c->c_loc.template as<double>(), nullptr));
    BBX_TRY(read_state(c));
    if (c->host_st->zero)
      return fail(BBX_ERR_NUMERIC,
                  "Hessian location: a risk-set sum of relative hazards is 0");
    return BBX_OK;
  }
  static int hessian_from_v(H* c, const double* d_v, double* d_out) {
    BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, c->h->stream, cst(c));
    BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
    return D::hessian(c, d_out);
  }
  static CoxShift shift(const H* c) { return D::shift(c); }
};

// ------------------------------------------------- prediction
// The two calls below evaluate the likelihood block at coefficients from the
// host; they use the trajectory's scratch (eta, hz, inv, cs, tmp, gl) and
// never the Hessian's location.  A No-U-Turn tree between nuts_begin and
// nuts_sample keeps its state in the same scratch: refused.
template <class F>
int predict_head(const typename F::H* c, const char* entry) {
  BBX_TRY(ham::check(c, F::name));
  if (c->nuts_open)
    return fail(BBX_ERR_STATE, std::string("bbx_") + F::name + "_" + entry +
                                   ": a No-U-Turn tree is installed on the "
                                   "handle (bbx_" + F::name +
                                   "_nuts_sample ends the draw)");
  return BBX_OK;
}

// log Lambda0 of n_draw coefficient vectors on one grid: per draw the flags
// are reset, eta = X~ beta, the likelihood block without its gradient, the
// gather; everything is enqueued before the one synchronisation.
template <class F>
int baseline_hazard_impl(typename F::H* c, const double* beta, int64_t n_draw,
                         int64_t n_grid, const int32_t* grid_event,
                         double* log_hazard) {
  bbx_design* h = c->h;
  hipStream_t s = h->stream;
  const size_t pbytes = sizeof(double) * c->P;
  DevMem d_beta, d_grid, d_out, d_bad;
  BBX_TRY(d_beta.alloc(pbytes * n_draw));
  BBX_TRY(d_grid.alloc(sizeof(int32_t) * n_grid));
  BBX_TRY(d_out.alloc(sizeof(double) * n_draw * n_grid));
  BBX_TRY(d_bad.alloc(sizeof(int) * n_draw));
  std::vector<int> bad(n_draw);
  BBX_HIP(hipMemcpyAsync(d_beta.ptr, beta, pbytes * n_draw,
                         hipMemcpyHostToDevice, s));
  BBX_HIP(hipMemcpyAsync(d_grid.ptr, grid_event, sizeof(int32_t) * n_grid,
                         hipMemcpyHostToDevice, s));
  BBX_HIP(hipMemsetAsync(d_bad.ptr, 0, sizeof(int) * n_draw, s));
  const int blocks =
      (int)((n_grid + VEC_BLOCK - 1) / VEC_BLOCK < NPART
                ? (n_grid + VEC_BLOCK - 1) / VEC_BLOCK
                : NPART);
  typename F::Lik lik{c};
  // the staging vector the one-draw calls use: the same eta, bit for bit
  double* d_in = h->stage_P.template as<double>();
  for (int64_t d = 0; d < n_draw; ++d) {
    BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, s, cst(c));
    BBX_HIP(hipGetLastError());
    BBX_HIP(hipMemcpyAsync(d_in, d_beta.template as<double>() + d * c->P,
                           pbytes, hipMemcpyDeviceToDevice, s));
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(lik(nullptr));
    BBX_LAUNCH(cox_hazard_grid_kernel, dim3(blocks), dim3(VEC_BLOCK), 0, s,
               F::shift(c), n_grid, d_grid.template as<const int32_t>(),
               c->cs.template as<const double>(),
               d_out.template as<double>() + d * n_grid,
               d_bad.template as<int>() + d, cst(c));
    BBX_HIP(hipGetLastError());
  }
  BBX_HIP(hipMemcpyAsync(log_hazard, d_out.ptr,
                         sizeof(double) * n_draw * n_grid,
                         hipMemcpyDeviceToHost, s));
  BBX_HIP(hipMemcpyAsync(bad.data(), d_bad.ptr, sizeof(int) * n_draw,
                         hipMemcpyDeviceToHost, s));
  BBX_HIP(hipStreamSynchronize(s));
  for (int64_t d = 0; d < n_draw; ++d) {
    if (bad[d])
      return fail(BBX_ERR_NUMERIC,
                  "draw " + std::to_string(d) +
                      ": a risk-set sum of relative hazards is 0");
  }
  return BBX_OK;
}

template <class F>
int baseline_hazard(typename F::H* c, const double* beta, int64_t n_draw,
                    int64_t n_grid, const int32_t* grid_event,
                    double* log_hazard) {
  BBX_TRY(predict_head<F>(c, "baseline_hazard"));
  if (!beta || !grid_event || !log_hazard)
    return fail(BBX_ERR_INVALID, "NULL argument");
  if (n_draw < 1) return fail(BBX_ERR_INVALID, "n_draw must be at least 1");
  if (n_grid < 1) return fail(BBX_ERR_INVALID, "n_grid must be at least 1");
  // the kernel indexes c[grid_event]: check them all
  for (int64_t j = 0; j < n_grid; ++j) {
    if (grid_event[j] < -1 || grid_event[j] >= c->ne)
      return fail(BBX_ERR_INVALID, "grid_event[" + std::to_string(j) +
                                       "] outside [-1, n_event)");
  }
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return baseline_hazard_impl<F>(c, beta, n_draw, n_grid, grid_event,
                                   log_hazard);
  });
}

// The row pass's w at beta (the martingale residuals): one gradient
// evaluation; X~^T w goes to the scratch c->gl
template <class F>
int residuals(typename F::H* c, const double* beta, double* out) {
  BBX_TRY(predict_head<F>(c, "residuals"));
  if (!beta || !out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    bbx_design* h = c->h;
    typename F::Lik lik{c};
    double* d_in = h->stage_P.template as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
    BBX_HIP(hipGetLastError());
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(lik(c->gl.template as<double>()));
    BBX_HIP(hipMemcpyAsync(out, c->tmp.ptr, sizeof(double) * c->n,
                           hipMemcpyDeviceToHost, h->stream));
    BBX_TRY(read_state(c));
    if (c->host_st->zero)
      return fail(BBX_ERR_NUMERIC,
                  "residuals: a risk-set sum of relative hazards is 0");
    return BBX_OK;
  });
}
}  // namespace
}  // namespace bbx

// The two prediction entry points include/bbx.h declares for every Cox handle
// type (BBX_COX_PREDICT_DECL), on bbx_<fam> under the family F; stamped next
// to BBX_HAM_ENTRY_POINTS, in the policy's own translation unit.
#define BBX_COX_PREDICT_ENTRY_POINTS(fam, F)                                   \
  extern "C" {                                                                 \
  int bbx_##fam##_baseline_hazard(bbx_##fam* c, const double* beta,            \
                                  int64_t n_draw, int64_t n_grid,              \
                                  const int32_t* grid_event,                   \
                                  double* log_hazard) {                        \
    return ::bbx::baseline_hazard<F>(c, beta, n_draw, n_grid, grid_event,      \
                                     log_hazard);                              \
  }                                                                            \
  int bbx_##fam##_residuals(bbx_##fam* c, const double* beta, double* out) {   \
    return ::bbx::residuals<F>(c, beta, out);                                  \
  }                                                                            \
  }
