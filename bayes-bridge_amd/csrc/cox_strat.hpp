// Stratified Cox partial likelihood: the kernels of a handle made by
// bbx_cox_create_stratified (included by cox.hip, whose host code drives them).
//
// Rows are stratum-major; inside stratum s the model's order holds (events by
// increasing time, then censored rows by decreasing censoring time).  Every
// quantity of cox.hip's header restarts per stratum:
//
//   m_s    = max eta over stratum s,  h_i = exp(eta_i - m_s(i))
//   scan_i = sum of h from i to the last event of i's stratum     (i an event)
//          = sum of h from the stratum's first censored row to i  (i censored)
//   H_k    = scan[start_k] + (end_k censored ? scan[end_k] : 0)
//   c      = cumsum_k 1/H_k, restarted at the first event of every stratum
//   w_i    = [i an event] - c[last_i] h_i
//
// The shift is per stratum: with one global max, a stratum whose eta lies 800
// below another's has h == 0 in every row and H_k == 0, although its own
// partial likelihood is perfectly finite (it is invariant to a shift of eta
// within the stratum).
//
// Scans.  One segmented scan serves all of them (seg_scan.hpp, whose header
// holds the contract): elements carry a head flag; SegSum restarts a sum and
// SegMax a max at every head.  The row range [0, n) (forward, and reversed for
// the suffix sums over events) and the event range [0, n_event) are each cut
// into SCAN_G chunks; pass A leaves one (flag, value) aggregate per chunk, pass
// B scans its chunk in tiles of SCAN_BLOCK x SCAN_E after those before it.
#pragma once
#include <type_traits>

#include "seg_scan.hpp"

namespace bbx {

enum RowFlag : uint8_t {
  RF_FWD = 1,     // forward head: first row or first censored row of a stratum
  RF_BWD = 2,     // backward head: last event or last row of a stratum
  RF_EVENT = 4,   // the row is an event
  RF_SHEAD = 8,   // first row of a stratum
  RF_SLAST = 16   // last row of a stratum
};
constexpr int EF_HEAD = 1;   // event flag: first event of a stratum

struct NanMaxOp {
  __device__ static double ident() { return -INFINITY; }
  __device__ static double op(double a, double b) { return nanmax(a, b); }
};
using SegMax = Seg<NanMaxOp>;   // the NaN-keeping max, restarted at a head

enum StratMode {
  SS_MAX = 0,   // eta_i, max                               (rows, forward)
  SS_H = 1,     // h_i = exp(eta_i - m_s(i))                (rows, both ways)
  SS_HU = 2,    // h_i u_i                                  (rows, both ways)
  SS_INVH = 3,  // 1 / H_k, and the loglik partials         (events, forward)
  SS_WU = 4     // (1/H_k) ((1/H_k) S_k)                    (events, forward)
};

struct StratArgs {
  int64_t len = 0;                  // n (rows) or n_event (events)
  const uint8_t* flag = nullptr;    // RowFlag per row / EF_HEAD per event
  const double* eta = nullptr;      // SS_MAX, SS_H, SS_INVH
  const double* ms = nullptr;       // SS_H, SS_INVH: max eta per stratum
  const int32_t* sid = nullptr;     // stratum of a row
  const double* h = nullptr;        // SS_HU
  const double* u = nullptr;        // SS_HU
  const double* scan = nullptr;     // SS_INVH, SS_WU: risk scan per row
  const double* inv = nullptr;      // SS_WU: 1 / H at the location
  const int32_t* evrow = nullptr;   // SS_INVH: row of an event
  const int32_t* start = nullptr;   // per event: row
  const int32_t* endc = nullptr;    // per event: row if censored, else -1
  double* val = nullptr;            // the per-element value, stored
  double* llpart = nullptr;         // SS_INVH: SCAN_G loglik partials
  CoxTraj* st = nullptr;            // SS_INVH: zero / skip flags
  double* aggv = nullptr;           // (directions) x SCAN_G chunk aggregates
  int* aggf = nullptr;
};

template <int MODE>
__device__ inline int strat_mask(int d) {
  if (MODE == SS_MAX) return RF_SHEAD;
  if (MODE == SS_H || MODE == SS_HU) return d ? RF_BWD : RF_FWD;
  return EF_HEAD;
}

// Pass A: the value of every element (stored in a.val) and one (flag, value)
// aggregate per chunk.  Block d * SCAN_G + b: chunk b of direction d (d == 1:
// the range read backwards).
template <int MODE>
__global__ __launch_bounds__(SCAN_BLOCK) void coxs_agg_kernel(
    StratArgs a, const int* __restrict__ skip) {
  if (skip && *skip) return;
  using M = std::conditional_t<MODE == SS_MAX, SegMax, SegSum>;
  using FV = typename M::T;
  __shared__ FV s_wave[SCAN_BLOCK / WAVE];
  const int d = blockIdx.x / SCAN_G, b = blockIdx.x % SCAN_G;
  const int mask = strat_mask<MODE>(d);
  const int64_t len = a.len;
  const auto [t0, t1] = chunk_range<SCAN_G>(len, b);
  FV carry = M::ident();
  double ll = 0.;
  bool zero = false;
  for (int64_t tile = t0; tile < t1; tile += SCAN_TILE) {
    const int64_t tb = tile + (int64_t)threadIdx.x * SCAN_E;
    FV run = M::ident();
#pragma unroll
    for (int e = 0; e < SCAN_E; ++e) {
      const int64_t t = tb + e;
      if (t >= t1) continue;
      const int64_t i = d ? len - 1 - t : t;
      FV x;
      x.f = (a.flag[i] & mask) != 0;
      if (MODE == SS_MAX) {
        x.v = a.eta[i];
      } else if (MODE == SS_H) {
        x.v = exp(a.eta[i] - a.ms[a.sid[i]]);
      } else if (MODE == SS_HU) {
        x.v = a.h[i] * a.u[i];
      } else {
        const int32_t e1 = a.endc[i];
        double H = a.scan[a.start[i]];
        if (e1 >= 0) H += a.scan[e1];
        if (MODE == SS_INVH) {
          const int32_t r = a.evrow[i];
          zero |= (H == 0.);
          x.v = 1. / H;
          ll += (a.eta[r] - a.ms[a.sid[r]]) - log(H);
        } else {
          const double iv = a.inv[i];
          x.v = iv * (iv * H);
        }
      }
      // both directions compute the same value; the forward one stores it
      if (MODE != SS_MAX && d == 0) a.val[i] = x.v;
      run = M::comb(run, x);
    }
    FV pre, tot;
    block_scan<M, SCAN_BLOCK>(run, s_wave, pre, tot);
    carry = M::comb(carry, tot);
  }
  if (MODE == SS_INVH) {
    ll = block_sum<SCAN_BLOCK>(ll);
    if (zero) {
      a.st->zero = 1;
      a.st->skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    M::put({a.aggv, a.aggf}, blockIdx.x, carry);
    if (MODE == SS_INVH) a.llpart[b] = ll;
  }
}

enum StratOut {
  SO_RISK = 0,  // rows, both ways: forward writes censored rows, backward events
  SO_MAX = 1,   // rows, forward: the last row of stratum s writes ms[s]
  SO_ALL = 2    // events, forward: every element
};

// Pass B: inclusive segmented scan of the stored values of each chunk, after
// the aggregates of the chunks before it.
template <int OUT>
__global__ __launch_bounds__(SCAN_BLOCK) void coxs_out_kernel(
    int64_t len, const uint8_t* __restrict__ flag,
    const int32_t* __restrict__ sid, const double* __restrict__ val,
    double* __restrict__ out, const double* __restrict__ aggv,
    const int* __restrict__ aggf, const int* __restrict__ skip) {
  if (skip && *skip) return;
  using M = std::conditional_t<OUT == SO_MAX, SegMax, SegSum>;
  using FV = typename M::T;
  __shared__ FV s_wave[SCAN_BLOCK / WAVE];
  const int d = blockIdx.x / SCAN_G, b = blockIdx.x % SCAN_G;
  const int mask = OUT == SO_MAX ? RF_SHEAD
                   : OUT == SO_RISK ? (d ? RF_BWD : RF_FWD) : EF_HEAD;
  const auto [t0, t1] = chunk_range<SCAN_G>(len, b);
  if (t0 >= t1) return;
  FV carry = chunk_prefix<M, SCAN_G>({aggv, aggf}, d * SCAN_G, b);
  for (int64_t tile = t0; tile < t1; tile += SCAN_TILE) {
    const int64_t tb = tile + (int64_t)threadIdx.x * SCAN_E;
    double x[SCAN_E];
    unsigned seen = 0, fl[SCAN_E];
    FV run = M::ident();
#pragma unroll
    for (int e = 0; e < SCAN_E; ++e) {
      const int64_t t = tb + e;
      fl[e] = 0;
      if (t < t1) {
        const int64_t i = d ? len - 1 - t : t;
        fl[e] = flag[i];
        FV y;
        y.f = (fl[e] & mask) != 0;
        y.v = val[i];
        run = M::comb(run, y);
      }
      x[e] = run.v;
      if (run.f) seen |= 1u << e;
    }
    FV pre, tot;
    block_scan<M, SCAN_BLOCK>(run, s_wave, pre, tot);
    const FV base = M::comb(carry, pre);
#pragma unroll
    for (int e = 0; e < SCAN_E; ++e) {
      const int64_t t = tb + e;
      if (t >= t1) continue;
      const int64_t i = d ? len - 1 - t : t;
      const double r = (seen >> e) & 1u ? x[e] : M::op(base.v, x[e]);
      if (OUT == SO_MAX) {
        if (fl[e] & RF_SLAST) out[sid[i]] = r;
      } else if (OUT == SO_RISK) {
        if (((fl[e] & RF_EVENT) != 0) == (d == 1)) out[i] = r;
      } else {
        out[i] = r;
      }
    }
    carry = M::comb(carry, tot);
  }
}

// w = [i an event] - c[last_i] h_i                       (HESS = false)
// w = -((c[last_i] h_i) u_i - h_i cz[last_i])            (HESS = true)
// and the NPART partials of sum(w).
template <bool HESS>
__global__ __launch_bounds__(VEC_BLOCK) void coxs_weight_kernel(
    int64_t n, const uint8_t* __restrict__ rflag, const double* __restrict__ h,
    const double* __restrict__ c, const int32_t* __restrict__ last,
    const double* __restrict__ u, const double* __restrict__ cz,
    double* __restrict__ w, double* __restrict__ part,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK) {
    const int32_t k = last[i];
    const double rs = c[k] * h[i];
    double v;
    if (HESS) {
      v = -(rs * u[i] - h[i] * cz[k]);
    } else {
      v = ((rflag[i] & RF_EVENT) ? 1. : 0.) - rs;
    }
    w[i] = v;
    acc += v;
  }
  acc = block_sum<VEC_BLOCK>(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

}  // namespace bbx
