// The blocked two-pass scan, written once: the device plumbing under the
// stratified Cox scans (cox_strat.hpp), the conditional Poisson passes
// (cpoisson.hip) and pass B of the unstratified Cox handles (cox_scan.hpp).
// Device inline templates only; the kernels stay with their users.
//
// Contract, for every user:
//   - The partition is FIXED by the length alone: a range of `len` elements is
//     cut into G chunks of ceil(len / G) (chunk_range), each scanned in tiles
//     of BLOCK threads x E elements.  Nothing else about the data -- the number
//     or sizes of strata, the values -- enters it or the number of launches.
//   - Pass A leaves one aggregate per chunk; pass B combines those of the
//     chunks before its own (every wave computes the same chunk_prefix) and
//     scans its chunk again.
//   - The exclusive prefix of a thread is the previous lane's inclusive value,
//     never a difference: incl - run loses the lanes before a run that exceeds
//     them by 2^53 (1/H grows that fast across a few late risk sets), and
//     under max or log-sum-exp it would form -inf - -inf.
//   - Every combination is in a fixed order and there are no float atomics:
//     the same inputs give the same bits on every run.
//
// A monoid policy M states
//   T, ident()         the element (plain data) and the neutral one
//   comb(a, b)         a before b in scan order; associative
//   up(x, off), bcast(x, lane)    the field-wise __shfl_up and __shfl
//   In, Out, get(in, idx), put(out, idx, x)    one chunk aggregate, kept as
//                      the parallel arrays the handles allocate
// and what else its users need (op; push: one more element behind a run).
#pragma once
#include <math.h>

#include "common.hpp"

// (binds where a template is written, not where it is instantiated)
#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// The plain sum of doubles (no chunk aggregates: cox_scan.hpp's chunk prefix
// is strided per lane, another order of addition than chunk_prefix's)
struct Sum {
  using T = double;
  __device__ static T ident() { return 0.; }
  __device__ static T comb(T a, T b) { return a + b; }
  __device__ static T up(T x, int off) { return __shfl_up(x, off); }
};

struct AddOp {
  __device__ static double ident() { return 0.; }
  __device__ static double op(double a, double b) { return a + b; }
};

// The segmented scan of (head flag, value) pairs under Op:
//   (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 (+) v2)
template <class Op>
struct Seg {
  struct T { int f; double v; };   // f: a head flag was seen
  struct In { const double* v; const int* f; };
  struct Out { double* v; int* f; };
  __device__ static double op(double a, double b) { return Op::op(a, b); }
  __device__ static T ident() { return {0, Op::ident()}; }
  __device__ static T comb(T a, T b) {
    return {a.f | b.f, b.f ? b.v : op(a.v, b.v)};
  }
  // One more element of value x behind the run of a thread
  __device__ static void push(T& run, bool head, double x) {
    run = comb(run, {head, x});
  }
  __device__ static T up(T x, int off) {
    return {__shfl_up(x.f, off), __shfl_up(x.v, off)};
  }
  __device__ static T bcast(T x, int lane) {
    return {__shfl(x.f, lane), __shfl(x.v, lane)};
  }
  __device__ static T get(In in, int idx) { return {in.f[idx], in.v[idx]}; }
  __device__ static void put(Out out, int idx, T x) {
    out.v[idx] = x.v;
    out.f[idx] = x.f;
  }
};

using SegSum = Seg<AddOp>;
// (SegMax = Seg<NanMaxOp> is cox_strat.hpp's, next to nanmax)

// The segmented log-sum-exp of (head flag, m, s) triples, the sum being
// s exp(m), under the "online softmax" operator
//   (m1, s1) o (m2, s2) = (m, s1 exp(m1 - m) + s2 exp(m2 - m)),  m = max(m1, m2)
// which a head restarts.  One of the two exponents is always 0, so a
// combination costs one exp.  An s of 0 marks "no row yet" (a row contributes 1
// to its own s): the difference of two -inf is never formed.
struct SegLse {
  struct T { int f; double m, s; };   // f: a head flag was seen
  struct In { const double *m, *s; const int* f; };
  struct Out { double *m, *s; int* f; };
  __device__ static T ident() { return {0, -INFINITY, 0.}; }
  __device__ static T comb(T a, T b) {
    T r;
    r.f = a.f | b.f;
    const double d = a.m - b.m;
    const double e = exp(-fabs(d));
    const bool a_top = d >= 0.;
    r.m = a_top ? a.m : b.m;
    r.s = a_top ? a.s + b.s * e : a.s * e + b.s;
    if (b.f || a.s == 0.) {
      r.m = b.m;
      r.s = b.s;
    } else if (b.s == 0.) {
      r.m = a.m;
      r.s = a.s;
    }
    return r;
  }
  // One more row of value x behind the run of a thread: comb(run, {head, x,
  // 1}) bit for bit, without its multiplication by 1 and its second select
  __device__ static void push(T& run, bool head, double x) {
    if (head || run.s == 0.) {
      run.m = x;
      run.s = 1.;
    } else {
      const double d = x - run.m;
      const double e = exp(-fabs(d));
      if (d > 0.) {
        run.s = run.s * e + 1.;
        run.m = x;
      } else {
        run.s = run.s + e;
      }
    }
    run.f |= head;
  }
  __device__ static T up(T x, int off) {
    return {__shfl_up(x.f, off), __shfl_up(x.m, off), __shfl_up(x.s, off)};
  }
  __device__ static T bcast(T x, int lane) {
    return {__shfl(x.f, lane), __shfl(x.m, lane), __shfl(x.s, lane)};
  }
  __device__ static T get(In in, int idx) {
    return {in.f[idx], in.m[idx], in.s[idx]};
  }
  __device__ static void put(Out out, int idx, T x) {
    out.m[idx] = x.m;
    out.s[idx] = x.s;
    out.f[idx] = x.f;
  }
};

// Chunk b of the G chunks of [0, len): [t0, t1), empty past the end
struct ChunkRange { int64_t t0, t1; };

template <int G>
__device__ inline ChunkRange chunk_range(int64_t len, int b) {
  const int64_t L = (len + G - 1) / G;
  const int64_t t0 = (int64_t)b * L;
  return {t0, t0 + L < len ? t0 + L : len};
}

// Inclusive scan across the wave, in lane order
template <class M>
__device__ inline typename M::T wave_incl(typename M::T x, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const typename M::T y = M::up(x, off);
    if (lane >= off) x = M::comb(y, x);
  }
  return x;
}

// Block-wide scan of one element per thread, in thread order.  `pre`:
// everything before this thread; `tot`: the whole block.  s_wave: BLOCK / WAVE
// elements of LDS, free again on return.
template <class M, int BLOCK>
__device__ inline void block_scan(typename M::T run, typename M::T* s_wave,
                                  typename M::T& pre, typename M::T& tot) {
  using T = typename M::T;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const T incl = wave_incl<M>(run, lane);
  T excl = M::up(incl, 1);
  if (lane == 0) excl = M::ident();
  if (lane == WAVE - 1) s_wave[wid] = incl;
  __syncthreads();
  T wpre = M::ident();
  tot = M::ident();
#pragma unroll
  for (int k = 0; k < BLOCK / WAVE; ++k) {
    const T w = s_wave[k];
    if (k < wid) wpre = M::comb(wpre, w);
    tot = M::comb(tot, w);
  }
  pre = M::comb(wpre, excl);
  __syncthreads();
}

// The aggregates first .. first + b - 1, those of the chunks before chunk b,
// combined in order: G / WAVE chunks per lane, then across the lanes
template <class M, int G>
__device__ inline typename M::T chunk_prefix(typename M::In agg, int first,
                                             int b) {
  static_assert(G % WAVE == 0, "G / WAVE chunks per lane");
  const int lane = threadIdx.x & (WAVE - 1);
  typename M::T acc = M::ident();
#pragma unroll
  for (int k = 0; k < G / WAVE; ++k) {
    const int c = lane * (G / WAVE) + k;
    if (c < b) acc = M::comb(acc, M::get(agg, first + c));
  }
  acc = wave_incl<M>(acc, lane);
  return M::bcast(acc, WAVE - 1);
}

}  // namespace bbx
