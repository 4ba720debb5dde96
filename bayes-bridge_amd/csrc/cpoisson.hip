// Conditional Poisson likelihood: counts with one nuisance baseline rate per
// stratum, conditioned on every stratum's total, for the Hamiltonian
// coefficient samplers -- its gradient, its Hessian-vector product at a fixed
// location, and the trajectory / No-U-Turn drivers of hamiltonian.hpp with this
// family's block between "eta is complete" and "grad_loglik is complete".
//
// Rows are stratum-major.  With eta = X~ beta, count y >= 0, offset
// o = log(exposure) and N_s the sum of y over stratum s, per row i of s:
//   a_i  = eta_i + o_i
//   L_s  = log sum_{j in s} exp(a_j) = m_s + log sum exp(a_j - m_s), m_s = max a
//   ll   = sum_i y_i (a_i - L_s(i))    (the multinomial coefficient is dropped)
//   pi_i = exp(a_i - L_s),  w_i = y_i - N_s pi_i,  grad = X~^T w
// Hessian-vector product at a fixed location: u = X~ v,
//   ubar_s = sum_{j in s} pi_j u_j,  out = X~^T (-(N_s pi_i (u_i - ubar_s)))
// There is no intercept: it cancels inside every stratum.
//
// The shift is per stratum (one global max would leave a stratum 800 below
// another with every exp == 0), and the max and the sum are found together, in
// one segmented pass over (head flag, m, s) triples under the associative
// "online softmax" operator
//   (m1, s1) o (m2, s2) = (m, s1 exp(m1 - m) + s2 exp(m2 - m)),  m = max(m1, m2)
// which a stratum's first row restarts (cox_strat.hpp's seg_comb).  One of the
// two exponents is always 0, so a combination costs one exp.  Since the sum of
// a stratum is >= 1 after its shift, the likelihood is finite for every finite
// eta: this family has no overflow or empty-sum case and never raises
// CoxTraj::zero.  A NaN in eta comes out of the sums as a NaN.
//
// Contract (cox_strat.hpp, glm_rows.hpp): the partition is FIXED by n alone --
// the row range [0, n) is cut into CP_G chunks of ceil(n / CP_G) rows, scanned
// in tiles of CP_BLOCK x CP_E -- and neither the number nor the sizes of the
// strata enter it or the number of launches.  Pass A (cp_agg_kernel) leaves one
// triple per chunk; pass B (cp_out_kernel) combines the triples of the chunks
// before its own in order, scans its chunk again and writes L_s at the last
// row of every stratum; the row kernel (cp_row_kernel) computes pi, w and the
// NPART partials of sum ll and sum w over the (i / VEC_BLOCK) % NPART partition
// of glm_rows.hpp, which launch_tdot and the post kernels consume unchanged.
// The Hessian's ubar_s is the same two passes under the plain sum.  No float
// atomics, every combination in a fixed order: the same inputs give the same
// bits on every run.  Nothing synchronises with the host.
#include <math.h>

#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

static_assert(SCAN_G == NPART, "the row kernel writes one loglik partial per "
                               "workgroup into HamCore::llpart");

constexpr int CP_G = 256;       // chunks of the row range
constexpr int CP_BLOCK = 256;   // threads of the scan kernels
constexpr int CP_E = 8;         // rows per thread and tile
constexpr int CP_TILE = 2048;   // rows per tile
constexpr int CP_U = 2;         // rows in flight per thread of the row kernel

static_assert(CP_TILE == CP_BLOCK * CP_E, "a tile is one row set per thread");
static_assert(CP_G % WAVE == 0, "CP_G / WAVE chunks per lane");

enum CpFlag : uint8_t {
  CF_HEAD = 1,   // first row of a stratum
  CF_LAST = 2    // last row of a stratum
};

// What the row kernel reads of a row, in one 32-byte record
struct __attribute__((aligned(32))) CpRow {
  double y, o, N;   // count, log exposure, total count of the row's stratum
  int32_t sid;      // the row's stratum
  int32_t pad;
};

enum CpOp {
  CO_LSE = 0,   // (m, s): log-sum-exp of a_i = eta_i + o_i
  CO_SUM = 1    // s: sum of pi_i u_i
};

struct Tri {
  int f;        // a head flag was seen
  double m, s;  // CO_LSE: the sum is s exp(m); CO_SUM: m unused
};

template <int OP>
__device__ inline Tri tri_ident() {
  Tri r;
  r.f = 0;
  r.m = OP == CO_LSE ? -INFINITY : 0.;
  r.s = 0.;
  return r;
}

// a comes before b in row order.  An s of 0 marks "no row yet" (a row
// contributes 1 to its own s): the difference of two -inf is never formed.
template <int OP>
__device__ inline Tri tri_comb(Tri a, Tri b) {
  Tri r;
  r.f = a.f | b.f;
  if (OP == CO_SUM) {
    r.m = 0.;
    r.s = b.f ? b.s : a.s + b.s;
    return r;
  }
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

// One more row behind the run of a thread
template <int OP>
__device__ inline void tri_push(Tri& run, bool head, double x) {
  if (OP == CO_SUM) {
    run.s = head ? x : run.s + x;
  } else if (head || run.s == 0.) {
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

template <int OP>
__device__ inline Tri wave_tri_incl(Tri x, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    Tri y;
    y.f = __shfl_up(x.f, off);
    y.m = __shfl_up(x.m, off);
    y.s = __shfl_up(x.s, off);
    if (lane >= off) x = tri_comb<OP>(y, x);
  }
  return x;
}

// Block-wide segmented scan of one triple per thread, in thread order.  `pre`:
// everything before this thread; `tot`: the whole block.
template <int OP>
__device__ inline void block_tri_scan(Tri run, Tri* s_wave, Tri& pre, Tri& tot) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const Tri incl = wave_tri_incl<OP>(run, lane);
  Tri excl;
  excl.f = __shfl_up(incl.f, 1);
  excl.m = __shfl_up(incl.m, 1);
  excl.s = __shfl_up(incl.s, 1);
  if (lane == 0) excl = tri_ident<OP>();
  if (lane == WAVE - 1) s_wave[wid] = incl;
  __syncthreads();
  Tri wpre = tri_ident<OP>();
  tot = tri_ident<OP>();
#pragma unroll
  for (int k = 0; k < CP_BLOCK / WAVE; ++k) {
    const Tri w = s_wave[k];
    if (k < wid) wpre = tri_comb<OP>(wpre, w);
    tot = tri_comb<OP>(tot, w);
  }
  pre = tri_comb<OP>(wpre, excl);
  __syncthreads();
}

// The triples of the chunks before chunk b, combined in order (every wave
// computes the same value)
template <int OP>
__device__ inline Tri chunk_tri_prefix(const double* aggm, const double* aggs,
                                       const int* aggf, int b) {
  const int lane = threadIdx.x & (WAVE - 1);
  Tri acc = tri_ident<OP>();
#pragma unroll
  for (int k = 0; k < CP_G / WAVE; ++k) {
    const int c = lane * (CP_G / WAVE) + k;
    if (c < b) {
      Tri x;
      x.f = aggf[c];
      x.m = aggm[c];
      x.s = aggs[c];
      acc = tri_comb<OP>(acc, x);
    }
  }
  acc = wave_tri_incl<OP>(acc, lane);
  Tri r;
  r.f = __shfl(acc.f, WAVE - 1);
  r.m = __shfl(acc.m, WAVE - 1);
  r.s = __shfl(acc.s, WAVE - 1);
  return r;
}

// The value of row i under OP.  CO_LSE: x = eta, z = o; CO_SUM: x = u, z = pi
template <int OP>
__device__ inline double cp_value(double x, double z) {
  return OP == CO_LSE ? x + z : z * x;
}

// Pass A: one triple per chunk.  Block b: chunk b.
template <int OP>
static __global__ __launch_bounds__(CP_BLOCK) void cp_agg_kernel(
    int64_t n, const uint8_t* __restrict__ flag, const double* __restrict__ x,
    const double* __restrict__ z, double* __restrict__ aggm,
    double* __restrict__ aggs, int* __restrict__ aggf,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ Tri s_wave[CP_BLOCK / WAVE];
  const int b = blockIdx.x;
  const int64_t L = (n + CP_G - 1) / CP_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < n ? t0 + L : n;
  Tri carry = tri_ident<OP>();
  for (int64_t tile = t0; tile < t1; tile += CP_TILE) {
    const int64_t tb = tile + (int64_t)threadIdx.x * CP_E;
    double v[CP_E];
    unsigned head = 0;
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      const int64_t i = tb + e;
      v[e] = 0.;
      if (i < t1) {
        v[e] = cp_value<OP>(x[i], z[i]);
        if (flag[i] & CF_HEAD) head |= 1u << e;
      }
    }
    Tri run = tri_ident<OP>();
#pragma unroll
    for (int e = 0; e < CP_E; ++e)
      if (tb + e < t1) tri_push<OP>(run, (head >> e) & 1u, v[e]);
    Tri pre, tot;
    block_tri_scan<OP>(run, s_wave, pre, tot);
    carry = tri_comb<OP>(carry, tot);
  }
  if (threadIdx.x == 0) {
    aggm[b] = carry.m;
    aggs[b] = carry.s;
    aggf[b] = carry.f;
  }
}

// Pass B: the inclusive segmented scan of each chunk, after the triples of the
// chunks before it; the last row of stratum s writes out[s]: L_s (CO_LSE) or
// ubar_s (CO_SUM).
template <int OP>
static __global__ __launch_bounds__(CP_BLOCK) void cp_out_kernel(
    int64_t n, const uint8_t* __restrict__ flag,
    const int32_t* __restrict__ sid, const double* __restrict__ x,
    const double* __restrict__ z, double* __restrict__ out,
    const double* __restrict__ aggm, const double* __restrict__ aggs,
    const int* __restrict__ aggf, const int* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ Tri s_wave[CP_BLOCK / WAVE];
  const int b = blockIdx.x;
  const int64_t L = (n + CP_G - 1) / CP_G;
  const int64_t t0 = (int64_t)b * L, t1 = t0 + L < n ? t0 + L : n;
  if (t0 >= t1) return;
  Tri carry = chunk_tri_prefix<OP>(aggm, aggs, aggf, b);
  for (int64_t tile = t0; tile < t1; tile += CP_TILE) {
    const int64_t tb = tile + (int64_t)threadIdx.x * CP_E;
    double v[CP_E], rm[CP_E], rs[CP_E];
    unsigned seen = 0, last = 0, head = 0;
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      const int64_t i = tb + e;
      v[e] = 0.;
      if (i < t1) {
        v[e] = cp_value<OP>(x[i], z[i]);
        const unsigned fl = flag[i];
        if (fl & CF_HEAD) head |= 1u << e;
        if (fl & CF_LAST) last |= 1u << e;
      }
    }
    Tri run = tri_ident<OP>();
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      if (tb + e < t1) tri_push<OP>(run, (head >> e) & 1u, v[e]);
      rm[e] = run.m;
      rs[e] = run.s;
      if (run.f) seen |= 1u << e;
    }
    Tri pre, tot;
    block_tri_scan<OP>(run, s_wave, pre, tot);
    const Tri base = tri_comb<OP>(carry, pre);
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      const int64_t i = tb + e;
      if (i >= t1 || !((last >> e) & 1u)) continue;
      Tri r;
      r.f = 0;
      r.m = rm[e];
      r.s = rs[e];
      if (!((seen >> e) & 1u)) r = tri_comb<OP>(base, r);
      out[sid[i]] = OP == CO_LSE ? r.m + log(r.s) : r.s;
    }
    carry = tri_comb<OP>(carry, tot);
  }
}

enum CpMode {
  CM_GRAD = 0,   // w = y - N pi, partials of sum ll and of sum w
  CM_LOC = 1,    // pi
  CM_HESS = 2    // w = -(N pi (u - ubar)), partials of sum w
};

// `a`: eta (CM_GRAD, CM_LOC) or u = X~ v (CM_HESS); `ps`: L_s (CM_GRAD,
// CM_LOC) or ubar_s (CM_HESS) per stratum; `pi`: the location's pi (CM_HESS);
// `out`: w or pi.  glm_row_kernel's partition and lap order (glm_rows.hpp).
template <int MODE>
static __global__ __launch_bounds__(VEC_BLOCK) void cp_row_kernel(
    int64_t n, const double* __restrict__ a, const CpRow* __restrict__ row,
    const double* __restrict__ ps, const double* __restrict__ pi,
    double* __restrict__ out, double* __restrict__ llpart,
    double* __restrict__ sumw_part, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int64_t lap = (int64_t)gridDim.x * VEC_BLOCK;
  double acc = 0., ll = 0.;
  for (int64_t i0 = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i0 < n;
       i0 += CP_U * lap) {
    double x[CP_U], t[CP_U], q[CP_U];
    CpRow r[CP_U];
#pragma unroll
    for (int k = 0; k < CP_U; ++k) {
      const int64_t i = i0 + k * lap;
      x[k] = q[k] = 0.;
      r[k].y = r[k].o = r[k].N = 0.;
      r[k].sid = 0;
      if (i < n) {
        x[k] = a[i];
        r[k] = row[i];
        if (MODE == CM_HESS) q[k] = pi[i];
      }
    }
#pragma unroll
    for (int k = 0; k < CP_U; ++k) {
      const int64_t i = i0 + k * lap;
      t[k] = i < n ? ps[r[k].sid] : 0.;
    }
#pragma unroll
    for (int k = 0; k < CP_U; ++k) {
      const int64_t i = i0 + k * lap;
      if (i >= n) break;
      double v;
      if (MODE == CM_HESS) {
        v = -((r[k].N * q[k]) * (x[k] - t[k]));
      } else {
        const double d = (x[k] + r[k].o) - t[k];
        const double p = exp(d);
        if (MODE == CM_LOC) {
          v = p;
        } else {
          v = r[k].y - r[k].N * p;
          ll += r[k].y * d;
        }
      }
      out[i] = v;
      acc += v;
    }
  }
  if (MODE == CM_LOC) return;
  acc = block_sum<VEC_BLOCK>(acc);
  if (MODE == CM_GRAD) ll = block_sum<VEC_BLOCK>(ll);
  if (threadIdx.x == 0) {
    sumw_part[blockIdx.x] = acc;
    if (MODE == CM_GRAD) llpart[blockIdx.x] = ll;
  }
}

}  // namespace bbx

using namespace bbx;

// One conditional Poisson likelihood on a design (borrowed: the design must
// outlive it).
struct bbx_cpoisson : HamCore {
  int64_t ns = 0;
  DevMem row;             // n CpRow
  DevMem o;               // n: log exposure, for the scan passes
  DevMem flag, sid;       // n: CpFlag, stratum of a row
  DevMem ls, ubar;        // ns: L_s, ubar_s
  DevMem pi_loc;          // n: the Hessian's location
  DevMem aggm, aggs, aggf;   // CP_G chunk triples
};

namespace {

using ham::cst;
using ham::eta_of;

// out[s] over the strata: L_s of x + z (CO_LSE) or the sum of z x (CO_SUM)
template <int OP>
int launch_strata(bbx_cpoisson* c, const double* x, const double* z,
                  double* out, const int* skip) {
  bbx_design* h = c->h;
  BBX_LAUNCH(cp_agg_kernel<OP>, dim3(CP_G), dim3(CP_BLOCK), 0, h->stream, c->n,
             c->flag.as<const uint8_t>(), x, z, c->aggm.as<double>(),
             c->aggs.as<double>(), c->aggf.as<int>(), skip);
  BBX_HIP(hipGetLastError());
  BBX_LAUNCH(cp_out_kernel<OP>, dim3(CP_G), dim3(CP_BLOCK), 0, h->stream, c->n,
             c->flag.as<const uint8_t>(), c->sid.as<const int32_t>(), x, z,
             out, c->aggm.as<const double>(), c->aggs.as<const double>(),
             c->aggf.as<const int>(), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <int MODE>
int launch_rows(bbx_cpoisson* c, const double* a, const double* ps,
                double* out, const int* skip) {
  bbx_design* h = c->h;
  BBX_LAUNCH(cp_row_kernel<MODE>, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->n, a, c->row.as<const CpRow>(), ps,
             c->pi_loc.as<const double>(), out, c->llpart.as<double>(),
             part_slot(h, PS_SUMW), skip);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// From eta (in c->eta, complete in stream order): w, the loglik partials and
// (grad != null) grad = X~^T w.
int likelihood_from_eta(bbx_cpoisson* c, double* grad) {
  bbx_design* h = c->h;
  const int* skip = &cst(c)->skip;
  BBX_TRY(launch_strata<CO_LSE>(c, c->eta.as<const double>(),
                                c->o.as<const double>(), c->ls.as<double>(),
                                skip));
  BBX_TRY(launch_rows<CM_GRAD>(c, c->eta.as<const double>(),
                               c->ls.as<const double>(), c->tmp.as<double>(),
                               skip));
  if (!grad) return BBX_OK;
  TdotEpilogue ep;
  return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, grad);
}

// The conditional Poisson block of a leapfrog step
struct CPoissonLik {
  bbx_cpoisson* c;
  int operator()(double* grad) const { return likelihood_from_eta(c, grad); }
};

int cpoisson_create_impl(bbx_design* h, const double* y,
                         const double* log_exposure, int64_t ns,
                         const int64_t* sptr, bbx_cpoisson** out) {
  if (!out) return fail(BBX_ERR_INVALID, "NULL output pointer");
  *out = nullptr;
  if (!h || !design_alive(h)) return fail(BBX_ERR_INVALID, "invalid design");
  if (!y) return fail(BBX_ERR_INVALID, "NULL y");
  if (!sptr) return fail(BBX_ERR_INVALID, "NULL stratum_ptr");
  const int64_t n = h->n;
  if (n >= (int64_t(1) << 31))
    return fail(BBX_ERR_INVALID,
                "the conditional Poisson model needs fewer than 2^31 rows");
  if (ns < 1 || ns > n)
    return fail(BBX_ERR_INVALID, "n_strata must be in [1, n]");
  for (int64_t i = 0; i < n; ++i) {
    const double yi = y[i], oi = log_exposure ? log_exposure[i] : 0.;
    if (!std::isfinite(yi))
      return fail(BBX_ERR_INVALID, "y[" + std::to_string(i) + "] is not finite");
    if (yi < 0.)
      return fail(BBX_ERR_INVALID, "y[" + std::to_string(i) + "] is negative");
    if (!std::isfinite(oi))
      return fail(BBX_ERR_INVALID,
                  "log_exposure[" + std::to_string(i) + "] is not finite");
  }
  if (sptr[0] != 0)
    return fail(BBX_ERR_INVALID, "stratum_ptr[0] must be 0");
  for (int64_t s = 0; s < ns; ++s)
    if (sptr[s + 1] <= sptr[s] || sptr[s + 1] > n)
      return fail(BBX_ERR_INVALID, "stratum " + std::to_string(s) +
                                       ": stratum_ptr is not increasing "
                                       "within [0, n]");
  if (sptr[ns] != n)
    return fail(BBX_ERR_INVALID, "stratum_ptr[n_strata] must be n");
  std::vector<CpRow> row((size_t)n);
  std::vector<double> off((size_t)n);
  std::vector<uint8_t> flag((size_t)n, 0);
  std::vector<int32_t> sid((size_t)n);
  for (int64_t s = 0; s < ns; ++s) {
    const int64_t r0 = sptr[s], r1 = sptr[s + 1];
    double total = 0.;
    for (int64_t r = r0; r < r1; ++r) total += y[r];
    if (!(total > 0.))
      return fail(BBX_ERR_INVALID, "stratum " + std::to_string(s) +
                                       ": the counts y sum to 0");
    for (int64_t r = r0; r < r1; ++r) {
      off[r] = log_exposure ? log_exposure[r] : 0.;
      row[r].y = y[r];
      row[r].o = off[r];
      row[r].N = total;
      row[r].sid = (int32_t)s;
      row[r].pad = 0;
      sid[r] = (int32_t)s;
    }
    flag[r0] |= CF_HEAD;
    flag[r1 - 1] |= CF_LAST;
  }
  bbx_cpoisson* c = new bbx_cpoisson;
  c->ns = ns;
  const size_t d8 = sizeof(double), i4 = sizeof(int32_t);
  int st = ham::init_core(c, h, "cpoisson");
  DevMem* nvec[] = {&c->pi_loc, &c->o};
  for (DevMem* m : nvec)
    if (st == BBX_OK) st = m->alloc(d8 * n);
  if (st == BBX_OK) st = c->row.alloc(sizeof(CpRow) * n);
  if (st == BBX_OK) st = c->flag.alloc(n);
  if (st == BBX_OK) st = c->sid.alloc(i4 * n);
  if (st == BBX_OK) st = c->ls.alloc(d8 * ns);
  if (st == BBX_OK) st = c->ubar.alloc(d8 * ns);
  if (st == BBX_OK) st = c->aggm.alloc(d8 * CP_G);
  if (st == BBX_OK) st = c->aggs.alloc(d8 * CP_G);
  if (st == BBX_OK) st = c->aggf.alloc(sizeof(int) * CP_G);
  if (st != BBX_OK) return ham::discard(c, st);
  const hipMemcpyKind H2D = hipMemcpyHostToDevice;
  hipError_t e = hipMemcpyAsync(c->row.ptr, row.data(), sizeof(CpRow) * n, H2D,
                                h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->o.ptr, off.data(), d8 * n, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->flag.ptr, flag.data(), n, H2D, h->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->sid.ptr, sid.data(), i4 * n, H2D, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    return ham::discard(c, fail(BBX_ERR_HIP, std::string("cpoisson upload: ") +
                                                 hipGetErrorString(e)));
  *out = c;
  return BBX_OK;
}

struct CPoissonFamily {
  static constexpr const char* name = "cpoisson";
  using Lik = CPoissonLik;
  static int locate(bbx_cpoisson* c, const double* d_in) {
    BBX_TRY(eta_of(c, d_in));
    BBX_TRY(launch_strata<CO_LSE>(c, c->eta.as<const double>(),
                                  c->o.as<const double>(), c->ls.as<double>(),
                                  nullptr));
    BBX_TRY(launch_rows<CM_LOC>(c, c->eta.as<const double>(),
                                c->ls.as<const double>(),
                                c->pi_loc.as<double>(), nullptr));
    BBX_HIP(hipStreamSynchronize(c->h->stream));   // beta is free again
    return BBX_OK;
  }
  static int hessian_from_v(bbx_cpoisson* c, const double* d_v,
                            double* d_out) {
    bbx_design* h = c->h;
    BBX_TRY(eta_of(c, d_v));   // u = X~ v, in c->eta
    BBX_TRY(launch_strata<CO_SUM>(c, c->eta.as<const double>(),
                                  c->pi_loc.as<const double>(),
                                  c->ubar.as<double>(), nullptr));
    BBX_TRY(launch_rows<CM_HESS>(c, c->eta.as<const double>(),
                                 c->ubar.as<const double>(),
                                 c->tmp.as<double>(), nullptr));
    TdotEpilogue ep;
    return launch_tdot(h, c->tmp.as<double>(), part_slot(h, PS_SUMW), ep, d_out);
  }
};

}  // namespace

extern "C" int bbx_cpoisson_create(bbx_design* design, const double* y,
                                   const double* log_exposure,
                                   int64_t n_strata,
                                   const int64_t* stratum_ptr,
                                   bbx_cpoisson** out) {
  return no_throw([&] {
    return cpoisson_create_impl(design, y, log_exposure, n_strata, stratum_ptr,
                                out);
  });
}

BBX_HAM_ENTRY_POINTS(cpoisson, CPoissonFamily)
