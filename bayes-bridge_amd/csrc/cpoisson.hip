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
// one segmented pass over (head flag, m, s) triples under seg_scan.hpp's SegLse,
// which a stratum's first row restarts.  Since the sum of a stratum is >= 1
// after its shift, the likelihood is finite for every finite eta: this family
// has no overflow or empty-sum case and never raises CoxTraj::zero.  A NaN in
// eta comes out of the sums as a NaN.
//
// Scans (seg_scan.hpp, whose header holds the contract: the partition fixed by
// n alone, the order of combination, no float atomics): the row range [0, n)
// is cut into CP_G chunks, scanned in tiles of CP_BLOCK x CP_E.  Pass A
// (cp_agg_kernel) leaves one aggregate per chunk; pass B (cp_out_kernel)
// scans its chunk again after the aggregates before it and writes L_s at the
// last row of every stratum; the row kernel (cp_row_kernel) computes pi, w and
// the NPART partials of sum ll and sum w over the (i / VEC_BLOCK) % NPART
// partition of glm_rows.hpp, which launch_tdot and the post kernels consume
// unchanged.  The Hessian's ubar_s is the same two passes under SegSum, which
// leaves aggm alone.  Nothing synchronises with the host.
#include <math.h>

#include <vector>

#include "common.hpp"
#include "hamiltonian.hpp"
#include "seg_scan.hpp"

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
  CO_LSE = 0,   // log-sum-exp of a_i = eta_i + o_i
  CO_SUM = 1    // sum of pi_i u_i
};

// What the passes need of OP: the monoid, the value of a row (CO_LSE: x = eta,
// z = o; CO_SUM: x = u, z = pi), a stratum's result from its scan, and the
// handle's chunk aggregates as the monoid keeps them
template <int OP>
struct CpScan;

template <>
struct CpScan<CO_LSE> {
  using M = SegLse;
  __device__ static double value(double x, double z) { return x + z; }
  __device__ static double result(M::T r) { return r.m + log(r.s); }
  __device__ static M::In agg(const double* m, const double* s,
                              const int* f) {
    return {m, s, f};
  }
  __device__ static M::Out agg(double* m, double* s, int* f) {
    return {m, s, f};
  }
};

template <>
struct CpScan<CO_SUM> {
  using M = SegSum;
  __device__ static double value(double x, double z) { return z * x; }
  __device__ static double result(M::T r) { return r.v; }
  __device__ static M::In agg(const double*, const double* s, const int* f) {
    return {s, f};
  }
  __device__ static M::Out agg(double*, double* s, int* f) { return {s, f}; }
};

// Pass A: one aggregate per chunk.  Block b: chunk b.
template <int OP>
static __global__ __launch_bounds__(CP_BLOCK) void cp_agg_kernel(
    int64_t n, const uint8_t* __restrict__ flag, const double* __restrict__ x,
    const double* __restrict__ z, double* __restrict__ aggm,
    double* __restrict__ aggs, int* __restrict__ aggf,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  using S = CpScan<OP>;
  using M = typename S::M;
  using T = typename M::T;
  __shared__ T s_wave[CP_BLOCK / WAVE];
  const int b = blockIdx.x;
  const auto [t0, t1] = chunk_range<CP_G>(n, b);
  T carry = M::ident();
  for (int64_t tile = t0; tile < t1; tile += CP_TILE) {
    const int64_t tb = tile + (int64_t)threadIdx.x * CP_E;
    double v[CP_E];
    unsigned head = 0;
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      const int64_t i = tb + e;
      v[e] = 0.;
      if (i < t1) {
        v[e] = S::value(x[i], z[i]);
        if (flag[i] & CF_HEAD) head |= 1u << e;
      }
    }
    T run = M::ident();
#pragma unroll
    for (int e = 0; e < CP_E; ++e)
      if (tb + e < t1) M::push(run, (head >> e) & 1u, v[e]);
    T pre, tot;
    block_scan<M, CP_BLOCK>(run, s_wave, pre, tot);
    carry = M::comb(carry, tot);
  }
  if (threadIdx.x == 0) M::put(S::agg(aggm, aggs, aggf), b, carry);
}

// Pass B: the inclusive segmented scan of each chunk, after the aggregates of
// the chunks before it; the last row of stratum s writes out[s]: L_s (CO_LSE)
// or ubar_s (CO_SUM).
template <int OP>
static __global__ __launch_bounds__(CP_BLOCK) void cp_out_kernel(
    int64_t n, const uint8_t* __restrict__ flag,
    const int32_t* __restrict__ sid, const double* __restrict__ x,
    const double* __restrict__ z, double* __restrict__ out,
    const double* __restrict__ aggm, const double* __restrict__ aggs,
    const int* __restrict__ aggf, const int* __restrict__ skip) {
  if (skip && *skip) return;
  using S = CpScan<OP>;
  using M = typename S::M;
  using T = typename M::T;
  __shared__ T s_wave[CP_BLOCK / WAVE];
  const int b = blockIdx.x;
  const auto [t0, t1] = chunk_range<CP_G>(n, b);
  if (t0 >= t1) return;
  T carry = chunk_prefix<M, CP_G>(S::agg(aggm, aggs, aggf), 0, b);
  for (int64_t tile = t0; tile < t1; tile += CP_TILE) {
    const int64_t tb = tile + (int64_t)threadIdx.x * CP_E;
    double v[CP_E];
    T at[CP_E];   // the thread's run up to each of its rows
    unsigned seen = 0, last = 0, head = 0;
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      const int64_t i = tb + e;
      v[e] = 0.;
      if (i < t1) {
        v[e] = S::value(x[i], z[i]);
        const unsigned fl = flag[i];
        if (fl & CF_HEAD) head |= 1u << e;
        if (fl & CF_LAST) last |= 1u << e;
      }
    }
    T run = M::ident();
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      if (tb + e < t1) M::push(run, (head >> e) & 1u, v[e]);
      at[e] = run;
      if (run.f) seen |= 1u << e;
    }
    T pre, tot;
    block_scan<M, CP_BLOCK>(run, s_wave, pre, tot);
    const T base = M::comb(carry, pre);
#pragma unroll
    for (int e = 0; e < CP_E; ++e) {
      const int64_t i = tb + e;
      if (i >= t1 || !((last >> e) & 1u)) continue;
      T r = at[e];
      r.f = 0;
      if (!((seen >> e) & 1u)) r = M::comb(base, r);
      out[sid[i]] = S::result(r);
    }
    carry = M::comb(carry, tot);
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
  DevMem aggm, aggs, aggf;   // CP_G chunk aggregates (aggm: CO_LSE only)
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
