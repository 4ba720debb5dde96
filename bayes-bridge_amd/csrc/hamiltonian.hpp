// The preconditioned Hamiltonian trajectory shared by the likelihood families
// (the Cox handles on cox_family.hpp; logit.hip, poisson.hip and negbin.hip on
// glm_rows.hpp; cpoisson.hip): the leapfrog kernels, the No-U-Turn tree, their
// drivers and the front of the C ABI (the ten entry points every handle has).
// Velocity Verlet in preconditioned coordinates
// q = coef / scale, f(q) = loglik(scale q) - 1/2 sum prior_prec q^2
// (hmc.py:137-174, dynamics.py, nuts.py).
//
// Per step (host enqueues, no synchronisation): step1 (half kick with the
// previous gradient, drift, the dot input), X~ v, the family's likelihood
// block (from "eta is complete" to "grad_loglik is complete", which also
// leaves SCAN_G log-likelihood partials in HamCore::llpart), post_a (gradient
// of f, the second half kick into p2, partial sums), post_b (one workgroup:
// logp, the Hamiltonian, min / max, the stop rule).  Once the rule fires,
// CoxTraj::skip is set; it is the design's skip flag during the trajectory,
// so every later kernel -- ours and the design's products -- returns at entry.
//
// The kernels are static: each translation unit that includes this file gets
// its own copy, and the family differs only in the callable it hands to the
// drivers.
#pragma once
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

constexpr int SCAN_G = 256;      // log-likelihood partials (Cox: chunks per segment)

// Device-resident scalars of the likelihood and of one trajectory.
struct CoxTraj {
  double logp;          // f at the current position (trajectory) / loglik
  double h0, hmin, hmax, hcur;
  double tol;
  int skip;             // kernels exit at entry (trajectory over, or H_k == 0)
  int done;             // the stop rule fired at an earlier step
  int zero;             // some H_k == 0 at the current position
  int kicked;           // the last step's second half kick happened: p2 holds p
  int n_grad;           // steps evaluated
  int instab;
};

// block sum in a fixed order; thread 0 gets the result
template <int NT>
__device__ inline double block_sum(double x) {
  __shared__ double s_w[NT / WAVE];
  x = wave_allsum(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_w[threadIdx.x / WAVE] = x;
  __syncthreads();
  double r = 0.;
#pragma unroll
  for (int k = 0; k < NT / WAVE; ++k) r += s_w[k];
  __syncthreads();
  return r;
}

// loglik of a single evaluation (no trajectory): the SCAN_G partials in order
static __global__ __launch_bounds__(WAVE) void cox_loglik_kernel(
    const double* __restrict__ llpart, CoxTraj* st) {
  double a = 0.;
#pragma unroll
  for (int k = 0; k < SCAN_G / WAVE; ++k) a += llpart[threadIdx.x + k * WAVE];
  a = wave_allsum(a);
  if (threadIdx.x == 0) st->logp = st->zero ? -INFINITY : a;
}

static __global__ void cox_reset_kernel(CoxTraj* st) {
  if (threadIdx.x == 0) {
    st->skip = 0;
    st->zero = 0;
  }
}

// Step 1 of a leapfrog step: p += (dt/2) g  (on p2 if the previous step's
// second kick went there); q += dt p; v = scale .* q and the partials of
// <offset, v[intercept:]> that the X~ v kernels expect (prep_v_kernel's form).
static __global__ __launch_bounds__(VEC_BLOCK) void cox_step1_kernel(
    int64_t P, int intercept, double half_dt, double dt,
    double* __restrict__ q, double* __restrict__ p,
    const double* __restrict__ p2, const double* __restrict__ g,
    const double* __restrict__ scale, const double* __restrict__ offset,
    double* __restrict__ v, double* __restrict__ c_part, const CoxTraj* st) {
  if (st->skip) return;
  const bool kicked = st->kicked;
  double acc = 0.;
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK) {
    const double pk = (kicked ? p2[j] : p[j]) + half_dt * g[j];
    p[j] = pk;
    const double qn = q[j] + dt * pk;
    q[j] = qn;
    const double val = qn * scale[j];
    v[j] = val;
    if (j >= intercept) acc += offset[j - intercept] * val;
  }
  acc = block_sum<VEC_BLOCK>(acc);
  if (threadIdx.x == 0) c_part[blockIdx.x] = acc;
}

// gradient of f, the second half kick into p2 and three partial sums:
// [0] sum -prior_prec q^2, [1] p2 . p2, [2] p . p
static __global__ __launch_bounds__(VEC_BLOCK) void cox_post_a_kernel(
    int64_t P, double half_dt, const double* __restrict__ q,
    const double* __restrict__ p, double* __restrict__ p2,
    double* __restrict__ g, const double* __restrict__ gl,
    const double* __restrict__ scale, const double* __restrict__ pp,
    double* __restrict__ part, const CoxTraj* st) {
  if (st->skip) return;
  double a0 = 0., a1 = 0., a2 = 0.;
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK) {
    const double qj = q[j], pj = p[j];
    double gj = scale[j] * gl[j];
    gj += -pp[j] * qj;
    g[j] = gj;
    const double p2j = pj + half_dt * gj;
    p2[j] = p2j;
    a0 += -pp[j] * (qj * qj);
    a1 += p2j * p2j;
    a2 += pj * pj;
  }
  a0 = block_sum<VEC_BLOCK>(a0);
  a1 = block_sum<VEC_BLOCK>(a1);
  a2 = block_sum<VEC_BLOCK>(a2);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = a0;
    part[NPART + blockIdx.x] = a1;
    part[2 * NPART + blockIdx.x] = a2;
  }
}

__device__ inline double part_sum_wave(const double* part, int len) {
  double a = 0.;
  for (int k = threadIdx.x; k < len; k += WAVE) a += part[k];
  return wave_allsum(a);
}

// One wave: logp, the Hamiltonian, the running min / max and the stop rule of
// hmc.py:157-171 (min / max as Python's min() / max(): a NaN never replaces).
static __global__ __launch_bounds__(WAVE) void cox_post_b_kernel(
    const double* __restrict__ llpart, const double* __restrict__ part,
    CoxTraj* st) {
  if (st->done) return;
  const double ll = part_sum_wave(llpart, SCAN_G);
  const double prior = part_sum_wave(part, NPART);
  const double k2 = part_sum_wave(part + NPART, NPART);
  const double k1 = part_sum_wave(part + 2 * NPART, NPART);
  if (threadIdx.x != 0) return;
  double logp;
  int kicked = 0;
  double ham;
  if (st->zero) {
    logp = -INFINITY;
    ham = INFINITY;
  } else {
    logp = ll + prior / 2.;
    kicked = isfinite(logp) ? 1 : 0;
    ham = -logp + 0.5 * (kicked ? k2 : k1);
  }
  st->logp = logp;
  st->kicked = kicked;
  st->hcur = ham;
  if (ham < st->hmin) st->hmin = ham;
  if (ham > st->hmax) st->hmax = ham;
  st->n_grad += 1;
  const int instab = isinf(logp) || (st->hmax - st->hmin) > st->tol;
  if (instab) {
    st->instab = 1;
    st->done = 1;
    st->skip = 1;
  }
}

// partials of p . p (the initial kinetic energy), post_a's slot [2]
static __global__ __launch_bounds__(VEC_BLOCK) void cox_sumsq_kernel(
    int64_t P, const double* __restrict__ p, double* __restrict__ part) {
  double a = 0.;
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK)
    a += p[j] * p[j];
  a = block_sum<VEC_BLOCK>(a);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

static __global__ __launch_bounds__(WAVE) void cox_traj_init_kernel(
    const double* __restrict__ part, double logp0, double tol, CoxTraj* st) {
  const double k = part_sum_wave(part, NPART);
  if (threadIdx.x != 0) return;
  const double ham = -logp0 + 0.5 * k;
  st->logp = logp0;
  st->h0 = st->hmin = st->hmax = st->hcur = ham;
  st->tol = tol;
  st->skip = st->done = st->zero = st->kicked = 0;
  st->n_grad = st->instab = 0;
}

// p = p2 where the last step's second half kick went
static __global__ __launch_bounds__(VEC_BLOCK) void cox_finish_kernel(
    int64_t P, double* __restrict__ p, const double* __restrict__ p2,
    const CoxTraj* st) {
  if (!st->kicked) return;
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK)
    p[j] = p2[j];
}

// ---------------------------------------------------------------- NUTS
// One doubling of nuts.py:230-297: a half-tree of 2^h leapfrog steps in one
// direction, its recursion (nuts.py:238-252) unrolled over the steps
// t = 1 .. 2^h.  After step t the new state is a singleton tree; while
// 2^(l+1) divides t, the pending left tree of height l absorbs the tree of
// height l that has just been completed.  A tree lives where its first leaf
// was stored and grows in place: the tree whose first leaf is step i + 1
// (i even) is in buffer tz(i), the one that starts the half-tree (i = 0) in
// buffer h.  A tree that ends at step t has the current state of the
// integrator as its far end, so a buffer keeps only the near end (q, p) and
// the sample (q, grad) as P-vectors.  The main tree (index NUTS_MAIN) keeps
// both ends.  Once a merged tree meets a termination criterion the flags and
// the min / max Hamiltonian are folded into every pending tree on its left
// (nuts.py:278-282: nothing else is), stop and CoxTraj::skip are raised and
// every later kernel of the doubling but the top-level merge exits at entry.
constexpr int NUTS_MAXH = 10;              // tallest half-tree: 1024 steps
constexpr int NUTS_LEAF = NUTS_MAXH + 1;   // the singleton of an even step
constexpr int NUTS_MAIN = NUTS_MAXH + 2;
constexpr int NUTS_NTREE = NUTS_MAXH + 3;

struct NutsTree {
  double logp;        // of the sample
  double hmin, hmax;
  double err, acc;    // ave_hamiltonian_error, ave_accept_prob
  int n_acc;          // n_acceptable_state
  int u_turn;
  int height;
  int pad;
};

struct NutsState {
  NutsTree tree[NUTS_NTREE];
  double init_joint, thr, tol;
  int stop;           // a tree inside the half-tree terminated
  int rejected;       // the top-level merge did not take the half-tree
  int n_uniform;      // uniforms consumed by this doubling
  int n_step;         // leapfrog steps taken by this doubling
};

// Python's min() / max(): the second argument replaces on a strict compare
__device__ inline double py_min(double a, double b) { return b < a ? b : a; }
__device__ inline double py_max(double a, double b) { return b > a ? b : a; }

__device__ inline bool nuts_terminated(const NutsTree& t, double tol) {
  return t.u_turn || (t.hmax - t.hmin) > tol;
}

__device__ inline void nuts_merge_flags(NutsTree& t, const NutsTree& a) {
  t.u_turn = t.u_turn || a.u_turn;
  t.hmin = py_min(t.hmin, a.hmin);
  t.hmax = py_max(t.hmax, a.hmax);
}

// buffer of the tree whose first leaf has the 0-based index i
__device__ __host__ inline int nuts_buf(int i, int h) {
  return i == 0 ? h : __builtin_ctz((unsigned)i);
}

// The tree in buffer `cur` (first leaf i) terminated: every pending tree on
// its left takes the flags in turn, the nearest first.
__device__ inline void nuts_propagate(NutsState* ns, int cur, int i, int h) {
  while (i > 0) {
    i -= i & -i;
    const int left = nuts_buf(i, h);
    nuts_merge_flags(ns->tree[left], ns->tree[cur]);
    cur = left;
  }
}

// _update_sample (nuts.py:299-313): 'swap' at the top level, else 'uniform'
template <bool TOP>
__device__ inline bool nuts_pick(const NutsTree& t, const NutsTree& a,
                                 double u) {
  double w;
  if (TOP) {
    w = (double)a.n_acc / (double)t.n_acc;
  } else {
    const int n = t.n_acc + a.n_acc;
    w = (double)a.n_acc / (double)(n > 1 ? n : 1);
  }
  return u < w;
}

__device__ inline double nuts_uniform(const NutsState* ns, const double* unif,
                                      int n_unif) {
  const int k = ns->n_uniform;
  return unif[k < n_unif ? k : n_unif - 1];
}

static __global__ void cox_nuts_init_kernel(NutsState* ns, double logp0,
                                     double joint0, double thr, double tol) {
  if (threadIdx.x != 0) return;
  NutsTree& m = ns->tree[NUTS_MAIN];
  m.logp = logp0;
  m.hmin = m.hmax = -joint0;
  m.err = fabs(joint0 - joint0);
  m.acc = py_min(1., exp(joint0 - joint0));
  m.n_acc = joint0 > thr ? 1 : 0;
  m.u_turn = 0;
  m.height = 0;
  ns->init_joint = joint0;
  ns->thr = thr;
  ns->tol = tol;
  ns->stop = ns->rejected = ns->n_uniform = ns->n_step = 0;
}

// The integrator restarts from the main tree's end in the doubling's direction.
static __global__ __launch_bounds__(VEC_BLOCK) void cox_nuts_start_kernel(
    int64_t P, const double* __restrict__ end_q,
    const double* __restrict__ end_p, const double* __restrict__ end_g,
    double* __restrict__ q, double* __restrict__ p, double* __restrict__ g,
    CoxTraj* st, NutsState* ns) {
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK) {
    q[j] = end_q[j];
    p[j] = end_p[j];
    g[j] = end_g[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->skip = st->done = st->zero = st->kicked = 0;
    st->n_grad = st->instab = 0;
    ns->stop = ns->rejected = ns->n_uniform = ns->n_step = 0;
  }
}

// One wave, after post_a: logp and the Hamiltonian as cox_post_b_kernel forms
// them, then the singleton tree of step t (nuts.py:254-262, 197-219) into
// tree[dst].  A singleton never terminates (max H == min H).  Where a
// risk-set sum is 0 there is no gradient to go on with: an even step is
// merged as usual (the merged tree is unstable: max H = inf); after an odd
// step of a taller half-tree the reference cannot take the next step, and the
// half-tree ends here as unstable.
static __global__ __launch_bounds__(WAVE) void cox_nuts_leaf_kernel(
    const double* __restrict__ llpart, const double* __restrict__ part,
    CoxTraj* st, NutsState* ns, int dst, int t, int h) {
  if (ns->stop) return;
  const double ll = part_sum_wave(llpart, SCAN_G);
  const double prior = part_sum_wave(part, NPART);
  const double k2 = part_sum_wave(part + NPART, NPART);
  const double k1 = part_sum_wave(part + 2 * NPART, NPART);
  if (threadIdx.x != 0) return;
  double logp, ham;
  int kicked = 0;
  if (st->zero) {
    logp = -INFINITY;
    ham = INFINITY;
  } else {
    logp = ll + prior / 2.;
    kicked = isfinite(logp) ? 1 : 0;
    ham = -logp + 0.5 * (kicked ? k2 : k1);
  }
  st->logp = logp;
  st->kicked = kicked;
  st->hcur = ham;
  st->n_grad += 1;
  ns->n_step += 1;
  const double joint = isinf(logp) ? -INFINITY : -ham;
  NutsTree& leaf = ns->tree[dst];
  leaf.logp = logp;
  leaf.hmin = leaf.hmax = -joint;
  leaf.err = fabs(ns->init_joint - joint);
  leaf.acc = py_min(1., exp(joint - ns->init_joint));
  leaf.n_acc = joint > ns->thr ? 1 : 0;
  leaf.u_turn = 0;
  leaf.height = 0;
  if (st->zero && (t & 1) && h > 0) {
    nuts_propagate(ns, dst, t - 1, h);
    ns->stop = 1;
    st->skip = 1;
  }
}

// An odd step starts a pending tree: its near end and its sample
static __global__ __launch_bounds__(VEC_BLOCK) void cox_nuts_store_kernel(
    int64_t P, const double* __restrict__ q, const double* __restrict__ p,
    const double* __restrict__ p2, const double* __restrict__ g,
    double* __restrict__ near_q, double* __restrict__ near_p,
    double* __restrict__ samp_q, double* __restrict__ samp_g,
    const CoxTraj* st, const NutsState* ns) {
  if (ns->stop) return;
  const bool kicked = st->kicked;
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK) {
    const double qj = q[j];
    near_q[j] = qj;
    near_p[j] = kicked ? p2[j] : p[j];
    samp_q[j] = qj;
    samp_g[j] = g[j];
  }
}

// The P-vector half of _merge_next_tree (nuts.py:271-297) of tree[absb] into
// tree[pend]: the sample choice (a conditional copy), TOP: the new end state
// of the main tree, and the NPART partials of the two dot products of the
// U-turn test, dot(q_front - q_rear, p_front) and dot(., p_rear).  The far
// end is the integrator's current state.  The scalars are read, not written:
// cox_nuts_merge_b_kernel repeats the decisions and updates them.  (abs_q,
// abs_g alias q, g when a singleton is absorbed: no __restrict__.)
template <bool TOP>
static __global__ __launch_bounds__(VEC_BLOCK) void cox_nuts_merge_a_kernel(
    int64_t P, int dir, int pend, int absb, const double* q, const double* p,
    const double* p2, const double* g, const double* near_q,
    const double* near_p, double* samp_q, double* samp_g, const double* abs_q,
    const double* abs_g, double* end_q, double* end_p, double* end_g,
    const double* unif, int n_unif, double* part, const CoxTraj* st,
    const NutsState* ns) {
  const NutsTree& a = ns->tree[absb];
  if (ns->stop || (TOP && nuts_terminated(a, ns->tol))) return;
  const bool pick =
      nuts_pick<TOP>(ns->tree[pend], a, nuts_uniform(ns, unif, n_unif));
  const bool kicked = st->kicked;
  double a0 = 0., a1 = 0.;
  for (int64_t j = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; j < P;
       j += (int64_t)gridDim.x * VEC_BLOCK) {
    const double qc = q[j], pc = kicked ? p2[j] : p[j];
    if (pick) {
      samp_q[j] = abs_q[j];
      samp_g[j] = abs_g[j];
    }
    if (TOP) {
      end_q[j] = qc;
      end_p[j] = pc;
      end_g[j] = g[j];
    }
    const double nq = near_q[j], np = near_p[j];
    const double dq = dir > 0 ? qc - nq : nq - qc;
    a0 += dq * (dir > 0 ? pc : np);
    a1 += dq * (dir > 0 ? np : pc);
  }
  a0 = block_sum<VEC_BLOCK>(a0);
  a1 = block_sum<VEC_BLOCK>(a1);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = a0;
    part[NPART + blockIdx.x] = a1;
  }
}

// One wave: the scalar half of _merge_next_tree, in the reference's order.
// `first`: the 0-based index of tree[pend]'s first leaf.
template <bool TOP>
static __global__ __launch_bounds__(WAVE) void cox_nuts_merge_b_kernel(
    int pend, int absb, int first, int h, const double* __restrict__ unif,
    int n_unif, const double* __restrict__ part, CoxTraj* st, NutsState* ns) {
  if (!TOP && ns->stop) return;
  const double d0 = part_sum_wave(part, NPART);
  const double d1 = part_sum_wave(part + NPART, NPART);
  if (threadIdx.x != 0) return;
  NutsTree& t = ns->tree[pend];
  const NutsTree a = ns->tree[absb];
  const bool term = ns->stop || nuts_terminated(a, ns->tol);
  const bool pick = nuts_pick<TOP>(t, a, nuts_uniform(ns, unif, n_unif));
  nuts_merge_flags(t, a);
  if (term) {
    ns->rejected = 1;
    return;
  }
  if (pick) t.logp = a.logp;
  ns->n_uniform += 1;
  t.n_acc += a.n_acc;
  if (d0 < 0. || d1 < 0.) t.u_turn = 1;
  const double nt = ldexp(1., t.height), na = ldexp(1., a.height);
  const double w = nt / (nt + na);
  t.err = w * t.err + (1 - w) * a.err;
  t.acc = w * t.acc + (1 - w) * a.acc;
  t.height += 1;
  if (!TOP && nuts_terminated(t, ns->tol)) {
    nuts_propagate(ns, pend, first, h);
    ns->stop = 1;
    st->skip = 1;
  }
}
// ---------------------------------------------------------------- host side
// What the trajectory, the tree and the C ABI front need from a likelihood
// handle; every handle derives from it -- the Cox ones through CoxCore, the
// row-wise GLM ones through GlmRowsCore, bbx_cpoisson directly (the design is
// borrowed: it must outlive them).
struct HamCore {
  bbx_design* h = nullptr;
  int device = 0;
  int64_t n = 0, P = 0;
  DevMem eta, tmp;                       // n: X~ beta (or X~ v), w
  DevMem llpart, post;                   // SCAN_G, 3 NPART
  DevMem q, p, p2, g, gl, v, scale, pp;  // P
  DevMem st;                             // CoxTraj
  CoxTraj* host_st = nullptr;            // pinned read-back
  bool have_location = false;
  // NUTS, allocated by the first nuts_begin
  DevMem nuts_vec;                       // (4 (NUTS_MAXH + 1) + 8) P-vectors
  DevMem nuts_st, nuts_u;                // NutsState, 2^NUTS_MAXH uniforms
  NutsState* host_nuts = nullptr;        // pinned read-back
  bool nuts_begun = false;
  // between nuts_begin and nuts_sample: the tree's draw is under way, and the
  // calls that would reuse its scratch (cox_family.hpp's prediction) refuse.
  // Only nuts_sample (valid at any time after nuts_begin) and the next
  // nuts_begin change it: that is how an abandoned tree is closed.
  bool nuts_open = false;
  // P-vector k of tree buffer b: 0 near q, 1 near p, 2 sample q, 3 sample grad
  double* nuts_tree_vec(int b, int k) const {
    return nuts_vec.as<double>() + (size_t)(4 * b + k) * P;
  }
  // main tree: 0-2 front q, p, grad; 3-5 rear q, p, grad; 6, 7 sample q, grad
  double* nuts_main_vec(int k) const {
    return nuts_vec.as<double>() + (size_t)(4 * (NUTS_MAXH + 1) + k) * P;
  }
};

namespace ham {

inline CoxTraj* cst(const HamCore* c) { return c->st.as<CoxTraj>(); }
inline NutsState* nst(const HamCore* c) { return c->nuts_st.as<NutsState>(); }

// While it lives the design's product kernels exit at entry once
// CoxTraj::skip is set.
struct SkipScope {
  bbx_design* h;
  SkipScope(bbx_design* h_, const int* flag) : h(h_) { h->skip_flag = flag; }
  ~SkipScope() { h->skip_flag = nullptr; }
  SkipScope(const SkipScope&) = delete;
  SkipScope& operator=(const SkipScope&) = delete;
};

inline int read_state(HamCore* c) {
  BBX_HIP(hipMemcpyAsync(c->host_st, c->st.ptr, sizeof(CoxTraj),
                         hipMemcpyDeviceToHost, c->h->stream));
  BBX_HIP(hipStreamSynchronize(c->h->stream));
  return BBX_OK;
}

// eta = X~ d_beta (d_beta: a P-vector on the device)
inline int eta_of(HamCore* c, const double* d_beta) {
  bbx_design* h = c->h;
  BBX_TRY(launch_prep_v(h, d_beta, nullptr, nullptr, part_slot(h, PS_C)));
  return launch_dot(h, d_beta, nullptr, c->eta.as<double>(), nullptr);
}

// Host-pointer wrapper: P-vector in (stage), P-vector out
template <class F>
int with_p_stage(HamCore* c, const double* in, double* out, F&& f) {
  bbx_design* h = c->h;
  double* d_in = h->stage_P.as<double>();
  double* d_out = c->gl.as<double>();
  BBX_HIP(hipMemcpyAsync(d_in, in, sizeof(double) * c->P,
                         hipMemcpyHostToDevice, h->stream));
  BBX_TRY(f(d_in, out ? d_out : nullptr));
  if (out)
    BBX_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * c->P,
                           hipMemcpyDeviceToHost, h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));
  return BBX_OK;
}

// The leapfrog step of both trajectories up to post_a: step1, X~ v, the
// family's likelihood block lik(grad_loglik) -- eta is complete in c->eta in
// stream order; it leaves X~^T w in its argument and the log-likelihood
// partials in c->llpart -- and post_a.
template <class Lik>
int launch_leapfrog(HamCore* c, double half_dt, double dt, Lik& lik) {
  bbx_design* h = c->h;
  CoxTraj* st = cst(c);
  BBX_LAUNCH(cox_step1_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->P, h->intercept, half_dt, dt, c->q.as<double>(),
             c->p.as<double>(), c->p2.as<const double>(),
             c->g.as<const double>(), c->scale.as<const double>(),
             h->offset.as<const double>(), c->v.as<double>(),
             part_slot(h, PS_C), st);
  BBX_HIP(hipGetLastError());
  BBX_TRY(launch_dot(h, c->v.as<double>(), nullptr, c->eta.as<double>(),
                     nullptr));
  BBX_TRY(lik(c->gl.as<double>()));
  BBX_LAUNCH(cox_post_a_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->P, half_dt, c->q.as<const double>(), c->p.as<const double>(),
             c->p2.as<double>(), c->g.as<double>(), c->gl.as<const double>(),
             c->scale.as<const double>(), c->pp.as<const double>(),
             c->post.as<double>(), st);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <class Lik>
int trajectory_impl(HamCore* c, Lik& lik, double dt, int n_step,
                    const double* scale, const double* prior_prec,
                    const double* q0, const double* p0, double logp0,
                    const double* grad0, double tol, double* q, double* p,
                    double* logp, double* grad, int* n_grad_evals,
                    int* instability, double* hamiltonian) {
  bbx_design* h = c->h;
  const size_t bytes = sizeof(double) * c->P;
  const hipMemcpyKind H2D = hipMemcpyHostToDevice, D2H = hipMemcpyDeviceToHost;
  BBX_HIP(hipMemcpyAsync(c->scale.ptr, scale, bytes, H2D, h->stream));
  BBX_HIP(hipMemcpyAsync(c->pp.ptr, prior_prec, bytes, H2D, h->stream));
  BBX_HIP(hipMemcpyAsync(c->q.ptr, q0, bytes, H2D, h->stream));
  BBX_HIP(hipMemcpyAsync(c->p.ptr, p0, bytes, H2D, h->stream));
  BBX_HIP(hipMemcpyAsync(c->g.ptr, grad0, bytes, H2D, h->stream));
  CoxTraj* st = cst(c);
  BBX_LAUNCH(cox_sumsq_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->P, c->p.as<const double>(), c->post.as<double>());
  BBX_HIP(hipGetLastError());
  BBX_LAUNCH(cox_traj_init_kernel, dim3(1), dim3(WAVE), 0, h->stream,
             c->post.as<const double>(), logp0, tol, st);
  BBX_HIP(hipGetLastError());
  // from here on the design's product kernels exit at entry once the rule fired
  SkipScope skip_scope(h, &st->skip);
  const double half_dt = 0.5 * dt;
  for (int i = 0; i < n_step; ++i) {
    BBX_TRY(launch_leapfrog(c, half_dt, dt, lik));
    BBX_LAUNCH(cox_post_b_kernel, dim3(1), dim3(WAVE), 0, h->stream,
               c->llpart.as<const double>(), c->post.as<const double>(), st);
    BBX_HIP(hipGetLastError());
  }
  BBX_LAUNCH(cox_finish_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->P, c->p.as<double>(), c->p2.as<const double>(), st);
  BBX_HIP(hipGetLastError());
  if (q) BBX_HIP(hipMemcpyAsync(q, c->q.ptr, bytes, D2H, h->stream));
  if (p) BBX_HIP(hipMemcpyAsync(p, c->p.ptr, bytes, D2H, h->stream));
  if (grad) BBX_HIP(hipMemcpyAsync(grad, c->g.ptr, bytes, D2H, h->stream));
  BBX_TRY(read_state(c));   // the one synchronisation of the trajectory
  const CoxTraj& hs = *c->host_st;
  if (logp) *logp = hs.logp;
  if (n_grad_evals) *n_grad_evals = hs.n_grad;
  if (instability) *instability = hs.instab;
  if (hamiltonian) {
    hamiltonian[0] = hs.h0;
    hamiltonian[1] = hs.hcur;
  }
  return BBX_OK;
}

inline int nuts_begin_impl(HamCore* c, const double* scale,
                           const double* prior_prec, const double* q0,
                           const double* p0, double logp0, const double* grad0,
                           double joint0, double thr, double tol) {
  bbx_design* h = c->h;
  const size_t bytes = sizeof(double) * c->P;
  c->nuts_begun = false;
  c->nuts_open = false;
  if (!c->nuts_vec.ptr) {
    BBX_TRY(c->nuts_vec.alloc(bytes * (4 * (NUTS_MAXH + 1) + 8)));
    BBX_TRY(c->nuts_st.alloc(sizeof(NutsState)));
    BBX_TRY(c->nuts_u.alloc(sizeof(double) << NUTS_MAXH));
    BBX_HIP(hipHostMalloc((void**)&c->host_nuts, sizeof(NutsState)));
  }
  const hipMemcpyKind H2D = hipMemcpyHostToDevice, D2D = hipMemcpyDeviceToDevice;
  BBX_HIP(hipMemcpyAsync(c->scale.ptr, scale, bytes, H2D, h->stream));
  BBX_HIP(hipMemcpyAsync(c->pp.ptr, prior_prec, bytes, H2D, h->stream));
  const double* src[3] = {q0, p0, grad0};
  for (int k = 0; k < 3; ++k) {
    BBX_HIP(hipMemcpyAsync(c->nuts_main_vec(k), src[k], bytes, H2D, h->stream));
    BBX_HIP(hipMemcpyAsync(c->nuts_main_vec(3 + k), c->nuts_main_vec(k), bytes,
                           D2D, h->stream));
  }
  BBX_HIP(hipMemcpyAsync(c->nuts_main_vec(6), c->nuts_main_vec(0), bytes, D2D,
                         h->stream));
  BBX_HIP(hipMemcpyAsync(c->nuts_main_vec(7), c->nuts_main_vec(2), bytes, D2D,
                         h->stream));
  BBX_HIP(hipMemsetAsync(c->nuts_st.ptr, 0, sizeof(NutsState), h->stream));
  BBX_LAUNCH(cox_nuts_init_kernel, dim3(1), dim3(WAVE), 0, h->stream, nst(c),
             logp0, joint0, thr, tol);
  BBX_HIP(hipGetLastError());
  BBX_HIP(hipStreamSynchronize(h->stream));   // the host arrays are free again
  c->nuts_begun = true;
  c->nuts_open = true;
  return BBX_OK;
}

template <bool TOP>
int launch_nuts_merge(HamCore* c, int dir, int pend, int absb, int first,
                      int height, int n_unif) {
  bbx_design* h = c->h;
  CoxTraj* st = cst(c);
  NutsState* ns = nst(c);
  const double *near_q, *near_p, *abs_q, *abs_g;
  double *samp_q, *samp_g, *end_q = nullptr, *end_p = nullptr, *end_g = nullptr;
  if (TOP) {
    const int far = dir > 0 ? 0 : 3, near = dir > 0 ? 3 : 0;
    near_q = c->nuts_main_vec(near);
    near_p = c->nuts_main_vec(near + 1);
    end_q = c->nuts_main_vec(far);
    end_p = c->nuts_main_vec(far + 1);
    end_g = c->nuts_main_vec(far + 2);
    samp_q = c->nuts_main_vec(6);
    samp_g = c->nuts_main_vec(7);
  } else {
    near_q = c->nuts_tree_vec(pend, 0);
    near_p = c->nuts_tree_vec(pend, 1);
    samp_q = c->nuts_tree_vec(pend, 2);
    samp_g = c->nuts_tree_vec(pend, 3);
  }
  if (absb == NUTS_LEAF) {       // a singleton: its sample is the current state
    abs_q = c->q.as<const double>();
    abs_g = c->g.as<const double>();
  } else {
    abs_q = c->nuts_tree_vec(absb, 2);
    abs_g = c->nuts_tree_vec(absb, 3);
  }
  BBX_LAUNCH(cox_nuts_merge_a_kernel<TOP>, dim3(NPART), dim3(VEC_BLOCK), 0,
             h->stream, c->P, dir, pend, absb, c->q.as<const double>(),
             c->p.as<const double>(), c->p2.as<const double>(),
             c->g.as<const double>(), near_q, near_p, samp_q, samp_g, abs_q,
             abs_g, end_q, end_p, end_g, c->nuts_u.as<const double>(), n_unif,
             c->post.as<double>(), st, ns);
  BBX_HIP(hipGetLastError());
  BBX_LAUNCH(cox_nuts_merge_b_kernel<TOP>, dim3(1), dim3(WAVE), 0, h->stream,
             pend, absb, first, height, c->nuts_u.as<const double>(), n_unif,
             c->post.as<const double>(), st, ns);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// One doubling: everything enqueued at once, one synchronisation at the end.
template <class Lik>
int nuts_doubling_impl(HamCore* c, Lik& lik, double dt, int dir, int height,
                       const double* uniforms) {
  bbx_design* h = c->h;
  CoxTraj* st = cst(c);
  NutsState* ns = nst(c);
  const int n_leaf = 1 << height;
  BBX_HIP(hipMemcpyAsync(c->nuts_u.ptr, uniforms, sizeof(double) * n_leaf,
                         hipMemcpyHostToDevice, h->stream));
  const int far = dir > 0 ? 0 : 3;
  BBX_LAUNCH(cox_nuts_start_kernel, dim3(NPART), dim3(VEC_BLOCK), 0, h->stream,
             c->P, c->nuts_main_vec(far), c->nuts_main_vec(far + 1),
             c->nuts_main_vec(far + 2), c->q.as<double>(), c->p.as<double>(),
             c->g.as<double>(), st, ns);
  BBX_HIP(hipGetLastError());
  SkipScope skip_scope(h, &st->skip);
  const double sdt = dir * dt, half_dt = 0.5 * sdt;
  for (int t = 1; t <= n_leaf; ++t) {
    BBX_TRY(launch_leapfrog(c, half_dt, sdt, lik));
    const bool odd = t & 1;
    const int dst = odd ? nuts_buf(t - 1, height) : NUTS_LEAF;
    BBX_LAUNCH(cox_nuts_leaf_kernel, dim3(1), dim3(WAVE), 0, h->stream,
               c->llpart.as<const double>(), c->post.as<const double>(), st,
               ns, dst, t, height);
    BBX_HIP(hipGetLastError());
    if (odd) {
      BBX_LAUNCH(cox_nuts_store_kernel, dim3(NPART), dim3(VEC_BLOCK), 0,
                 h->stream, c->P, c->q.as<const double>(),
                 c->p.as<const double>(), c->p2.as<const double>(),
                 c->g.as<const double>(), c->nuts_tree_vec(dst, 0),
                 c->nuts_tree_vec(dst, 1), c->nuts_tree_vec(dst, 2),
                 c->nuts_tree_vec(dst, 3), st, ns);
      BBX_HIP(hipGetLastError());
      continue;
    }
    // the merges that are due: the trailing zeros of t
    for (int l = 0; l < height && t % (2 << l) == 0; ++l) {
      const int first = t - (2 << l);
      BBX_TRY(launch_nuts_merge<false>(c, dir, nuts_buf(first, height),
                                       l == 0 ? NUTS_LEAF : l, first, height,
                                       n_leaf));
    }
  }
  // double_trajectory's merge into the main tree (sampling_method='swap')
  BBX_TRY(launch_nuts_merge<true>(c, dir, NUTS_MAIN, height, 0, height,
                                  n_leaf));
  BBX_HIP(hipMemcpyAsync(c->host_nuts, c->nuts_st.ptr, sizeof(NutsState),
                         hipMemcpyDeviceToHost, h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));
  return BBX_OK;
}

// ------------------------------------------------------------ the C ABI front
// Everything of a handle's C entry points that does not depend on the family:
// the checks, the HamCore part of `create`, `destroy` and one template per
// shared entry point.  A family states a policy F:
//   F::name                          "cox", "logit", ...: bbx_<name>_* and the
//                                    messages
//   F::Lik                           its likelihood block, built as Lik{c}
//   F::locate(c, d_in)               set_location between the upload of beta
//                                    (in d_in) and have_location = true; the
//                                    host's beta is free when it returns
//   F::hessian_from_v(c, d_v, d_out) the Hessian matvec at the location
// and stamps its ten entry points with BBX_HAM_ENTRY_POINTS.
inline int check(const HamCore* c, const char* family) {
  if (!c)
    return fail(BBX_ERR_INVALID, std::string("NULL ") + family + " handle");
  if (!design_alive(c->h))
    return fail(BBX_ERR_STATE, std::string("the ") + family +
                                   " handle's design has been destroyed");
  return BBX_OK;
}

// bbx_<family>_<entry> has to succeed before the call that was made
inline int not_yet(const char* family, const char* entry) {
  return fail(BBX_ERR_STATE, std::string("bbx_") + family + "_" + entry +
                                 " has not succeeded");
}

inline int nuts_doubling_args(const HamCore* c, const char* family,
                              const double* uniforms, int direction,
                              int height) {
  if (!c->nuts_begun) return not_yet(family, "nuts_begin");
  if (!uniforms) return fail(BBX_ERR_INVALID, "NULL argument");
  if (direction != 1 && direction != -1)
    return fail(BBX_ERR_INVALID, "direction must be 1 or -1");
  if (height < 0 || height > NUTS_MAXH)
    return fail(BBX_ERR_INVALID, "height outside [0, " +
                                     std::to_string(NUTS_MAXH) + "]");
  return BBX_OK;
}

inline void nuts_doubling_out(const HamCore* c, int* n_uniform_used,
                              int* n_steps, int* flags, int* tree,
                              double* averages) {
  const NutsState& hs = *c->host_nuts;
  const NutsTree& m = hs.tree[NUTS_MAIN];
  if (n_uniform_used) *n_uniform_used = hs.n_uniform;
  if (n_steps) *n_steps = hs.n_step;
  if (flags) {
    flags[0] = m.u_turn;
    flags[1] = (m.hmax - m.hmin) > hs.tol;
    flags[2] = hs.rejected;
  }
  if (tree) {
    tree[0] = m.height;
    tree[1] = m.n_acc;
  }
  if (averages) {
    averages[0] = m.err;
    averages[1] = m.acc;
  }
}

inline int nuts_sample_impl(HamCore* c, double* q, double* logp,
                            double* grad) {
  bbx_design* h = c->h;
  const size_t bytes = sizeof(double) * c->P;
  if (q)
    BBX_HIP(hipMemcpyAsync(q, c->nuts_main_vec(6), bytes,
                           hipMemcpyDeviceToHost, h->stream));
  if (grad)
    BBX_HIP(hipMemcpyAsync(grad, c->nuts_main_vec(7), bytes,
                           hipMemcpyDeviceToHost, h->stream));
  BBX_HIP(hipMemcpyAsync(c->host_nuts, c->nuts_st.ptr, sizeof(NutsState),
                         hipMemcpyDeviceToHost, h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));
  if (logp) *logp = c->host_nuts->tree[NUTS_MAIN].logp;
  c->nuts_open = false;
  return BBX_OK;
}

inline void free_pinned(HamCore* c) {
  if (c->host_st) (void)hipHostFree(c->host_st);
  if (c->host_nuts) (void)hipHostFree(c->host_nuts);
  c->host_st = nullptr;
  c->host_nuts = nullptr;
}

// The HamCore part of a family's `create`, on a fresh handle: every buffer
// HamCore declares but the NUTS ones, the pinned read-back and the device
// state zeroed (queued on the design's stream: the family synchronises once,
// after its own uploads).  After a failure the caller discards the handle.
// (static, as the kernels are: a handle type's name in an exported symbol
// would read as part of the C ABI.)
static int init_core(HamCore* c, bbx_design* h, const char* family) {
  c->h = h;
  c->device = h->device;
  c->n = h->n;
  c->P = h->P;
  if (hipSetDevice(h->device) != hipSuccess)
    return fail(BBX_ERR_HIP, "hipSetDevice");
  const size_t d8 = sizeof(double);
  BBX_TRY(c->eta.alloc(d8 * c->n));
  BBX_TRY(c->tmp.alloc(d8 * c->n));
  DevMem* pvec[] = {&c->q, &c->p, &c->p2, &c->g, &c->gl, &c->v, &c->scale, &c->pp};
  for (DevMem* m : pvec) BBX_TRY(m->alloc(d8 * c->P));
  BBX_TRY(c->llpart.alloc(d8 * SCAN_G));
  BBX_TRY(c->post.alloc(d8 * 3 * NPART));
  BBX_TRY(c->st.alloc(sizeof(CoxTraj)));
  if (hipHostMalloc((void**)&c->host_st, sizeof(CoxTraj)) != hipSuccess) {
    c->host_st = nullptr;
    return fail(BBX_ERR_HIP, "hipHostMalloc");
  }
  const hipError_t e = hipMemsetAsync(c->st.ptr, 0, sizeof(CoxTraj), h->stream);
  if (e != hipSuccess)
    return fail(BBX_ERR_HIP, std::string(family) + " upload: " +
                                 hipGetErrorString(e));
  return BBX_OK;
}

// Frees a handle and passes `st` on: the end of a `create` that failed
template <class H>
static int discard(H* c, int st) {
  free_pinned(c);
  delete c;
  return st;
}

template <class H>
static int destroy(H* c) {
  if (!c) return BBX_OK;
  if (design_alive(c->h)) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->h->stream);
  }
  return discard(c, BBX_OK);
}

// loglik (and, d_grad != null, its gradient) at a P-vector on the device
template <class Lik>
int loglik_grad_impl(HamCore* c, Lik& lik, const double* d_beta,
                     double* loglik, double* d_grad) {
  bbx_design* h = c->h;
  // a trajectory that stopped early leaves its skip flag set
  BBX_LAUNCH(cox_reset_kernel, dim3(1), dim3(WAVE), 0, h->stream, cst(c));
  BBX_HIP(hipGetLastError());
  BBX_TRY(eta_of(c, d_beta));
  BBX_TRY(lik(d_grad));
  BBX_LAUNCH(cox_loglik_kernel, dim3(1), dim3(WAVE), 0, h->stream,
             c->llpart.as<const double>(), cst(c));
  BBX_HIP(hipGetLastError());
  BBX_TRY(read_state(c));
  *loglik = c->host_st->logp;
  return BBX_OK;
}

template <class F, class H>
int hessian_impl(H* c, const double* d_v, double* d_out) {
  if (!c->have_location) return not_yet(F::name, "set_location");
  return F::hessian_from_v(c, d_v, d_out);
}

template <class F, class H>
int loglik_grad_dev(H* c, const double* d_beta, double* loglik,
                    double* d_grad) {
  BBX_TRY(check(c, F::name));
  if (!d_beta || !loglik) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    typename F::Lik lik{c};
    return loglik_grad_impl(c, lik, d_beta, loglik, d_grad);
  });
}

template <class F, class H>
int loglik_grad(H* c, const double* beta, double* loglik, double* grad) {
  BBX_TRY(check(c, F::name));
  if (!beta || !loglik) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    typename F::Lik lik{c};
    double ll = 0.;
    BBX_TRY(with_p_stage(c, beta, grad, [&](const double* d_in, double* d_out) {
      return loglik_grad_impl(c, lik, d_in, &ll, d_out);
    }));
    *loglik = ll;
    return BBX_OK;
  });
}

template <class F, class H>
int set_location(H* c, const double* beta) {
  BBX_TRY(check(c, F::name));
  if (!beta) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    bbx_design* h = c->h;
    c->have_location = false;
    double* d_in = h->stage_P.as<double>();
    BBX_HIP(hipMemcpyAsync(d_in, beta, sizeof(double) * c->P,
                           hipMemcpyHostToDevice, h->stream));
    BBX_TRY(F::locate(c, d_in));
    c->have_location = true;
    return BBX_OK;
  });
}

template <class F, class H>
int hessian_matvec_dev(H* c, const double* d_v, double* d_out) {
  BBX_TRY(check(c, F::name));
  if (!d_v || !d_out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return hessian_impl<F>(c, d_v, d_out); });
}

template <class F, class H>
int hessian_matvec(H* c, const double* v, double* out) {
  BBX_TRY(check(c, F::name));
  if (!v || !out) return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return with_p_stage(c, v, out, [&](const double* d_in, double* d_out) {
      return hessian_impl<F>(c, d_in, d_out);
    });
  });
}

template <class F, class H>
int hmc_trajectory(H* c, double dt, int n_step, const double* precond_scale,
                   const double* prior_prec, const double* q0,
                   const double* p0, double logp0, const double* grad0,
                   double hamiltonian_tol, double* q, double* p, double* logp,
                   double* grad, int* n_grad_evals, int* instability,
                   double* hamiltonian) {
  BBX_TRY(check(c, F::name));
  if (!precond_scale || !prior_prec || !q0 || !p0 || !grad0)
    return fail(BBX_ERR_INVALID, "NULL argument");
  if (n_step < 0) return fail(BBX_ERR_INVALID, "n_step < 0");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    typename F::Lik lik{c};
    return trajectory_impl(c, lik, dt, n_step, precond_scale, prior_prec, q0,
                           p0, logp0, grad0, hamiltonian_tol, q, p, logp, grad,
                           n_grad_evals, instability, hamiltonian);
  });
}

template <class F, class H>
int nuts_begin(H* c, const double* precond_scale, const double* prior_prec,
               const double* q0, const double* p0, double logp0,
               const double* grad0, double joint_logp0,
               double joint_logp_threshold, double hamiltonian_tol) {
  BBX_TRY(check(c, F::name));
  if (!precond_scale || !prior_prec || !q0 || !p0 || !grad0)
    return fail(BBX_ERR_INVALID, "NULL argument");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    return nuts_begin_impl(c, precond_scale, prior_prec, q0, p0, logp0, grad0,
                           joint_logp0, joint_logp_threshold, hamiltonian_tol);
  });
}

template <class F, class H>
int nuts_doubling(H* c, double dt, int direction, int height,
                  const double* uniforms, int* n_uniform_used, int* n_steps,
                  int* flags, int* tree, double* averages) {
  BBX_TRY(check(c, F::name));
  BBX_TRY(nuts_doubling_args(c, F::name, uniforms, direction, height));
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] {
    typename F::Lik lik{c};
    BBX_TRY(nuts_doubling_impl(c, lik, dt, direction, height, uniforms));
    nuts_doubling_out(c, n_uniform_used, n_steps, flags, tree, averages);
    return BBX_OK;
  });
}

template <class F, class H>
int nuts_sample(H* c, double* q, double* logp, double* grad) {
  BBX_TRY(check(c, F::name));
  if (!c->nuts_begun) return not_yet(F::name, "nuts_begin");
  BBX_HIP(hipSetDevice(c->device));
  return no_throw([&] { return nuts_sample_impl(c, q, logp, grad); });
}

}  // namespace ham
}  // namespace bbx

// The ten entry points that include/bbx.h declares for every family, on the
// handle type bbx_<fam> under the policy F: one forwarding line each.
#define BBX_HAM_ENTRY_POINTS(fam, F)                                           \
  extern "C" {                                                                 \
  int bbx_##fam##_destroy(bbx_##fam* c) { return ::bbx::ham::destroy(c); }     \
  int bbx_##fam##_loglik_grad_dev(bbx_##fam* c, const double* d_beta,          \
                                  double* loglik, double* d_grad) {            \
    return ::bbx::ham::loglik_grad_dev<F>(c, d_beta, loglik, d_grad);          \
  }                                                                            \
  int bbx_##fam##_loglik_grad(bbx_##fam* c, const double* beta,                \
                              double* loglik, double* grad) {                  \
    return ::bbx::ham::loglik_grad<F>(c, beta, loglik, grad);                  \
  }                                                                            \
  int bbx_##fam##_set_location(bbx_##fam* c, const double* beta) {             \
    return ::bbx::ham::set_location<F>(c, beta);                               \
  }                                                                            \
  int bbx_##fam##_hessian_matvec_dev(bbx_##fam* c, const double* d_v,          \
                                     double* d_out) {                          \
    return ::bbx::ham::hessian_matvec_dev<F>(c, d_v, d_out);                   \
  }                                                                            \
  int bbx_##fam##_hessian_matvec(bbx_##fam* c, const double* v,                \
                                 double* out) {                                \
    return ::bbx::ham::hessian_matvec<F>(c, v, out);                           \
  }                                                                            \
  int bbx_##fam##_hmc_trajectory(                                              \
      bbx_##fam* c, double dt, int n_step, const double* precond_scale,        \
      const double* prior_prec, const double* q0, const double* p0,            \
      double logp0, const double* grad0, double hamiltonian_tol, double* q,    \
      double* p, double* logp, double* grad, int* n_grad_evals,                \
      int* instability, double* hamiltonian) {                                 \
    return ::bbx::ham::hmc_trajectory<F>(                                      \
        c, dt, n_step, precond_scale, prior_prec, q0, p0, logp0, grad0,        \
        hamiltonian_tol, q, p, logp, grad, n_grad_evals, instability,          \
        hamiltonian);                                                          \
  }                                                                            \
  int bbx_##fam##_nuts_begin(bbx_##fam* c, const double* precond_scale,        \
                             const double* prior_prec, const double* q0,       \
                             const double* p0, double logp0,                   \
                             const double* grad0, double joint_logp0,          \
                             double joint_logp_threshold,                      \
                             double hamiltonian_tol) {                         \
    return ::bbx::ham::nuts_begin<F>(c, precond_scale, prior_prec, q0, p0,     \
                                     logp0, grad0, joint_logp0,                \
                                     joint_logp_threshold, hamiltonian_tol);   \
  }                                                                            \
  int bbx_##fam##_nuts_doubling(bbx_##fam* c, double dt, int direction,        \
                                int height, const double* uniforms,            \
                                int* n_uniform_used, int* n_steps, int* flags, \
                                int* tree, double* averages) {                 \
    return ::bbx::ham::nuts_doubling<F>(c, dt, direction, height, uniforms,    \
                                        n_uniform_used, n_steps, flags, tree,  \
                                        averages);                             \
  }                                                                            \
  int bbx_##fam##_nuts_sample(bbx_##fam* c, double* q, double* logp,           \
                              double* grad) {                                  \
    return ::bbx::ham::nuts_sample<F>(c, q, logp, grad);                       \
  }                                                                            \
  }
