// Device-resident Gibbs chain: the handle and the three phases of one
// iteration (bayesbridge.py:210-240), shared by chain.hip (one chain per pass
// over the matrix) and batch.hip (K chains per pass).
#pragma once
#include <cmath>

#include "common.hpp"

namespace bbx {

constexpr int ROW_GRID = 2048;  // blocks of the n-length sampler kernels

// Two 128-byte halves: after the coefficient draw the Omega update and the
// tau / lambda updates run as two branches on two streams (chain_step), each
// writing only its own half, so that no cache line is dirty in two L2s.
struct alignas(128) ChainScalars {
  // ---- written by the tau / lambda branch
  double gscale;         // tau, raw parametrisation
  double logprior;       // log posterior minus the log-likelihood
  double abs_pow_sum;    // sum |beta_j|^alpha over shrunk coordinates
  long long n_gscale_clamped;
  long long n_lscale_fixed;
  // ---- written by the Omega branch
  alignas(128) double obs_prec;  // linear model; Student-t, censored,
                                 // quantile: tau
  double loglik;                 // of the current coef
  // log posterior (bayesbridge.py:480-511)
  __host__ __device__ double logp() const { return loglik + logprior; }
};

}  // namespace bbx

struct bbx_chain {
  bbx_design* h = nullptr;
  int model = BBX_MODEL_LOGIT;
  int n_unshrunk = 0;
  double bridge_exp = .5, slab = INFINITY, shape0 = 0., rate0 = 0.;
  uint64_t seed = 0;
  int64_t iter = 0;        // iterations done (Philox key)
  int64_t n_averaged = 0;  // summariser count
  bool mean_zero = true;   // running mean still all zeros => CG warm start 0
  int gscale_update = BBX_GSCALE_SAMPLE;
  int coef_sampler = BBX_SAMPLER_CG;   // bbx_chain_set_coef_sampler
  // BBX_MODEL_STUDENT_T: the degrees of freedom nu (bbx_chain_set_df) and the
  // log-likelihood's per-row constant lgamma((nu+1)/2) - lgamma(nu/2) -
  // 1/2 log(nu/2), computed on the host when nu is set
  double df = 4., df_const = 0.;
  // BBX_MODEL_QUANTILE: the level q (bbx_chain_set_quantile); df_const then
  // holds its row constant log(q (1 - q))
  double quantile = .5;
  // bbx_chain_set_progress: called from the host loop of a run every
  // `progress_every` iterations (gibbs_util.py:214-238 prints from there)
  void (*progress)(int, void*) = nullptr;
  void* progress_ctx = nullptr;
  int progress_every = 0;
  bbx::DevMem outcome, n_trial, kappa;  // n
  bbx::DevMem zbase;                    // P: X~^T kappa (logit) or X~^T y
  bbx::DevMem coef, phi, x0, sd, z, mean, square, sd_unshrunk;  // P-length
  bbx::DevMem lscale;                   // P - n_unshrunk
  bbx::DevMem obs_prec, psi;            // n
  bbx::DevMem latent;                   // n: the probit and censored models' z,
                                        // the Student-t model's omega, the
                                        // quantile model's w (else empty)
  bbx::DevMem status;                   // n bytes: the censored model's row status
                                        // (outcome holds the bounds; else empty)
  bbx::DevMem scalars;                 // ChainScalars
  bbx::DevMem row_part;                 // ROW_GRID partials x 2
  bbx::DevMem misc_part;                // NPART x 3: sums over the coefficients (tau branch)
  // The normals of the NEXT draw (cg_sampler.py:61-62), filled on the design's
  // stream while the Polya-Gamma and lambda kernels run: Philox values depend on
  // (seed, iteration, element) only, so WHEN they are generated changes no bit.
  // eta_iter = the iteration these buffers hold (-1: none).
  bbx::DevMem eta1_next, eta2_next;     // n, P
  long long eta_iter = -1;
  bbx::DevMem samp_gscale, samp_logp;   // per kept sample (device)
  // deferred bookkeeping of a kept iteration: its scalars are stored by the
  // next chain_prior_kernel (pending_store = sample index, -1: none); its
  // coefficients by the CG loop's finish kernel when the run loop announced the
  // slot beforehand (coef_sample, else chain_save_sample copies)
  int pending_store = -1;
  double* coef_sample = nullptr;
  void* pinned = nullptr;
  // second stream for the tau / lambda branch of an iteration
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_join = nullptr;
};

namespace bbx {

// Philox key of the CG draw's normals at 0-based iteration `it`.
inline uint64_t cg_draw_seed(const bbx_chain* c, uint64_t it) {
  return c->seed + 0x9E3779B97F4A7C15ull * (it + 1);
}

// beta | Omega, tau, lambda, part 1 (bayesbridge.py:372-395): phi, the CG warm
// start, the preconditioner sd and z of this iteration, on the design's stream.
int chain_pre_draw(bbx_chain* c);
// Everything after the coefficient draw: Omega | beta (the linear predictor
// psi = X~ beta unless `have_psi`: a batch computes it for all its chains in
// one pass), running summaries, tau | beta, lambda | tau, beta, log posterior.
// In three phases, so that a batch can start the tau / lambda branch of EVERY
// chain (each on the chain's own second stream, with the chain's own partial
// slots) before the first Omega update occupies the design's stream:
// POST_BRANCH launches the branch, POST_MAIN the Omega update on the design's
// stream, POST_JOIN makes the design's stream wait for the branch and advances
// c->iter.  One chain on its own: POST_ALL.  `branch_of`: the chain whose second
// stream carries this chain's branch (a wide batch folds its chains' branches
// onto a few streams); nullptr = the chain's own.
enum { POST_BRANCH = 1, POST_MAIN = 2, POST_JOIN = 4, POST_ALL = 7 };
int chain_post_draw(bbx_chain* c, bool have_psi, int phases,
                    bbx_chain* branch_of = nullptr);
// Sample bookkeeping of a run (gibbs_util.py:126-174): per-sample scalars are
// collected on the device and copied out once at the end.
int chain_begin_run(bbx_chain* c, int n_sample);
int chain_save_sample(bbx_chain* c, int idx, double* d_coef, double* d_lscale,
                      double* d_obs_prec);
int chain_end_run(bbx_chain* c, int n_sample, double* gscale, double* logp);

// The `count` (<= ROW_GRID) block sums of an n-vector w folded onto the NPART
// slots of the design's PS_SUMW that launch_tdot(w) re-adds: slot t takes
// blocks t, t + NPART, ... in that order (chain.hip).
int launch_sumw_fold(bbx_design* h, const double* block_sums, int count);

// The row update of a latent family (probit.hip, student_t.hip, censored.hip,
// quantile.hip:
// each defines its model's specialisation on latent_rows.hpp, which states
// what the call leaves where), and what the Student-t model needs besides:
// launch_student_t_tau draws scalars->obs_prec = gamma_draw(Philox(seed,
// stream, 0), n/2) / (S/2), S = sum_i latent_i (y_i - psi_i)^2 with the
// weights in place; student_t_row_const is the log-likelihood's row constant.
// latent_family_name: a latent model's name in messages, else nullptr.
template <int MODEL>
int launch_latent_rows(bbx_chain* c, uint64_t stream, int* row_blocks);
template <> int launch_latent_rows<BBX_MODEL_PROBIT>(bbx_chain*, uint64_t, int*);
template <> int launch_latent_rows<BBX_MODEL_STUDENT_T>(bbx_chain*, uint64_t, int*);
template <> int launch_latent_rows<BBX_MODEL_CENSORED>(bbx_chain*, uint64_t, int*);
template <> int launch_latent_rows<BBX_MODEL_QUANTILE>(bbx_chain*, uint64_t, int*);
int launch_student_t_tau(bbx_chain* c, uint64_t stream);
double student_t_row_const(double nu);
// The quantile model's (quantile.hip): scalars->obs_prec = gamma_draw(Philox(
// seed, stream, 0), 3n/2) / S, S = sum_i [1 / w_i + w_i (r_i - theta / w_i)^2 /
// (2 kappa2)] with the weights in place; `init`: n / sum_i rho_q(r_i), no draw.
// quantile_row_const is log(q (1 - q)).
int launch_quantile_tau(bbx_chain* c, uint64_t stream, bool init);
double quantile_row_const(double q);
const char* latent_family_name(int model);

// ---- what the n-length kernels of chain.hip and of the latent families share

inline int grid_for(int64_t len, int cap) {
  int64_t nb = (len + 255) / 256;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// The grid of a row kernel: from ROW_GRID x 256 rows on a lane takes a second
// row.
inline int row_grid(int64_t n) { return grid_for(n, ROW_GRID); }

// Block totals of blocks of 256 in a fixed order: the waves' sums, added by
// thread 0 in index order.  Thread 0 holds the result.
__device__ inline double block_total_256(double x) {
  __shared__ double s_w[256 / WAVE];
  x = wave_allsum(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_w[threadIdx.x / WAVE] = x;
  __syncthreads();
  double r = 0.;
  if (threadIdx.x == 0)
    for (int k = 0; k < 256 / WAVE; ++k) r += s_w[k];
  __syncthreads();
  return r;  // thread 0 only
}

// ... of two lane values at once, in place
__device__ inline void block_totals_256(double& a, double& b) {
  __shared__ double s_a[256 / WAVE], s_b[256 / WAVE];
  a = wave_allsum(a);
  b = wave_allsum(b);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    s_a[threadIdx.x / WAVE] = a;
    s_b[threadIdx.x / WAVE] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0.;
    b = 0.;
    for (int k = 0; k < 256 / WAVE; ++k) {
      a += s_a[k];
      b += s_b[k];
    }
  }
}

// One block: `count` partials, lane t taking t, t + 256, ... in that order
__device__ inline double sum_row_parts(const double* part, int count) {
  double acc = 0.;
  for (int k = threadIdx.x; k < count; k += 256) acc += part[k];
  return block_total_256(acc);
}

}  // namespace bbx
