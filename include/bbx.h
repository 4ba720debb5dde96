/*
 * bbx.h -- C ABI of libbbx.so: the MI355X (gfx950) implementation of the
 * bayes-bridge CG-accelerated regression-coefficient sampler.
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes
 * plain pointers and sizes, returns an int status and never throws.  The
 * reference interface each one replaces is cited as file:line relative to the
 * upstream repository (OHDSI/bayes-bridge, version 0.2.6).
 *
 * Status convention (mirrors SciPy's `info` of scipy.sparse.linalg.cg, which
 * the reference inspects at cg_sampler.py:82-92):
 *     0   success
 *   < 0   invalid input / runtime failure (see bbx_last_error())
 *   > 0   only from the CG entry points: the solver stopped at `maxiter`
 *         without reaching the tolerance; the result is still written, as the
 *         reference does (it warns and continues, cg_sampler.py:82-87).
 *
 * Threading/ownership: a handle is bound to one HIP device and one stream and
 * is NOT thread-safe (the reference is single-threaded and uses the process
 * global RNG, cg_sampler.py:51-62).  Host pointers are caller-owned and are
 * only read/written for the duration of the call.  The library owns the device
 * copies of X (both orientations) and all persistent work vectors.
 *
 * The ctypes precedent in the reference for such a boundary is
 * design_matrix/mkl_matvec.py:17-56 (MKL `mkl_dcsrmv`).
 */
#ifndef BBX_H
#define BBX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 113: + bbx_design_predictive_summary: posterior prediction, log pointwise
 *      predictive density and the WAIC terms of the linear, logit and Poisson
 *      models.  One new symbol and nothing else, so the number stays 113.
 *      + prediction from the Cox handles: the cumulative baseline hazard and
 *      the martingale residuals of every handle type (BBX_COX_PREDICT_DECL)
 *      and bbx_cox_survival_summary.  New symbols and nothing else, so the
 *      number stays 113.
 *      + the negative-binomial likelihood with a dispersion parameter
 *      (bbx_negbin_*: create, destroy, the shared entry points of every
 *      likelihood handle, set_dispersion, dispersion_loglik) and its
 *      prediction (bbx_design_predictive_summary_negbin).  New symbols and
 *      nothing else, so the number stays 113.
 *      + the proportional-odds model of an ordered outcome with K - 1
 *      cutpoints (bbx_ordinal_*: create, destroy, the shared entry points of
 *      every likelihood handle, set_cutpoints, cutpoint_loglik) and its
 *      prediction (bbx_design_predictive_summary_ordinal).  New symbols and
 *      nothing else, so the number stays 113.
 *      + the Weibull proportional-hazards model of right-censored times with
 *      a shape parameter (bbx_weibull_*: create, destroy, the shared entry
 *      points of every likelihood handle, set_shape, shape_loglik) and its
 *      prediction (bbx_design_predictive_summary_weibull).  New symbols and
 *      nothing else, so the number stays 113.
 *      + the Fine-Gray competing-risks model (bbx_coxfg_*: create, destroy and
 *      the shared entry points of every likelihood handle).  New symbols and
 *      nothing else, so the number stays 113.
 *      + Efron's approximation for tied event times in the Cox model
 *      (bbx_coxef_*), on the plain handle's arrays, with the trajectory and
 *      the No-U-Turn sampler of the Cox handle.
 *      + case weights in the Cox model (bbx_coxw_*: create, destroy and the
 *      shared entry points of every likelihood handle).  New symbols and
 *      nothing else, so the number stays 113: a binding written against 113
 *      before them runs unchanged, one that needs them looks them up.
 *      + the probit model on the device chain (BBX_MODEL_PROBIT,
 *      bbx_chain_get_latent, bbx_chain_get_zbase, bbx_device_truncated_normal,
 *      bbx_design_predictive_summary_probit; in libbbx_hostrng
 *      bbx_replay_truncated_normal and bbx_host_log_norm_cdf).  A new model code
 *      and new symbols and nothing else, so the number stays 113.
 *      + the Student-t regression model on the device chain
 *      (BBX_MODEL_STUDENT_T, bbx_chain_set_df, bbx_chain_get_df,
 *      bbx_design_predictive_summary_student_t; bbx_chain_get_latent serves
 *      it too).  Again a new model code and new symbols: the number stays 113.
 *      + the censored-outcome model on the device chain (BBX_MODEL_CENSORED,
 *      bbx_chain_create_censored, bbx_device_censored_normal,
 *      bbx_design_predictive_summary_censored; bbx_chain_get_latent serves it
 *      too).  Again a new model code and new symbols: the number stays 113.
 *      + the quantile regression model on the device chain
 *      (BBX_MODEL_QUANTILE, bbx_chain_set_quantile, bbx_chain_get_quantile,
 *      bbx_device_inverse_gaussian, bbx_design_predictive_summary_quantile;
 *      bbx_chain_get_latent serves it too; in libbbx_hostrng
 *      bbx_replay_inverse_gaussian).  Again a new model code and new symbols:
 *      the number stays 113.
 * 112: + the Cox model in counting-process form (bbx_coxcp_*): delayed entry
 *      and (start, stop] rows, with the trajectory and the No-U-Turn sampler
 *      of the Cox handle.
 * 111: + the conditional Poisson likelihood (bbx_cpoisson_*): counts with one
 *      nuisance baseline rate per stratum, conditioned on the stratum totals,
 *      with the trajectory and the No-U-Turn sampler of the Cox handle.
 * 110: + strata in the Cox model (bbx_cox_create_stratified): one partial
 *      likelihood per stratum on shared coefficients, through every other
 *      bbx_cox_* entry point unchanged.
 * 109: + the Poisson likelihood (log link, exposure offset) with the HMC
 *      trajectory and the No-U-Turn sampler of the Cox handle (bbx_poisson_*).
 * 108: + the logit likelihood with the HMC trajectory and the No-U-Turn
 *      sampler of the Cox handle (bbx_logit_*).
 * 107: + the No-U-Turn sampler on the Cox model (bbx_cox_nuts_*).
 * 106: + bbx_design_transposed_fisher_info, bbx_woodbury_sample (the n-space
 *      draw for dense designs with more columns than rows; the reference leaves
 *      it as a TODO, gibbs_util.py:66-68), BBX_SAMPLER_WOODBURY; dense designs
 *      of more than 19 200 columns.
 * 105: + the Cox likelihood and its HMC trajectory (bbx_cox_*).
 * 103: + bbx_design_cg_stats (solves and launches enqueued past the stopping
 *      iteration since the last reset), bbx_launch_count, bbx_chain_set_progress.
 * 102: + bbx_design_create_csr64 (64-bit index arrays, 2^31 or more entries).
 * 101: bbx_design_tiled_info takes nine pointers (`packed`, since round 4),
 *      bbx_setup_lock_acquire/_release, bbx_design_useful_bytes.  A binding
 *      compares bbx_version() with the BBX_VERSION it was written against
 *      (bayesbridge_amd/_lib.py does) instead of calling with a stale arity. */
#define BBX_VERSION 113 /* 0.1.13 */

/* status codes */
#define BBX_OK 0
#define BBX_ERR_INVALID (-1)   /* bad argument (shape, NULL pointer, ...)      */
#define BBX_ERR_HIP (-2)       /* a HIP runtime call failed                     */
#define BBX_ERR_NODEVICE (-3)  /* no usable gfx950 device                       */
#define BBX_ERR_NUMERIC (-4)   /* NaN/Inf or non-positive curvature inside CG   */
#define BBX_ERR_STATE (-5)     /* call order violated (e.g. chain not set up)   */

/* storage formats of the sparse operator (bbx_design_create_csr `format`) */
#define BBX_FORMAT_AUTO 0  /* tiled when it applies, else csr                   */
#define BBX_FORMAT_CSR 1   /* reference layout: f64 values + i32 indices, CSR of
                              X and CSR of X^T (sparse_matrix.py:49,96,126)     */
#define BBX_FORMAT_TILED 2 /* LDS-tiled panels: u16 block-local indices, values
                              dropped when every stored entry is 1.0 (the idea
                              of cython_matmal/binary_matmul.pyx:21-25)         */

/* dtypes of dense storage */
#define BBX_F64 0
#define BBX_F32 1

/* likelihood families of a chain (model/factory.py:53-66) */
#define BBX_MODEL_LINEAR 0
#define BBX_MODEL_LOGIT 1
#define BBX_MODEL_PROBIT 2 /* Albert-Chib latents: no counterpart in the
                              reference; see bbx_chain_create                   */
#define BBX_MODEL_CENSORED 4 /* normal outcome with right- and left-censored
                                rows (log-normal AFT, Tobit): no counterpart in
                                the reference; see bbx_chain_create_censored   */
#define BBX_MODEL_STUDENT_T 3 /* linear regression with Student-t errors as a
                                 scale mixture of normals: no counterpart in
                                 the reference; see bbx_chain_create            */
#define BBX_MODEL_QUANTILE 5 /* quantile regression at a fixed level q: the
                                asymmetric-Laplace likelihood as a scale
                                mixture of normals; no counterpart in the
                                reference; see bbx_chain_create                 */

/* global-scale update of a chain: SamplerOptions.gscale_update
 * (gibbs_util.py:9-31; bayesbridge.py:412-448) */
#define BBX_GSCALE_SAMPLE 0   /* 'sample': conjugate Gamma draw of tau^-alpha  */
#define BBX_GSCALE_OPTIMIZE 1 /* 'optimize': Monte-Carlo EM step
                                 (bayesbridge.py:450-456)                       */
#define BBX_GSCALE_FIXED 2    /* None: tau stays at its current value           */

typedef struct bbx_design bbx_design; /* opaque: one design operator on one GPU */
typedef struct bbx_chain bbx_chain;   /* opaque: one device-resident Gibbs chain */
typedef struct bbx_batch bbx_batch;   /* opaque: chains that share the passes over X */

/* ---------------------------------------------------------------- library */

int bbx_version(void);
/* Thread-local text of the last failure; never NULL. */
const char* bbx_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only box; never touches a GPU
 * context beyond counting). */
int bbx_device_count(int* count);
/* Host worker threads the layout builder of a sparse design uses in this
 * process: the affinity mask, capped by the cgroup CPU quota (a box may show
 * 256 cores and grant 16), shared evenly among the LOCAL_WORLD_SIZE ranks
 * torch.distributed.run started on this node, at most 64;
 * BBX_BUILD_THREADS=N overrides.  (The reference builds nothing on extra
 * threads: SciPy's CSR is used as is, sparse_matrix.py:21-49.) */
int bbx_builder_threads(int* count);
/* Ranks that SHARE a GPU take the device-heavy part of their set-up one at a
 * time: when the environment variable BBX_SETUP_LOCK names a lock file, the
 * constructors hold an exclusive flock on it around their device work, and a
 * host wrapper brackets its own device set-up (data generation) with this
 * pair.  The lock is process-global and RE-ENTRANT for the thread that holds
 * it: nested acquires -- a constructor called inside a bracket -- only count;
 * another thread of the same process waits until the holder's last release,
 * and a release from a thread that does not hold it is ignored.  acquire returns 1 when
 * the lock is held afterwards (release it), 0 when BBX_SETUP_LOCK is unset or
 * the file cannot be opened (a note goes to stderr; nothing to release).
 * (No counterpart in the reference: one chain per process, one process per
 * device, bayesbridge.py:109.) */
int bbx_setup_lock_acquire(void);
int bbx_setup_lock_release(void);

/* ---------------------------------------------------- design operator (L1) */

/*
 * Build the operator  X~ = [1_n | X - 1_n offset^T]  (never materialised) from
 * a host CSR matrix.  Replaces SparseDesignMatrix.__init__
 * (design_matrix/sparse_matrix.py:21-49) for the part after zero-variance
 * column removal (done by the host wrapper, abstract_matrix.py:93-107).
 *   indptr[n+1], indices[nnz]: int32, as SciPy CSR; data[nnz] f64 or NULL when
 *   every stored value is 1.0; col_offset[p] f64 or NULL (= zeros, i.e. not
 *   centred); add_intercept: 1 => shape is (n, p+1) (sparse_matrix.py:51-54).
 * The structure is validated on the device (both constructors): indptr must
 * run 0 .. nnz non-decreasing, column indices must lie in [0, p) and ascend
 * within a row (duplicates allowed, they add up like in SciPy's csr_matvec;
 * SciPy users call X.sort_indices() first) -- otherwise BBX_ERR_INVALID.
 */
int bbx_design_create_csr(int64_t n, int64_t p, int64_t nnz,
                          const int32_t* indptr, const int32_t* indices,
                          const double* data, const double* col_offset,
                          int add_intercept, int device, int format,
                          bbx_design** out);

/*
 * The same from 64-BIT index arrays: what scipy.sparse.csr_matrix holds once a
 * matrix has 2^31 or more stored entries (SparseDesignMatrix keeps whatever
 * SciPy built, design_matrix/sparse_matrix.py:49; scipy.sparse picks int64 by
 * get_index_dtype), or when it was assembled from int64 arrays.  n and p must
 * still fit int32 (column and row ids are stored as 32-bit or narrower).
 *   nnz < 2^31: narrowed copies go through bbx_design_create_csr -- same
 *     formats, same validation, same results bit for bit.
 *   nnz >= 2^31: validation, the all-ones test and the transposition run on
 *     the HOST (threads: bbx_builder_threads), the design is stored in the
 *     LDS-tiled layout only -- format must be BBX_FORMAT_AUTO or
 *     BBX_FORMAT_TILED (the reference-layout kernels index with int32), and
 *     the layouts for batched chains (bbx_batch_*) are refused with
 *     BBX_ERR_STATE: such a design runs one chain at a time.
 */
int bbx_design_create_csr64(int64_t n, int64_t p, int64_t nnz,
                            const int64_t* indptr, const int64_t* indices,
                            const double* data, const double* col_offset,
                            int add_intercept, int device, int format,
                            bbx_design** out);

/* Same, but indptr/indices/data/col_offset are DEVICE pointers on `device`
 * (used when the matrix is generated on the GPU; the arrays are copied, the
 * caller keeps ownership). */
int bbx_design_create_csr_dev(int64_t n, int64_t p, int64_t nnz,
                              const int32_t* d_indptr, const int32_t* d_indices,
                              const double* d_data, const double* d_col_offset,
                              int add_intercept, int device, int format,
                              bbx_design** out);

/*
 * Dense operator.  Replaces DenseDesignMatrix.__init__/dot/Tdot
 * (design_matrix/dense_matrix.py:9-27,37-52).  X is row-major n x p (C order,
 * as NumPy), WITHOUT the intercept column; centring (col_offset != NULL) and
 * the intercept column are applied while the device copy is made, so the host
 * array is not modified (the reference centres the caller's array in place,
 * dense_matrix.py:21-22).  in_dtype is the dtype of X, storage_dtype the dtype
 * kept in HBM (BBX_F32 halves the traffic; all arithmetic stays f64).
 */
int bbx_design_create_dense(int64_t n, int64_t p, const void* X, int in_dtype,
                            int storage_dtype, const double* col_offset,
                            int add_intercept, int device, bbx_design** out);
/* X is a DEVICE pointer (row-major n x p, in_dtype). */
int bbx_design_create_dense_dev(int64_t n, int64_t p, const void* d_X,
                                int in_dtype, int storage_dtype,
                                const double* d_col_offset, int add_intercept,
                                int device, bbx_design** out);

int bbx_design_destroy(bbx_design* h);

/* shape -> (n, P) with P = p + add_intercept (sparse_matrix.py:51-54);
 * nnz -> stored entries of X_main (sparse_matrix.py:60-66; n*p for dense). */
int bbx_design_shape(const bbx_design* h, int64_t* n, int64_t* P);
int bbx_design_nnz(const bbx_design* h, int64_t* nnz);
int bbx_design_is_sparse(const bbx_design* h, int* flag);
/* 1 for a sparse design whose stored entries all equal 1.0 (kept value-free,
 * the counterpart of cython_matmal/binary_matmul.pyx:21-25), else 0. */
int bbx_design_is_binary(const bbx_design* h, int* flag);
/* HIP device index the handle lives on (the reference's counterpart is the
 * CuPy array's device, sparse_matrix.py:35). */
int bbx_design_device(const bbx_design* h, int* device);
/* Format actually in use (BBX_FORMAT_CSR / BBX_FORMAT_TILED; 0 for dense). */
int bbx_design_format(const bbx_design* h, int* format);
/* HBM bytes held by the operator's matrix storage (both orientations; a dense
 * design's transposed copy exists once a batch of chains has run on it). */
int bbx_design_storage_bytes(const bbx_design* h, int64_t* bytes);
/* Algorithmic HBM bytes of one dot / one Tdot in the storage format actually
 * read (nnz*(b_val+b_idx) + row pointers + in + out). */
int bbx_design_matvec_bytes(const bbx_design* h, int64_t* dot_bytes,
                            int64_t* tdot_bytes);
/* The part of those bytes that the kernels TIMED by bbx_design_get_timing
 * (which = 0 / 1) move.  Differs from bbx_design_matvec_bytes where a product
 * is more than one kernel and only the main one is stamped: the tiled and
 * dense Tdot write partial slabs that a separate epilogue kernel adds up
 * (the epilogue's slab read and its P-vector output are not counted here). */
int bbx_design_timed_bytes(const bbx_design* h, int64_t* dot_bytes,
                           int64_t* tdot_bytes);
/* The USEFUL part of bbx_design_timed_bytes: the stored entries at the
 * layout's index rate (tiled: 2 bytes per entry, 1.6 in groups of five, + 8 per
 * stored value -- no padding of the 16-byte steps, no schedules), the slices'
 * row ids, the vector in, the output.  *pad_dot / *pad_tdot = the share of the
 * id (and value) stream of X / X^T that is padding (0 for layouts without).
 * SURVEY.md 8(d) credits a kernel with the bytes it moves; this is the figure
 * beside it that a format with less padding would also have to move.  Mixed
 * designs (bbx_design_hybrid_info) and the other layouts report the timed
 * bytes.  Any output pointer may be NULL. */
int bbx_design_useful_bytes(const bbx_design* h, int64_t* dot_bytes,
                            int64_t* tdot_bytes, double* pad_dot,
                            double* pad_tdot);
/* Kernel launches per CG iteration of bbx_cg_sample / the chains on this design
 * (the loop of scipy.sparse.linalg.cg called at cg_sampler.py:77-80): 3 where
 * the direction step rides in the X~ v kernel and the update in the X~^T w
 * epilogue (tiled value-free layout with one column group), 4 where only the
 * update is merged, 5 otherwise.  Inside the CG loop the X~ v kernel that
 * bbx_design_timed_bytes describes then also moves 8 P-vectors. */
int bbx_design_cg_launches(const bbx_design* h, int* per_iteration);
/* The host side of that loop (cg_sampler.py:77-80 is a Python loop around two
 * products; here the host only enqueues, runs ahead of the device's stop test
 * and reads its outcome from a host-mapped progress word): CG solves on this
 * design since creation / the last reset, and the kernel launches they enqueued
 * past their stopping iteration (such kernels return at entry, ~2 us each);
 * `naps`: how often the host slept between two stop tests instead of polling
 * (only with fewer than three host cores per rank, or BBX_CG_SLEEP=1).
 * reset != 0 zeroes all after reading.  Output pointers may be NULL. */
int bbx_design_cg_stats(bbx_design* h, int64_t* solves, int64_t* empty_launches,
                        int64_t* naps, int reset);
/* Kernel launches this process has made through the library, all designs and
 * chains (a diagnostic: launches per second and rank is what the host side of
 * an N-rank node has to sustain; the reference launches nothing). */
uint64_t bbx_launch_count(void);
/* The 3-launch form: the direction step inside the X~ v kernel -- every
 * workgroup re-adds the r.r partials (rho, stop test, beta), the kernel streams
 * X~ (s.*r) and its epilogue forms t_k = X~ (s.*r_k) + beta t_{k-1}, which is
 * X~ (s.*p_k) by linearity.  Costs the X~ v kernel two n-vector passes, saves a
 * P-vector launch: +3.5 % Gibbs it/s at 100k x 10k, -1 % at 1M x 50k, hence ON by
 * default for designs of up to 250 000 rows where it applies.  on = 1 / 0
 * switches it for this design, -1 restores the default (BBX_CG_FOLD=0|1 sets
 * it for the process).  Same recurrence as scipy.sparse.linalg.cg
 * (cg_sampler.py:77-80) either way, to rounding. */
int bbx_design_set_cg_fold(bbx_design* h, int on);
/* Algorithmic bytes of the single-pass dense operator kernel X^T(Omega (X v))
 * (dense designs that qualify for it; 0 otherwise): one pass over the stored
 * matrix + v + Omega + the per-workgroup slabs it writes. */
int bbx_design_fused_operator_bytes(const bbx_design* h, int64_t* bytes);

/* Mixed designs (binary covariates plus a few continuous ones: the reference's
 * tests build simulate_design(n, p, binary_frac=.9), tests/helper.py:13) are
 * stored split by VALUE in the tiled format: the entries equal to 1.0 in the
 * value-free layout, the other entries of columns that hold many of them in a
 * dense column-major f64 block, what is left in the valued layout; the three
 * products are added in a fixed order.  *is_hybrid says whether that happened,
 * the counts how the entries were divided. */
int bbx_design_hybrid_info(const bbx_design* h, int* is_hybrid,
                           int64_t* ones_nnz, int64_t* rest_nnz,
                           int64_t* dense_nnz, int* dense_cols);
/* Which form the LAST X~ v and the last X~^T w of a mixed design took (written
 * on the host where the kernels are launched; 0 before the first product, and
 * for designs that are not mixed):
 *   *dot_form   BBX_HYB_DOT_EPI             dense block in the value-free
 *                                           kernel's epilogue (kd <= 8)
 *               BBX_HYB_DOT_FUSED_WAVE      one pass over the row-major block,
 *                                           a wave per row; *dot_width = column
 *                                           pairs per lane (1, 2, 4, 8)
 *               BBX_HYB_DOT_FUSED_WG        ... a workgroup per row block;
 *                                           *dot_width = 1, 2, 4
 *               BBX_HYB_DOT_SEPARATE        addend kernel, direct epilogue
 *               BBX_HYB_DOT_SEPARATE_SLABS  addend kernel, slabs + finalize
 *   *tdot_form  BBX_HYB_TDOT_DW_REUSED      D^T w from the partials the X~ v
 *                                           kernel of the same operator
 *                                           application left
 *               BBX_HYB_TDOT_SEPARATE       its own pass over D (or no D)
 * Any output pointer may be NULL. */
enum {
  BBX_HYB_DOT_NONE = 0,
  BBX_HYB_DOT_EPI = 1,
  BBX_HYB_DOT_FUSED_WAVE = 2,
  BBX_HYB_DOT_FUSED_WG = 3,
  BBX_HYB_DOT_SEPARATE = 4,
  BBX_HYB_DOT_SEPARATE_SLABS = 5
};
enum {
  BBX_HYB_TDOT_NONE = 0,
  BBX_HYB_TDOT_DW_REUSED = 1,
  BBX_HYB_TDOT_SEPARATE = 2
};
int bbx_design_hybrid_forms(const bbx_design* h, int* dot_form, int* dot_width,
                            int* tdot_form);
/* Geometry of the tiled format (BBX_FORMAT_TILED only): which = 0 for X, 1 for
 * X^T; W = column-block width, n_block = column blocks, PR = rows per panel,
 * G = column-block groups (partial-sum slabs), n_quad = 1024-byte steps (16
 * bytes x 64 lanes: per lane four 16-bit ids, or -- *packed = 1, value-free
 * designs -- one group of up to five entries, for each of its two rows),
 * n_slice = 128-row slices.  Any output pointer may be NULL. */
int bbx_design_tiled_info(const bbx_design* h, int which, int* W,
                          int* n_block, int* PR, int* G, int64_t* n_quad,
                          int64_t* n_slice, int* packed);

/*
 * out[n] = X~ v,  v[P].  Replaces SparseDesignMatrix.dot / main_dot
 * (sparse_matrix.py:68-101) and DenseDesignMatrix.dot (dense_matrix.py:37-48):
 *   out = v[0] + X_main v[1:] - <offset, v[1:]>.
 * Host pointers; synchronous.
 */
int bbx_design_dot(bbx_design* h, const double* v, double* out);
/*
 * out[P] = X~^T w,  w[n].  Replaces SparseDesignMatrix.Tdot / main_Tdot
 * (sparse_matrix.py:103-129) and DenseDesignMatrix.Tdot (dense_matrix.py:50-52):
 *   out = [sum(w) ; X_main^T w - sum(w) * offset].
 */
int bbx_design_tdot(bbx_design* h, const double* w, double* out);
/* Device-pointer forms: asynchronous on the handle's stream, which is a
 * NON-BLOCKING stream (it does not wait for the legacy null stream).  The
 * caller's buffers must be complete when the call is made (synchronise the
 * stream that produced them, or launch the producer on bbx_design_stream()),
 * and d_out is ready after bbx_design_synchronize().  The constructors taking
 * device pointers synchronise the whole device once before they start. */
int bbx_design_dot_dev(bbx_design* h, const double* d_v, double* d_out);
int bbx_design_tdot_dev(bbx_design* h, const double* d_w, double* d_out);

/*
 * out[P] = X~^T (obs_prec .* (X~ v)): the data part of the CG operator
 * (the closure at cg_sampler.py:106-109 without the diagonal scalings; also the
 * Hessian-matvec of the likelihood, logistic_model.py:62-78), issued through
 * the same launches the CG loop uses -- for dense designs that qualify this is
 * the single-pass kernel, so the entry lets a test compare it with the two
 * separate products.  Host pointers, synchronous; `_dev`: device pointers,
 * asynchronous on the handle's stream.
 * Mixed designs: the one-pass forms of the dense block (bbx_design_hybrid_forms:
 * EPI, FUSED_WAVE, FUSED_WG) need v + intercept 16-byte aligned.  The host
 * entry stages v at the start of an aligned buffer, so a design WITH an
 * intercept runs the separate kernels here (the CG loop, whose vectors start
 * one element into their buffers, runs the one-pass forms); a design without
 * one, or a `_dev` caller who passes d_v with d_v + 1 aligned, gets them.
 */
int bbx_design_gram_matvec(bbx_design* h, const double* obs_prec,
                           const double* v, double* out);
int bbx_design_gram_matvec_dev(bbx_design* h, const double* d_obs_prec,
                               const double* d_v, double* d_out);

/*
 * Fisher information of a DENSE design (dense_matrix.py:54-58):
 *   out = X~^T diag(weight) X~     (P x P, row-major, symmetric), or
 *   out = diag of it                (P entries) when diag_only != 0,
 * with weight[n] (NULL: ones).  X~ is the stored matrix: intercept column,
 * centred, and for f32 storage the f32-rounded values (accumulated in f64).
 * Bitwise reproducible.  A sparse design returns BBX_ERR_INVALID.
 * Host pointers, synchronous; `_dev`: device pointers, asynchronous on the
 * handle's stream (d_out is ready after bbx_design_synchronize()).
 */
int bbx_design_fisher_info(bbx_design* h, const double* weight, int diag_only,
                           double* out);
int bbx_design_fisher_info_dev(bbx_design* h, const double* d_weight,
                               int diag_only, double* d_out);

/*
 * The direct ('cholesky') coefficient draw of direct_gaussian_sampler.py:4-44
 * on a DENSE design:
 *   F = X~^T diag(obs_prec) X~, d = prior_prec_sqrt^2 + diag(F), s = 1/sqrt(d),
 *   A = diag(s) F diag(s) + diag((s prior_prec_sqrt)^2) = U^T U (U upper),
 *   coef_out = s .* (A^-1 (s .* z) + U^-1 normals)
 * with obs_prec[n], prior_prec_sqrt[P], z[P] (= X~^T (obs_prec .* y)) and
 * normals[P] (the reference's np.random.randn(P)).
 * bbx_chol_sample_scalar: obs_prec is one number (linear models); F is then
 * obs_prec * (X~^T X~) with X~^T X~ computed once per design and cached, which
 * rounds differently from forming X~^T (obs_prec X~).
 * Returns BBX_ERR_NUMERIC, with the first non-positive pivot in
 * bbx_last_error(), when A is not numerically positive definite (coef_out is
 * then unspecified; the design stays usable); BBX_ERR_INVALID on a sparse
 * design or a NULL array.  All forms synchronise the handle's stream before
 * they return: coef_out / d_coef_out is complete on return.
 */
int bbx_chol_sample(bbx_design* h, const double* obs_prec,
                    const double* prior_prec_sqrt, const double* z,
                    const double* normals, double* coef_out);
int bbx_chol_sample_dev(bbx_design* h, const double* d_obs_prec,
                        const double* d_prior_prec_sqrt, const double* d_z,
                        const double* d_normals, double* d_coef_out);
int bbx_chol_sample_scalar(bbx_design* h, double obs_prec,
                           const double* prior_prec_sqrt, const double* z,
                           const double* normals, double* coef_out);
/* The sampler keeps its work memory on the design after a call: a P x P f64
 * matrix (A and its factor, Pp = P rounded up to 64: 8 Pp^2 bytes, 2.9 GB at
 * 19 200 columns), a second one once bbx_chol_sample_scalar has cached
 * X~^T X~, and up to 256 MB of Gram partials.  bbx_chol_release frees all of
 * it (the next call allocates it again); bbx_design_destroy does too. */
int bbx_chol_release(bbx_design* h);

/*
 * Transposed Fisher information of a DENSE design (the reference declares
 * compute_transposed_fisher_info, dense_matrix.py:60-61, with an empty body;
 * the meaning is fixed here):
 *   out = X~ diag(weight) X~^T      (n x n, row-major, symmetric bit for bit)
 * with weight[P] >= 0 over ALL columns of the stored matrix, the intercept
 * column included (give it weight 0 to leave it out).  f64 accumulation on
 * the matrix cores, bitwise reproducible.  A sparse design, n > 19 200 or a
 * NULL array returns BBX_ERR_INVALID.  Host pointers, synchronous; `_dev`:
 * device pointers, asynchronous on the handle's stream.
 */
int bbx_design_transposed_fisher_info(bbx_design* h, const double* weight,
                                      double* out);
int bbx_design_transposed_fisher_info_dev(bbx_design* h, const double* d_weight,
                                          double* d_out);

/*
 * The n-space ('woodbury') coefficient draw on a DENSE design, for P > n: the
 * same Gaussian as bbx_chol_sample / bbx_cg_sample,
 *   N(A^-1 X~^T (obs_prec .* y), A^-1),  A = X~^T diag(obs_prec) X~ + diag(prior_prec_sqrt^2),
 * from an n x n system (Bhattacharya, Chakraborty and Mallick 2016, extended
 * to coefficients with a flat prior; DESIGN.md 11 has the algebra):
 * n^2 P + n^3 / 3 flops and 8 n^2 bytes instead of n P^2 + P^3 / 3 and 8 P^2.
 *   obs_prec[n] > 0 (bbx_woodbury_sample_scalar: one number, linear models);
 *   prior_prec_sqrt[P] >= 0: 1 / prior sd; a ZERO marks a coefficient with a
 *     flat prior (the intercept under the default prior), at most 32 of them,
 *     and their columns must be linearly independent;
 *   y[n]: the (pseudo-)outcome;
 *   normals_n[n], normals_P[P]: standard normals; normals_P[j] belongs to
 *     coefficient j;
 *   coef_out[P].
 * Returns BBX_ERR_NUMERIC, with the first non-positive pivot in
 * bbx_last_error(), when a factorisation fails; BBX_ERR_INVALID on a sparse
 * design, n > 19 200 (the n x n matrix would pass 2.9 GB), more than 32 flat
 * coefficients, a negative prior_prec_sqrt or a NULL array.  All forms
 * synchronise the handle's stream before they return.  Work memory (8 n_pad^2
 * bytes, n_pad = n rounded up to 64, the Gram partials of at most 256 MB, and
 * about 80 n-vectors) stays on the design until bbx_chol_release.
 */
int bbx_woodbury_sample(bbx_design* h, const double* obs_prec,
                        const double* prior_prec_sqrt, const double* y,
                        const double* normals_n, const double* normals_P,
                        double* coef_out);
int bbx_woodbury_sample_dev(bbx_design* h, const double* d_obs_prec,
                            const double* d_prior_prec_sqrt, const double* d_y,
                            const double* d_normals_n,
                            const double* d_normals_P, double* d_coef_out);
int bbx_woodbury_sample_scalar(bbx_design* h, double obs_prec,
                               const double* prior_prec_sqrt, const double* y,
                               const double* normals_n, const double* normals_P,
                               double* coef_out);

/* The hipStream_t (as void*) every kernel of this handle is launched on, and a
 * blocking wait on it. */
int bbx_design_stream(bbx_design* h, void** stream);
int bbx_design_synchronize(bbx_design* h);

/* ------------------------------------------------------- CG sampler (L3) */

/*
 * One draw  beta ~ N(Sigma z, Sigma),  Sigma^-1 = X~^T diag(obs_prec) X~ +
 * diag(prior_prec_sqrt^2), by perturbation-optimisation + prior-preconditioned
 * conjugate gradient.  Replaces ConjugateGradientSampler.sample
 * (reg_coef_sampler/cg_sampler.py:20-94) with precond_by='prior'
 * (cg_sampler.py:128-138), including precondition_linear_system
 * (cg_sampler.py:96-113) and the SciPy >= 1.14 `cg` recurrence it calls
 * (cg_sampler.py:77-80).
 *
 *   obs_prec[n]          Omega
 *   prior_prec_sqrt[P]   phi = 1/prior_sd (0 for a flat prior)
 *   z[P]                 X~^T (Omega y)
 *   x0[P]                coef_cg_init (CG warm start, in beta coordinates)
 *   precond_sd[P]        coef_scaled_sd; only the first n_unshrunk entries are
 *                        used: s_j = 2*precond_sd[j] (cg_sampler.py:133-136)
 *   randn_n[n], randn_P[P]  the standard-normal draws eta1, eta2 of
 *                        cg_sampler.py:61-62 (the reference draws them from the
 *                        global NumPy RNG, n first).  Pass NULL for BOTH to
 *                        draw them on the device from Philox4x32-10 keyed by
 *                        `seed` (distribution parity only).
 *   maxiter, atol        as cg_sampler.py:22-23; the stop rule is
 *                        ||r||_2 < atol in preconditioned coordinates.
 *   coef_out[P]          the draw; n_iter_out = number of completed CG
 *                        iterations (the reference's callback count);
 *   info_out             SciPy-style info: 0 converged, maxiter if exhausted.
 * Return value: 0, or > 0 (= info) when not converged, or < 0 on error.
 */
int bbx_cg_sample(bbx_design* h, const double* obs_prec,
                  const double* prior_prec_sqrt, const double* z,
                  const double* x0, const double* precond_sd, int n_unshrunk,
                  const double* randn_n, const double* randn_P, uint64_t seed,
                  int maxiter, double atol, double* coef_out, int* n_iter_out,
                  int* info_out);
/* All array arguments are DEVICE pointers; n_iter_out/info_out stay host. */
int bbx_cg_sample_dev(bbx_design* h, const double* d_obs_prec,
                      const double* d_prior_prec_sqrt, const double* d_z,
                      const double* d_x0, const double* d_precond_sd,
                      int n_unshrunk, const double* d_randn_n,
                      const double* d_randn_P, uint64_t seed, int maxiter,
                      double atol, double* d_coef_out, int* n_iter_out,
                      int* info_out);

/* Counters of operator applications since creation / last reset, the
 * equivalent of AbstractDesignMatrix.get_dot_count / reset_matvec_count
 * (abstract_matrix.py:61-72).  Applications inside bbx_cg_sample count too:
 * n_iter products with X~ and with X~^T for the iterations, one product with
 * X~ for a non-zero warm start, and ONE product with X~^T for the initial
 * residual -- the reference's two (the right-hand side's and the one inside
 * A x0) are a single pass over X~^T here, by linearity.  A pass is a pass:
 * it counts once. */
int bbx_design_matvec_count(const bbx_design* h, int64_t* n_dot,
                            int64_t* n_tdot);
int bbx_design_reset_matvec_count(bbx_design* h);

/* ------------------------------------------------ kernel timing (profiling) */

/* enabled = 1: HIP events are recorded on the handle's stream around every
 * dot / Tdot kernel launch (also those inside the CG loop and the chain);
 * enabled = N > 1: around every N-th launch of each family only (an event pair
 * costs a few microseconds of stream time, ~10% of a Gibbs iteration when
 * every launch is timed); 0: off. */
int bbx_design_set_timing(bbx_design* h, int enabled);
/* Resolves all pending event pairs (synchronises the stream) and returns the
 * number of timed launches and their summed device time per kernel family:
 * which = 0 dot (X v; for dense designs inside the CG loop: the single-pass
 * operator kernel), 1 Tdot (X^T w, main kernel), 2 one whole application of
 * the CG operator (dot + Tdot + epilogue; bracketed by two record commands,
 * which adds ~2-3 us of dispatch to the interval).  Launches that returned at
 * entry because their CG solve had already stopped (the host enqueues ahead
 * of the stop test) are not executions and are left out: samples below half
 * the family's median are dropped. */
int bbx_design_get_timing(bbx_design* h, int which, int64_t* n_launch,
                          double* total_ms);
int bbx_design_reset_timing(bbx_design* h);

/* Attainable-HBM probe ("confirm with a device-to-device
 * copy/stream on the box"): streams a scratch buffer of `bytes` through a
 * read-only kernel and a copy kernel `reps` times each, 16 bytes per lane, and
 * returns the HIP-event rates.  read_gbps counts bytes read; copy_gbps counts
 * bytes read + written.  Diagnostic only; not on the sampling path. */
int bbx_hbm_probe(int device, int64_t bytes, int reps, double* read_gbps,
                  double* copy_gbps);

/* ------------------------------------------- device-resident Gibbs chain */

/*
 * A whole Gibbs iteration of BayesBridge.gibbs(coef_sampler_type='cg')
 * (bayesbridge.py:210-240) kept in HBM: beta | rest by the CG sampler above,
 * Omega | beta (Polya-Gamma for logit, bayesbridge.py:397-410; Gamma for the
 * linear model's precision), tau | beta (bayesbridge.py:412-448), lambda |
 * tau, beta (tilted stable, bayesbridge.py:458-478), log-posterior
 * (bayesbridge.py:480-511), and the running summaries that give the CG warm
 * start and preconditioner scale (reg_coef_posterior_summarizer.py:3-124).
 * Random numbers come from Philox4x32-10 keyed by (seed, iteration, element):
 * distribution parity with the reference, never stream parity.
 *
 *   model          BBX_MODEL_LINEAR or BBX_MODEL_LOGIT
 *   outcome[n]     y (linear) or n_success (logit)          host pointer
 *   n_trial[n]     logit only; NULL => ones                  host pointer
 *   sd_unshrunk[n_unshrunk]  prior sd of the unshrunk coefficients
 *                  (intercept first; +inf = flat prior; bayesbridge.py:26-32)
 *   bridge_exp, slab_size    prior.py:9-15
 *   gscale_shape0, gscale_rate0  Gamma prior on tau^-bridge_exp (prior.py:77-81)
 * The chain borrows `design` (which must outlive it) and its stream.
 *
 * BBX_MODEL_PROBIT (no counterpart in the reference): P(y_i = 1) = Phi(psi_i)
 * under Albert & Chib's augmentation.  outcome[n] must be 0 or 1 and n_trial
 * NULL or all ones (BBX_ERR_INVALID names the first offending row).  Each
 * iteration draws the latents z_i | beta ~ N(psi_i, 1) on z > 0 (y_i = 1) or
 * z <= 0 (y_i = 0), element i from Philox(seed, 7 | iteration << 8, i, trial);
 * beta | z is the linear model's conditional with outcome z and the
 * observation precision fixed at 1, drawn by any of the three samplers.  The
 * chain has no obs_prec: set_state, get_state and the runs refuse a non-NULL
 * one.  bbx_chain_set_state and bbx_chain_init_obs_prec recompute psi, the
 * latents, X~^T z and the log-likelihood from the coefficients with the stream
 * of iteration `iteration - 1`, so a chain resumed from (coef, lscale, gscale,
 * iteration, summaries) continues bit for bit.  bbx_batch_create refuses
 * probit chains.
 *
 * BBX_MODEL_STUDENT_T (no counterpart in the reference): y_i = psi_i + e_i with
 * e_i sqrt(tau) ~ Student-t on nu degrees of freedom, nu fixed (4 at creation:
 * bbx_chain_set_df), written as y_i | omega_i ~ N(psi_i, 1 / (tau omega_i)),
 * omega_i ~ Gamma(nu/2, rate nu/2).  outcome[n] must be finite (BBX_ERR_INVALID
 * names the first offending row) and n_trial NULL.  After the coefficient draw
 * of iteration `it`, with r = y - psi:
 *   tau     = gamma_draw(Philox(seed, 6 | it << 8, 0), n/2) / (S/2),
 *             S = sum_i omega_i r_i^2 with the omega of the iteration before;
 *   omega_i = gamma_draw(Philox(seed, 8 | it << 8, i), (nu+1)/2)
 *             / ((nu + tau r_i^2)/2) with the new tau;
 *   beta    | tau, omega is the Gaussian conditional at the per-row precision
 *             tau omega_i, drawn by any of the three samplers.
 * obs_prec is the scalar tau (length 1, as for the linear model) in set_state,
 * get_state and the runs; bbx_chain_get_latent returns omega.  The
 * log-likelihood is the marginal t-density, sum_i [1/2 log tau - (nu+1)/2
 * log1p(tau r_i^2 / nu)] + n [lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu/2)]
 * (the linear model's convention: -n/2 log 2 pi dropped).  bbx_chain_set_state,
 * bbx_chain_set_df and bbx_chain_init_obs_prec (which first sets tau =
 * 1 / mean(r^2)) recompute psi, omega, X~^T (tau omega y) and the
 * log-likelihood from (coef, tau) with the stream of iteration `iteration -
 * 1`, without redrawing tau, so a chain resumed from (coef, obs_prec, lscale,
 * gscale, iteration, summaries, seed, nu) continues bit for bit.  A psi_i that
 * is not finite gives a NaN omega_i and log-likelihood.  bbx_batch_create
 * refuses student_t chains.
 *
 * BBX_MODEL_QUANTILE (no counterpart in the reference): regression of the q-th
 * conditional quantile, q fixed in (0, 1) (1/2 at creation:
 * bbx_chain_set_quantile), under the asymmetric-Laplace likelihood p(y_i) = q (1
 * - q) tau exp(-tau rho_q(y_i - psi_i)), rho_q(u) = u (q - 1[u < 0]), written
 * (Kozumi & Kobayashi 2011) with theta = (1 - 2q) / (q (1 - q)) and kappa2 = 2 /
 * (q (1 - q)) as v_i ~ Exp(rate tau), y_i | v_i ~ N(psi_i + theta v_i, kappa2
 * v_i / tau); the stored latent is w_i = 1 / v_i.  outcome[n] must be finite
 * (BBX_ERR_INVALID names the first offending row) and n_trial NULL.  After the
 * coefficient draw of iteration `it`, with r = y - psi:
 *   tau  = gamma_draw(Philox(seed, 6 | it << 8, 0), 3n/2) / S, S = sum_i [1 /
 *          w_i + w_i (r_i - theta / w_i)^2 / (2 kappa2)] with the w of the
 *          iteration before (the prior is 1 / tau, the linear model's);
 *   w_i  ~ InverseGaussian(mean 1 / (q (1 - q) |r_i|), shape tau / (2 q (1 -
 *          q))) with the new tau, from one normal z and one uniform u of
 *          Philox(seed, 9 | it << 8, i) in this order: with m = q (1 - q) |r_i|,
 *          lambda the shape and s = z^2 / (2 lambda), x = 1 / (m + s + sqrt(s^2 +
 *          2 s m)), w = x where u (1 + m x) <= 1, else 1 / (m (m x)); at r_i = 0
 *          that is Levy's law lambda / z^2;
 *   beta | tau, w is the Gaussian conditional at the per-row precision Omega_i =
 *          tau w_i / kappa2 with kappa_i = Omega_i y_i - tau theta / kappa2,
 *          drawn by any of the three samplers.
 * obs_prec is the scalar tau (length 1, as for the linear model) in set_state,
 * get_state and the runs; bbx_chain_get_latent returns w.  The log-likelihood is
 * sum_i [log tau - tau rho_q(r_i)] + n log(q (1 - q)).  bbx_chain_set_state,
 * bbx_chain_set_quantile and bbx_chain_init_obs_prec (which first sets tau = 1 /
 * mean rho_q(r), the likelihood's maximiser in tau) recompute psi, w, X~^T kappa
 * and the log-likelihood from (coef, tau) with the stream of iteration
 * `iteration - 1`, without redrawing tau, so a chain resumed from (coef,
 * obs_prec, lscale, gscale, iteration, summaries, seed, q) continues bit for
 * bit.  A psi_i that is not finite gives a NaN w_i and log-likelihood; |r_i| up
 * to 1e150 gives a finite positive w_i (beyond about 1e300 the draw's s m can
 * overflow and the weight be 0).  bbx_batch_create refuses quantile chains.
 */
int bbx_chain_create(bbx_design* design, int model, const double* outcome,
                     const double* n_trial, int n_unshrunk,
                     const double* sd_unshrunk, double bridge_exp,
                     double slab_size, double gscale_shape0,
                     double gscale_rate0, uint64_t seed, bbx_chain** out);
/*
 * BBX_MODEL_CENSORED (no counterpart in the reference): bbx_chain_create's
 * arguments with the row status where n_trial stands; bbx_chain_create itself
 * refuses the model, and this entry refuses every other one.  Row i has a value
 * bound[i] (finite) and status[i]: 0 observed (z_i = bound_i), 1 right-censored
 * (z_i > bound_i), 2 left-censored (z_i <= bound_i; the open and closed sides
 * are the probit model's); BBX_ERR_INVALID names the first row with a bound
 * that is not finite or a status above 2.  z_i ~ N(psi_i, 1 / tau): the
 * accelerated-failure-time model with log-normal errors when bound = log t,
 * the Tobit model when the outcome is censored at a limit.  After the
 * coefficient draw of iteration `it`:
 *   tau = gamma_draw(Philox(seed, 6 | it << 8, 0), n/2) / (S/2), S = sum_i
 *         (z_i - psi_i)^2 with the latents of the iteration before: the linear
 *         model's rule and kernels with z for y;
 *   z_i = bound_i + u / sqrt(tau) on a censored row, u ~ N(psi', 1) on u > 0
 *         (status 1) or u <= 0 (status 2), psi' = (psi_i - bound_i) sqrt(tau),
 *         trial t on Philox(seed, 7 | it << 8, i, t), with the new tau;
 *   beta | tau, z is the linear model's conditional with z for y, drawn by any
 *         of the three samplers (the direct ones from the cached Gram).
 * obs_prec is the scalar tau (length 1, as for the linear model);
 * bbx_chain_get_latent returns z.  The log-likelihood is sum over observed rows
 * of 1/2 log tau - 1/2 tau (bound - psi)^2 (the linear model's convention:
 * -1/2 log 2 pi dropped) plus sum over censored rows of log Phi(+-psi').  At
 * creation z = bound.  bbx_chain_set_state and bbx_chain_init_obs_prec (which
 * first sets tau = 1 / mean((bound - psi)^2)) recompute psi, z, X~^T z and the
 * log-likelihood from (coef, tau) with the stream of iteration `iteration - 1`
 * (-1: a chain that has not run), without redrawing tau, so a chain resumed
 * from (coef, obs_prec, lscale, gscale, iteration, summaries, seed) continues
 * bit for bit.  A psi_i that is not finite gives a NaN log-likelihood and, on a
 * censored row, a NaN latent.  bbx_batch_create refuses censored chains.
 */
int bbx_chain_create_censored(bbx_design* design, int model,
                              const double* bound, const unsigned char* status,
                              int n_unshrunk, const double* sd_unshrunk,
                              double bridge_exp, double slab_size,
                              double gscale_shape0, double gscale_rate0,
                              uint64_t seed, bbx_chain** out);
int bbx_chain_destroy(bbx_chain* c);

/* Markov-chain state, host pointers.  obs_prec has n entries for logit and 1
 * for linear; lscale has P - n_unshrunk entries; gscale is in the RAW
 * parametrisation the sampler runs in (prior.py:129-141).  NULL = leave. */
int bbx_chain_set_state(bbx_chain* c, const double* coef,
                        const double* obs_prec, const double* lscale,
                        const double* gscale);
int bbx_chain_get_state(bbx_chain* c, double* coef, double* obs_prec,
                        double* lscale, double* gscale);
/* Running summaries (checkpoint/resume: bayesbridge.py:253-275,
 * reg_coef_sampler.py:42-58). */
int bbx_chain_set_summary(bbx_chain* c, const double* mean,
                          const double* square, int64_t n_averaged);
int bbx_chain_get_summary(bbx_chain* c, double* mean, double* square,
                          int64_t* n_averaged);
/* Omega at its initial value for the current coef: Polya-Gamma mean for logit
 * (logistic_model.py:80-87), 1/mean(resid^2) for linear
 * (bayesbridge.py:355-370). */
int bbx_chain_init_obs_prec(bbx_chain* c);
/* Iterations done so far (keys the Philox streams; settable for resume). */
int bbx_chain_get_iteration(bbx_chain* c, int64_t* iteration);
int bbx_chain_set_iteration(bbx_chain* c, int64_t iteration);
/* The Philox key of the chain (bbx_chain_create's `seed`); settable so that a
 * handle can continue another run's streams (gibbs_resume,
 * bayesbridge.py:43-107 restores the generator state the same way). */
int bbx_chain_get_seed(bbx_chain* c, uint64_t* seed);
int bbx_chain_set_seed(bbx_chain* c, uint64_t seed);
/* How tau is updated each iteration: BBX_GSCALE_SAMPLE (default),
 * BBX_GSCALE_OPTIMIZE or BBX_GSCALE_FIXED (bayesbridge.py:412-448 `method`). */
int bbx_chain_set_gscale_update(bbx_chain* c, int mode);
/* How the chain draws beta | rest: BBX_SAMPLER_CG (default) or, on DENSE
 * designs only (else BBX_ERR_INVALID), BBX_SAMPLER_CHOLESKY -- the direct draw
 * of bbx_chol_sample with the P normals of the CG draw's eta2 stream
 * (bbx_chain_eta), no running summary (its state is left as it is), n_cg_iter
 * 0 and no unconverged solves.  bbx_batch_create refuses such chains. */
#define BBX_SAMPLER_CG 0
#define BBX_SAMPLER_CHOLESKY 1
/* BBX_SAMPLER_WOODBURY (dense designs only, refused by bbx_batch_create like
 * BBX_SAMPLER_CHOLESKY): the draw of bbx_woodbury_sample; normals_n is the
 * chain's eta1 stream and normals_P its eta2 stream (bbx_chain_eta), no
 * running summary, n_cg_iter 0. */
#define BBX_SAMPLER_WOODBURY 2
int bbx_chain_set_coef_sampler(bbx_chain* c, int sampler);
/*
 * Regenerates, on the device, the standard normals the chain's CG draw
 * consumes at 0-based iteration `iteration` (cg_sampler.py:61-62: eta1[n] for
 * the likelihood part, eta2[P] for the prior part) and copies them to the
 * host.  Philox is counter-based, so this does not disturb the chain; it
 * exists so that a test can feed the very same perturbation to the CPU oracle
 * and compare the device chain's draw exactly.
 */
int bbx_chain_eta(bbx_chain* c, int64_t iteration, double* eta1, double* eta2);
/* Log-likelihood and log-posterior of the state left by the last iteration
 * (bayesbridge.py:480-511), host pointers, either may be NULL. */
int bbx_chain_get_logp(bbx_chain* c, double* loglik, double* logp);
/* The n latents of a BBX_MODEL_PROBIT or BBX_MODEL_CENSORED chain's current
 * state, or the n mixing weights omega of a BBX_MODEL_STUDENT_T chain's, or the
 * n mixing weights w of a BBX_MODEL_QUANTILE chain's (host pointer);
 * BBX_ERR_INVALID for a chain of another model or a NULL out. */
int bbx_chain_get_latent(bbx_chain* c, double* out);
/* The degrees of freedom nu of a BBX_MODEL_STUDENT_T chain (4 at creation).
 * Setting them recomputes the weights, X~^T kappa and the log-likelihood of
 * the current (coef, tau) under the new nu, as bbx_chain_set_state does.
 * BBX_ERR_INVALID for a chain of another model, a df that is not finite and
 * positive, a NULL df pointer. */
int bbx_chain_set_df(bbx_chain* c, double df);
int bbx_chain_get_df(bbx_chain* c, double* df);
/* The level q of a BBX_MODEL_QUANTILE chain (1/2 at creation).  Setting it
 * recomputes the weights, X~^T kappa and the log-likelihood of the current
 * (coef, tau) under the new q, as bbx_chain_set_state does.  BBX_ERR_INVALID for
 * a chain of another model, a q outside (0, 1), a NULL quantile pointer. */
int bbx_chain_set_quantile(bbx_chain* c, double quantile);
int bbx_chain_get_quantile(bbx_chain* c, double* quantile);
/* The P-vector the next draw's right-hand side is scaled from: X~^T kappa
 * (logit), X~^T y (linear), X~^T z of the current latents (probit), X~^T (tau
 * omega y) of the current weights (student_t); host pointer.  For the tests that pin it to the latents. */
int bbx_chain_get_zbase(bbx_chain* c, double* out);

/*
 * Runs n_iter Gibbs iterations; a sample is kept every `thin` iterations
 * after `n_burnin` (gibbs_util.py:164-189), n_sample = (n_iter-n_burnin)/thin.
 *   maxiter, atol   of the CG solve; atol <= 0 => 1e-5*sqrt(P)
 *                   (reg_coef_sampler.py:95), maxiter <= 0 => 500.
 *   d_coef[n_sample*P]       DEVICE buffer, sample-major (sample s at s*P), or NULL
 *   d_lscale[n_sample*(P-n_unshrunk)], d_obs_prec[n_sample*n (logit) |
 *                   n_sample (linear)]   DEVICE buffers or NULL
 *   gscale[n_sample], logp[n_sample], n_cg_iter[n_sample]   HOST buffers or NULL
 * Returns 0, or the number of iterations whose CG solve hit maxiter (> 0), or
 * < 0 on error.
 */
int bbx_chain_run(bbx_chain* c, int n_iter, int n_burnin, int thin,
                  int maxiter, double atol, double* d_coef, double* d_lscale,
                  double* d_obs_prec, double* gscale, double* logp,
                  double* n_cg_iter);
/* Progress of a run (BayesBridge.gibbs(n_status_update=...), gibbs_util.py:
 * 214-238 prints "<k> Gibbs iterations complete: ..."): fn(iteration, ctx) is
 * called on the calling thread every `every` iterations of bbx_chain_run[_host],
 * after the coefficient draw of that iteration has been confirmed; every = 0
 * or fn = NULL switches it off.  The callback must not call back into the chain. */
int bbx_chain_set_progress(bbx_chain* c, int every, void (*fn)(int, void*),
                           void* ctx);
/* Same with HOST sample buffers for coef/lscale/obs_prec (copied at the end). */
int bbx_chain_run_host(bbx_chain* c, int n_iter, int n_burnin, int thin,
                       int maxiter, double atol, double* coef, double* lscale,
                       double* obs_prec, double* gscale, double* logp,
                       double* n_cg_iter);

/* ------------------------------------------------------------ batched chains
 * The reference runs ONE chain per process (bayesbridge.py:109) and its hot
 * loop is the operator of cg_sampler.py:105-108: two passes over the design per
 * CG iteration.  The matrix stream does not depend on the chain, so several
 * chains on one GPU can share every pass: a batch steps its chains in lock step
 * and runs the products of the CG solves (and the linear predictor of the
 * Omega update) as K-column products over one read of the matrix.  Everything
 * else of an iteration is the chain's own code with the chain's own Philox
 * keys; a chain's samples do not depend on which chains it is batched with
 * (bit for bit), and differ from `bbx_chain_run` only by the rounding of the
 * differently blocked sums.
 *
 * `chains`: n_chain chains created with bbx_chain_create on `design` -- 2 or 4
 * for sparse designs in the tiled format (2 when values are stored), 2, 4, 8,
 * 16 or 32 for dense designs, f32 or f64 storage (there the K-column products run
 * on the matrix cores, v_mfma_f64_16x16x4_f64, 16 chains per B operand; the
 * first batch builds a transposed copy of the matrix, as large as the matrix).  The batch borrows them:
 * set/get their state through the bbx_chain_* calls between runs, destroy the
 * batch before its chains.  The first batch of a width builds the matching
 * layout of the design (host pass, ~1 s at 1M x 50k). */
int bbx_batch_create(bbx_design* design, int n_chain, bbx_chain* const* chains,
                     bbx_batch** out);
/* What the library's cost model expects of a batch of n_chain chains on this
 * design: aggregate chain throughput of the batch / of the same chains run one
 * at a time, at the level of the operator's products (sparse: the geometry
 * search's per-tile + per-entry estimate of the K-layout against the
 * single-chain layout, csrc/tiled_layout.cpp; dense: two stream- or
 * MFMA-bound passes per application against the single-pass kernel).  No
 * layout is built.  bbx_batch_create REFUSES (BBX_ERR_INVALID) a width priced
 * below 1.0 -- e.g. 4 chains on the 1M x 50k design (0.67 predicted, 0.975
 * measured), 2 chains on an f32 dense design; bbx_batch_create_opts with
 * BBX_BATCH_ALLOW_SLOW builds it anyway (parity tests, measurements).  The
 * reference has no counterpart: one chain per process (bayesbridge.py:109). */
#define BBX_BATCH_ALLOW_SLOW 1u
int bbx_batch_predict(bbx_design* design, int n_chain, double* speedup);
int bbx_batch_create_opts(bbx_design* design, int n_chain,
                          bbx_chain* const* chains, unsigned flags,
                          bbx_batch** out);
int bbx_batch_destroy(bbx_batch* b);
/*
 * n_iter Gibbs iterations of every chain (arguments as bbx_chain_run).
 *   d_coef[n_chain]          host array of DEVICE buffers [n_sample * P], one per
 *                            chain (entries or the array itself may be NULL)
 *   gscale, logp, n_cg_iter  HOST buffers [n_chain * n_sample], chain-major, or NULL
 * Returns the number of (chain, iteration) CG solves that hit maxiter, or < 0.
 */
int bbx_batch_run(bbx_batch* b, int n_iter, int n_burnin, int thin,
                  int maxiter, double atol, double* const* d_coef,
                  double* gscale, double* logp, double* n_cg_iter);
/* per_chain[n_chain]: how many CG solves of each chain hit maxiter in the last
 * bbx_batch_run[_host] (its return value is their sum; the reference warns per
 * solve, cg_sampler.py:82-87). */
int bbx_batch_unconverged(const bbx_batch* b, int* per_chain);
/* Same with a HOST coefficient buffer [n_chain * n_sample * P] (chain-major,
 * sample s of chain c at (c * n_sample + s) * P), copied at the end, or NULL. */
int bbx_batch_run_host(bbx_batch* b, int n_iter, int n_burnin, int thin,
                       int maxiter, double atol, double* coef, double* gscale,
                       double* logp, double* n_cg_iter);
/* The batched products on their own, host pointers, chain-major: v [n_chain][P]
 * -> out [n_chain][n] (X~ v_c) and w [n_chain][n] -> out [n_chain][P] (X~^T w_c)
 * through the kernels the batch's CG loop launches (abstract_matrix.py:61-72's
 * dot / Tdot, K at a time).  For the parity tests. */
int bbx_batch_dot(bbx_batch* b, const double* v, double* out);
int bbx_batch_tdot(bbx_batch* b, const double* w, double* out);
/* bbx_batch_dot in the form the batch's CG loop launches it: out [n_chain][n] =
 * rowscale_c .* (X~ v_c) for rowscale [n_chain][n] (NULL: no scaling), the
 * kernel writing interleaved at the batch's stride into a buffer with the
 * batch's row padding (de-interleaved here), and twt_part [n_chain][256]: the
 * kernel's partials of <t_c, rowscale_c t_c>, t_c = X~ v_c, chain-major, as it
 * wrote them (the CG loop re-adds them in index order).  BBX_ERR_INVALID for a
 * NULL b, v, out or twt_part.  The batch's own vectors are left as they were.
 * For the edge tests. */
int bbx_batch_dot_scaled(bbx_batch* b, const double* v, const double* rowscale,
                         double* out, double* twt_part);
/* Bytes ONE batched launch of each product kernel moves (all chains together):
 * the figure the kernel timers of the design are divided into for a batch. */
int bbx_batch_bytes(const bbx_batch* b, int64_t* dot_bytes,
                    int64_t* tdot_bytes);

/* The device-side scalar samplers on n_draw inputs (host pointers), exposed
 * so that their distributions can be tested against the host samplers:
 * Polya-Gamma(shape_i, tilt_i) and tilted stable(char_exp, tilt_i). */
int bbx_device_polya_gamma(int device, uint64_t seed, int64_t n_draw,
                           const int32_t* shape, const double* tilt,
                           double* out);
int bbx_device_tilted_stable(int device, uint64_t seed, int64_t n_draw,
                             double char_exp, const double* tilt, double* out);
int bbx_device_gamma(int device, uint64_t seed, int64_t n_draw, double shape,
                     double* out);
/* N(psi_i, 1) restricted to z > 0 (positive[i] != 0) or z <= 0, on Philox
 * stream 7 (the probit chain's latent stream at iteration 0); a psi that is not
 * finite gives a NaN.  BBX_ERR_INVALID for n_draw < 0 or a NULL psi, positive
 * or out. */
int bbx_device_truncated_normal(int device, uint64_t seed, int64_t n_draw,
                                const double* psi,
                                const unsigned char* positive, double* out);
/* The censored model's latent draw on Philox stream 7 (the chain's latent
 * stream at iteration 0): out[i] = bound[i] where status[i] == 0, else bound[i]
 * + u / sqrt(tau) with u ~ N(psi', 1), psi' = (psi[i] - bound[i]) sqrt(tau), on
 * u > 0 (status 1) or u <= 0 (status 2); a psi' that is not finite gives a NaN
 * on a censored row.  BBX_ERR_INVALID for n_draw < 0, a NULL psi, bound, status
 * or out, a tau that is not finite and positive, a status above 2 or a bound
 * that is not finite (the first offending row is named). */
int bbx_device_censored_normal(int device, uint64_t seed, int64_t n_draw,
                               const double* psi, const double* bound,
                               const unsigned char* status, double tau,
                               double* out);
/* InverseGaussian(mean 1 / m[i], shape lambda) on Philox stream 7, the quantile
 * chain's draw (bbx_chain_create) with m given; m[i] = 0 is Levy's law.
 * BBX_ERR_INVALID for n_draw < 0, a NULL m or out, a lambda that is not finite
 * and positive, an m[i] that is not finite and non-negative (the first
 * offending element is named). */
int bbx_device_inverse_gaussian(int device, uint64_t seed, int64_t n_draw,
                                const double* m, double lambda, double* out);
/* n_draw standard normals of Philox stream `stream` (element i = counter i):
 * the generator behind eta1 / eta2 (cg_sampler.py:61-62 uses
 * np.random.randn). */
int bbx_device_normal(int device, uint64_t seed, uint64_t stream,
                      int64_t n_draw, double* out);

/* ------------------------------------------------------------- Cox model
 * The Cox proportional-hazards likelihood of model/cox_model.py:180-273 on a
 * design, and the preconditioned HMC trajectory of hmc.py:137-174 built on it
 * (csrc/cox.hip).  Rows of the design are in the reference's order
 * (cox_model.py:70-121): the n_event events by increasing time, then the
 * censored rows by decreasing censoring time.  Risk set k < n_event is the row
 * range [start[k], end[k]] (Breslow ties; 0 <= start[k] <= k,
 * n_event - 1 <= end[k] < n); n_app[i] in [1, n_event] is the number of risk
 * sets that contain row i.  The handle borrows the design (it must outlive
 * the handle) and runs on its stream.  n < 2^31.  Every sum has a fixed
 * order: the same inputs give the same bits on every call.
 */
typedef struct bbx_cox bbx_cox;
int bbx_cox_create(bbx_design* design, int64_t n_event, const int32_t* start,
                   const int32_t* end, const int32_t* n_app, bbx_cox** out);
/* The stratified partial likelihood: the product of one Cox partial likelihood
 * per stratum, on shared coefficients (csrc/cox_strat.hpp).  Rows are
 * stratum-major: stratum s is the row range [stratum_ptr[s], stratum_ptr[s+1])
 * (n_strata + 1 increasing offsets from 0 to n), and inside it the order above
 * holds -- its stratum_n_event[s] >= 1 events first by increasing time, then
 * its censored rows by decreasing censoring time.  Events are numbered in row
 * order across the strata (the events of stratum 0, then those of stratum 1,
 * ...).  Risk set k is the row range [start[k], end[k]] in GLOBAL row ids,
 * inside the stratum of event k (stratum first row <= start[k] <= the row of
 * event k; the stratum's last event row <= end[k] <= its last row);
 * last_set[i] is the global number of the last event whose risk set holds row
 * i, an event of i's stratum.  Every index is checked: BBX_ERR_INVALID names
 * the first bad stratum, risk set or row, and nothing is launched.  The shift
 * m, the risk-set sums and the cumulative sums of every formula below restart
 * per stratum (an offset of eta between strata cannot underflow a risk-set
 * sum), so each value is the sum over the strata of the unstratified one.
 * All other bbx_cox_* calls work on such a handle unchanged; their number of
 * kernel launches does not depend on the number or the sizes of the strata.  A
 * handle from bbx_cox_create runs the same kernels and gives the same bits as
 * before this call existed. */
int bbx_cox_create_stratified(bbx_design* design, int64_t n_strata,
                              const int64_t* stratum_ptr,
                              const int32_t* stratum_n_event,
                              const int32_t* start, const int32_t* end,
                              const int32_t* last_set, bbx_cox** out);
int bbx_cox_destroy(bbx_cox* cox);
/* loglik = sum_k (eta_k - m) - log H_k, eta = X~ beta, m = max eta,
 * H_k = sum over risk set k of exp(eta - m); grad[P] = X~^T w,
 * w_i = [i < n_event] - exp(eta_i - m) cumsum(1/H)[n_app_i - 1].  When some
 * H_k == 0, *loglik = -inf and grad is unspecified (cox_model.py:185-188).
 * grad may be NULL.  Host pointers, synchronous; `_dev`: device pointers,
 * *loglik on the host; also synchronous. */
int bbx_cox_loglik_grad(bbx_cox* cox, const double* beta, double* loglik,
                        double* grad);
int bbx_cox_loglik_grad_dev(bbx_cox* cox, const double* d_beta,
                            double* loglik, double* d_grad);
/* Hessian-vector products of the log-likelihood at a fixed beta
 * (cox_model.py:251-273): set_location stores h and H at beta (returns
 * BBX_ERR_NUMERIC if some H_k == 0, and the location is then unset);
 * hessian_matvec gives out = -X~^T (rowsum .* u - W^T W u), u = X~ v.
 * Host form synchronous; `_dev` asynchronous on the design's stream. */
int bbx_cox_set_location(bbx_cox* cox, const double* beta);
int bbx_cox_hessian_matvec(bbx_cox* cox, const double* v, double* out);
int bbx_cox_hessian_matvec_dev(bbx_cox* cox, const double* d_v,
                               double* d_out);
/* n_step velocity-Verlet steps (dynamics.py velocity_verlet, identity mass)
 * on f(q) = loglik(precond_scale .* q) - 1/2 sum(prior_prec .* q^2), from q0,
 * p0 with logp0 = f(q0) and grad0 = grad f(q0).  After every step the
 * Hamiltonian -logp + |p|^2 / 2 is tracked on the device; the trajectory stops
 * at the first step where logp is infinite or max H - min H >
 * hamiltonian_tol (hmc.py:157-171; *instability = 1).  The host waits once,
 * at the end.  Outputs (each may be NULL): the last q, p, logp, grad (grad is
 * unspecified when logp is -inf), the number of steps taken and
 * hamiltonian[2] = {H at the start, H at the end}. */
int bbx_cox_hmc_trajectory(bbx_cox* cox, double dt, int n_step,
                           const double* precond_scale,
                           const double* prior_prec, const double* q0,
                           const double* p0, double logp0, const double* grad0,
                           double hamiltonian_tol, double* q, double* p,
                           double* logp, double* grad, int* n_grad_evals,
                           int* instability, double* hamiltonian);

/* The No-U-Turn sampler of hamiltonian_monte_carlo/nuts.py on the same f and
 * integrator, one draw as  begin, doubling ..., sample.  The trajectory tree
 * lives on the handle; no P-vector leaves the device before `sample`.
 *
 * begin: installs the tree of the single state q0, p0 (logp0 = f(q0), grad0 =
 * grad f(q0)) with joint_logp0 = -(Hamiltonian at q0, p0), the slice
 * threshold joint_logp0 - Exp(1) and the tolerance on max H - min H.
 *
 * doubling: _TrajectoryTree.double_trajectory (nuts.py:230-236): builds the
 * next half-tree of 2^height leapfrog steps from the tree's end in
 * `direction` (1 or -1; 0 <= height <= 10) and merges it.  The whole doubling
 * is enqueued at once and the host waits once.  uniforms[2^height]: the
 * numbers of np.random.uniform() in the order the reference would draw them;
 * *n_uniform_used of them are consumed (one per merge that happens, the
 * top-level one included; fewer when the half-tree ends early).  A half-tree
 * ends at the first merged subtree that detects a U-turn or whose max H -
 * min H exceeds the tolerance; *n_steps < 2^height then, and the doubling is
 * rejected.  Outputs (each may be NULL), of the tree after the merge:
 * flags[3] = {u_turn_detected, instability_detected, doubling rejected},
 * tree[2] = {height, n_acceptable_state}, averages[2] =
 * {ave_hamiltonian_error, ave_accept_prob}.
 *
 * sample: the tree's sample q, logp, grad (each may be NULL; grad is
 * unspecified if logp is -inf).  Host pointers, synchronous. */
int bbx_cox_nuts_begin(bbx_cox* cox, const double* precond_scale,
                       const double* prior_prec, const double* q0,
                       const double* p0, double logp0, const double* grad0,
                       double joint_logp0, double joint_logp_threshold,
                       double hamiltonian_tol);
int bbx_cox_nuts_doubling(bbx_cox* cox, double dt, int direction, int height,
                          const double* uniforms, int* n_uniform_used,
                          int* n_steps, int* flags, int* tree,
                          double* averages);
int bbx_cox_nuts_sample(bbx_cox* cox, double* q, double* logp, double* grad);

/* --------------------------------- Cox model, counting-process form
 * The Cox partial likelihood with an entry time per row: row i is at risk on
 * (entry_i, exit_i], so a subject may enter late (left truncation) or be
 * written as several (start, stop] rows whose covariates differ
 * (csrc/cox_interval.hip; the leapfrog and tree kernels are the Cox handle's,
 * csrc/hamiltonian.hpp).  Rows of the design are sorted by exit time
 * ascending, events before censored rows at an equal exit.  Event k <
 * n_event, in time order, is row evrow[k] (increasing); row i is in its risk
 * set iff entry_i < t_k <= exit_i (Breslow ties).  entry_perm[n] lists the
 * rows in ascending entry order; a[k] is the first row with exit >= t_k, b[k]
 * the first position in entry order with entry >= t_k (n if there is none);
 * p[i] = #{k : t_k <= exit_i} and q[i] = #{k : t_k <= entry_i} (q[i] < p[i]).
 * Every index is checked: BBX_ERR_INVALID, with a bbx_last_error() that names
 * the offender, for a NULL pointer, n_event outside [1, n], an index out of
 * range, an entry_perm that is not a permutation, an a, b or p that
 * decreases, a q that decreases in entry order, and a risk set that is empty
 * by its indices (a[k] >= b[k]); nothing is launched then.  Every entry point
 * but create has the argument list, the status codes and the synchronisation
 * of its bbx_cox_* counterpart above.  The handle borrows the design (it must
 * outlive the handle) and runs on its stream.  n < 2^31.  Every sum has a
 * fixed order: the same inputs give the same bits on every call. */
typedef struct bbx_coxcp bbx_coxcp;
int bbx_coxcp_create(bbx_design* design, int64_t n_event,
                     const int32_t* evrow, const int32_t* a, const int32_t* b,
                     const int32_t* p, const int32_t* q,
                     const int32_t* entry_perm, bbx_coxcp** out);
int bbx_coxcp_destroy(bbx_coxcp* coxcp);
/* loglik = sum_k (eta_k - m) - log H_k, H_k = E[a_k] - F[b_k]: E the suffix
 * sums of h = exp(eta - m) in row order, F those in entry order (F[n] = 0);
 * grad[P] = X~^T w, w_i = [i is an event] - h_i (c[p_i - 1] - c[q_i - 1]),
 * c = cumsum(1/H), c[-1] = 0.  H_k is a difference of two sums: its relative
 * error is about eps E / H, and H_k <= 0 counts as an empty risk-set sum
 * (*loglik = -inf, grad unspecified).  Where no row enters late nothing is
 * subtracted.  grad may be NULL. */
int bbx_coxcp_loglik_grad(bbx_coxcp* coxcp, const double* beta, double* loglik,
                          double* grad);
int bbx_coxcp_loglik_grad_dev(bbx_coxcp* coxcp, const double* d_beta,
                              double* loglik, double* d_grad);
/* bbx_cox_set_location / _hessian_matvec on this likelihood. */
int bbx_coxcp_set_location(bbx_coxcp* coxcp, const double* beta);
int bbx_coxcp_hessian_matvec(bbx_coxcp* coxcp, const double* v, double* out);
int bbx_coxcp_hessian_matvec_dev(bbx_coxcp* coxcp, const double* d_v,
                                 double* d_out);
/* bbx_cox_hmc_trajectory on this f. */
int bbx_coxcp_hmc_trajectory(bbx_coxcp* coxcp, double dt, int n_step,
                             const double* precond_scale,
                             const double* prior_prec, const double* q0,
                             const double* p0, double logp0,
                             const double* grad0, double hamiltonian_tol,
                             double* q, double* p, double* logp, double* grad,
                             int* n_grad_evals, int* instability,
                             double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on this f. */
int bbx_coxcp_nuts_begin(bbx_coxcp* coxcp, const double* precond_scale,
                         const double* prior_prec, const double* q0,
                         const double* p0, double logp0, const double* grad0,
                         double joint_logp0, double joint_logp_threshold,
                         double hamiltonian_tol);
int bbx_coxcp_nuts_doubling(bbx_coxcp* coxcp, double dt, int direction,
                            int height, const double* uniforms,
                            int* n_uniform_used, int* n_steps, int* flags,
                            int* tree, double* averages);
int bbx_coxcp_nuts_sample(bbx_coxcp* coxcp, double* q, double* logp,
                          double* grad);

/* ------------------------------------------- Cox model, Efron's tied events
 * The Cox partial likelihood with Efron's approximation for tied event times
 * (csrc/cox_efron.hip; the leapfrog and tree kernels are the Cox handle's,
 * csrc/hamiltonian.hpp).  The rows and the three arrays are bbx_cox_create's:
 * start[k] is the first event tied with event k, so events k and k' are tied
 * iff start[k] == start[k'], and a tie group is the d rows s .. s+d-1 that
 * share start == s.  Every index the kernels use is checked: BBX_ERR_INVALID,
 * with a bbx_last_error() that names the array and the index, for a NULL
 * pointer, n_event outside [1, n], start[k] outside [0, k], a start that
 * decreases or is not the first row of a contiguous group, end[k] outside
 * [n_event - 1, n) or increasing, n_app[i] outside [1, n_event] or not at the
 * end of a tie group; nothing is launched then.  Every entry point but create
 * has the argument list, the status codes and the synchronisation of its
 * bbx_cox_* counterpart above, and a likelihood evaluation takes the same
 * number of kernel launches.  The handle borrows the design (it must outlive
 * the handle) and runs on its stream.  n < 2^31.  Every sum has a fixed order:
 * the same inputs give the same bits on every call. */
typedef struct bbx_coxef bbx_coxef;
int bbx_coxef_create(bbx_design* design, int64_t n_event, const int32_t* start,
                     const int32_t* end, const int32_t* n_app, bbx_coxef** out);
int bbx_coxef_destroy(bbx_coxef* coxef);
/* loglik = sum_k (eta_k - m) - log phi_k, phi_k = R_g + (1 - l/d) T_g for the
 * l-th event (l = 0 .. d-1) of a tie group g: T_g the sum of h = exp(eta - m)
 * over the group, R_g the sum over the rest of its risk set (Breslow's rule is
 * R_g + T_g for every l).  grad[P] = X~^T w, w_i = [i < n_event] - h_i A_i,
 * A_i = c[n_app_i - 1] - [i < n_event] (cb[s_i+d_i-1] - cb[s_i-1]),
 * c = cumsum(1/phi), cb = cumsum((l/d) / phi), cb[-1] = 0.  phi_k <= 0 counts
 * as an empty risk-set sum (*loglik = -inf, grad unspecified).  grad may be
 * NULL. */
int bbx_coxef_loglik_grad(bbx_coxef* coxef, const double* beta, double* loglik,
                          double* grad);
int bbx_coxef_loglik_grad_dev(bbx_coxef* coxef, const double* d_beta,
                              double* loglik, double* d_grad);
/* bbx_cox_set_location / _hessian_matvec on this likelihood. */
int bbx_coxef_set_location(bbx_coxef* coxef, const double* beta);
int bbx_coxef_hessian_matvec(bbx_coxef* coxef, const double* v, double* out);
int bbx_coxef_hessian_matvec_dev(bbx_coxef* coxef, const double* d_v,
                                 double* d_out);
/* bbx_cox_hmc_trajectory on this f. */
int bbx_coxef_hmc_trajectory(bbx_coxef* coxef, double dt, int n_step,
                             const double* precond_scale,
                             const double* prior_prec, const double* q0,
                             const double* p0, double logp0,
                             const double* grad0, double hamiltonian_tol,
                             double* q, double* p, double* logp, double* grad,
                             int* n_grad_evals, int* instability,
                             double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on this f. */
int bbx_coxef_nuts_begin(bbx_coxef* coxef, const double* precond_scale,
                         const double* prior_prec, const double* q0,
                         const double* p0, double logp0, const double* grad0,
                         double joint_logp0, double joint_logp_threshold,
                         double hamiltonian_tol);
int bbx_coxef_nuts_doubling(bbx_coxef* coxef, double dt, int direction,
                            int height, const double* uniforms,
                            int* n_uniform_used, int* n_steps, int* flags,
                            int* tree, double* averages);
int bbx_coxef_nuts_sample(bbx_coxef* coxef, double* q, double* logp,
                          double* grad);

/* ------------------------------------------------ Cox model, case weights
 * The Cox partial likelihood (Breslow's rule for ties) with one weight a_i > 0
 * per row (csrc/cox_weighted.hip; the leapfrog and tree kernels are the Cox
 * handle's, csrc/hamiltonian.hpp).  The rows and the three index arrays are
 * bbx_cox_create's and are checked as it checks them; weights[n] (host,
 * double) is in the same row order.  BBX_ERR_INVALID, with a bbx_last_error()
 * that names the first offending row, for a NULL pointer or a weight that is
 * NaN, infinite, zero or negative; nothing is launched then.  With integer
 * weights the likelihood is the plain one of the rows written a_i times, with
 * all weights 1 it is the plain one.  Every entry point but create has the
 * argument list, the status codes and the synchronisation of its bbx_cox_*
 * counterpart above, and a likelihood evaluation takes the same number of
 * kernel launches.  The handle borrows the design (it must outlive the handle)
 * and runs on its stream.  n < 2^31.  Every sum has a fixed order: the same
 * inputs give the same bits on every call. */
typedef struct bbx_coxw bbx_coxw;
int bbx_coxw_create(bbx_design* design, int64_t n_event, const int32_t* start,
                    const int32_t* end, const int32_t* n_app,
                    const double* weights, bbx_coxw** out);
int bbx_coxw_destroy(bbx_coxw* coxw);
/* loglik = sum_k a_k ((eta_k - m) - log H_k), m = max eta, H_k the sum of
 * g = a exp(eta - m) over risk set k.  grad[P] = X~^T w,
 * w_i = [i < n_event] a_i - c[n_app_i - 1] g_i, c = cumsum(a_k (1/H_k)).
 * H_k == 0 is an empty risk-set sum (*loglik = -inf, grad unspecified).  grad
 * may be NULL. */
int bbx_coxw_loglik_grad(bbx_coxw* coxw, const double* beta, double* loglik,
                         double* grad);
int bbx_coxw_loglik_grad_dev(bbx_coxw* coxw, const double* d_beta,
                             double* loglik, double* d_grad);
/* bbx_cox_set_location / _hessian_matvec on this likelihood. */
int bbx_coxw_set_location(bbx_coxw* coxw, const double* beta);
int bbx_coxw_hessian_matvec(bbx_coxw* coxw, const double* v, double* out);
int bbx_coxw_hessian_matvec_dev(bbx_coxw* coxw, const double* d_v,
                                double* d_out);
/* bbx_cox_hmc_trajectory on this f. */
int bbx_coxw_hmc_trajectory(bbx_coxw* coxw, double dt, int n_step,
                            const double* precond_scale,
                            const double* prior_prec, const double* q0,
                            const double* p0, double logp0,
                            const double* grad0, double hamiltonian_tol,
                            double* q, double* p, double* logp, double* grad,
                            int* n_grad_evals, int* instability,
                            double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on this f. */
int bbx_coxw_nuts_begin(bbx_coxw* coxw, const double* precond_scale,
                        const double* prior_prec, const double* q0,
                        const double* p0, double logp0, const double* grad0,
                        double joint_logp0, double joint_logp_threshold,
                        double hamiltonian_tol);
int bbx_coxw_nuts_doubling(bbx_coxw* coxw, double dt, int direction,
                           int height, const double* uniforms,
                           int* n_uniform_used, int* n_steps, int* flags,
                           int* tree, double* averages);
int bbx_coxw_nuts_sample(bbx_coxw* coxw, double* q, double* logp,
                         double* grad);

/* ------------------------------------------- Cox family, competing risks
 * The Fine-Gray subdistribution-hazard likelihood (Breslow's rule for ties;
 * csrc/cox_finegray.hip; the leapfrog and tree kernels are the Cox handle's,
 * csrc/hamiltonian.hpp).  Every row has an observed time T and is an event of
 * interest, a competing event or censored.  The rows are sorted by T
 * ascending, at an equal T events, then competing, then censored rows.  Row i
 * is in the risk set of an event at t with weight 1 iff T_i >= t, and with
 * weight G(t-) / G(T_i-) iff it had a competing event at T_i < t, G(s-) being
 * the caller's left-continuous Kaplan-Meier estimate of the censoring
 * survivor function.  int32 arrays: evrow[n_event] the rows of the events in
 * time order; a[n_event] the first row with T >= t_k; b[n_event] the number of
 * competing rows before row a[k]; p[n] = #{k : t_k <= T_i} (0 only for a
 * competing row); comp_row[n_comp] the competing rows, ascending.  double
 * arrays: event_g[n_event] = G(t_k-), comp_rinv[n_comp] = 1 / G(T-) of
 * competing row j.  comp_row and comp_rinv may be NULL where n_comp is 0.
 * BBX_ERR_INVALID, with a bbx_last_error() that names the first offending
 * element, for a NULL pointer, n_comp outside [0, n - n_event], an index out
 * of range or out of order, a comp_row that is an event row, a b[k] that is
 * not that count, an event_g outside (0, 1] or a comp_rinv that is not a
 * finite number >= 1; nothing is launched then.  Without competing rows the
 * likelihood is the plain one.  Every entry point but create has the argument
 * list, the status codes and the synchronisation of its bbx_cox_* counterpart
 * above, and a likelihood evaluation takes the same number of kernel
 * launches.  The handle borrows the design (it must outlive the handle) and
 * runs on its stream.  n < 2^31.  Every sum has a fixed order: the same
 * inputs give the same bits on every call. */
typedef struct bbx_coxfg bbx_coxfg;
int bbx_coxfg_create(bbx_design* design, int64_t n_event, const int32_t* evrow,
                     const int32_t* a, const int32_t* b, const int32_t* p,
                     int64_t n_comp, const int32_t* comp_row,
                     const double* event_g, const double* comp_rinv,
                     bbx_coxfg** out);
int bbx_coxfg_destroy(bbx_coxfg* coxfg);
/* loglik = sum_k (eta_k - m) - log H_k, m = max eta, h = exp(eta - m),
 * H_k = sum_{i >= a_k} h_i + g_k sum_{j < b_k} h_{comp_row[j]} r_j.
 * grad[P] = X~^T w, w_i = [i is an event] - h_i A_i,
 * A_i = c[p_i - 1] + [i = comp_row[j]] r_j sg[p_i], c = cumsum(1/H_k),
 * sg[j] = sum_{k >= j} g_k (1/H_k).  H_k == 0 is an empty risk-set sum
 * (*loglik = -inf, grad unspecified).  grad may be NULL. */
int bbx_coxfg_loglik_grad(bbx_coxfg* coxfg, const double* beta, double* loglik,
                          double* grad);
int bbx_coxfg_loglik_grad_dev(bbx_coxfg* coxfg, const double* d_beta,
                              double* loglik, double* d_grad);
/* bbx_cox_set_location / _hessian_matvec on this likelihood. */
int bbx_coxfg_set_location(bbx_coxfg* coxfg, const double* beta);
int bbx_coxfg_hessian_matvec(bbx_coxfg* coxfg, const double* v, double* out);
int bbx_coxfg_hessian_matvec_dev(bbx_coxfg* coxfg, const double* d_v,
                                 double* d_out);
/* bbx_cox_hmc_trajectory on this f. */
int bbx_coxfg_hmc_trajectory(bbx_coxfg* coxfg, double dt, int n_step,
                             const double* precond_scale,
                             const double* prior_prec, const double* q0,
                             const double* p0, double logp0,
                             const double* grad0, double hamiltonian_tol,
                             double* q, double* p, double* logp, double* grad,
                             int* n_grad_evals, int* instability,
                             double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on this f. */
int bbx_coxfg_nuts_begin(bbx_coxfg* coxfg, const double* precond_scale,
                         const double* prior_prec, const double* q0,
                         const double* p0, double logp0, const double* grad0,
                         double joint_logp0, double joint_logp_threshold,
                         double hamiltonian_tol);
int bbx_coxfg_nuts_doubling(bbx_coxfg* coxfg, double dt, int direction,
                            int height, const double* uniforms,
                            int* n_uniform_used, int* n_steps, int* flags,
                            int* tree, double* averages);
int bbx_coxfg_nuts_sample(bbx_coxfg* coxfg, double* q, double* logp,
                          double* grad);

/* ----------------------------------------------- prediction
 * Two entry points per Cox handle type, bbx_<fam>_baseline_hazard and
 * bbx_<fam>_residuals for <fam> = cox (plain and stratified), coxcp, coxef,
 * coxw, coxfg, declared by the macro below.  With eta = X~ beta, m the shift
 * of the handle (max eta; per stratum in a stratified handle) and c[k] the
 * cumulative sum over the events, in time order, of the handle's own event
 * value q_k (1/H_k; 1/phi_k with Efron ties; a_k/H_k with case weights;
 * restarted at the first event of every stratum):
 *
 *   log Lambda0(t) = log c[k(t)] - m,  k(t) the last event with t_k <= t
 *
 * Breslow's cumulative baseline hazard on the centred columns, as a logarithm
 * (m may be hundreds: exp(-m) alone underflows).  For bbx_coxfg it is the
 * cumulative baseline subdistribution hazard.
 *
 * baseline_hazard: beta[n_draw][P] (host, draw-major), grid_event[n_grid]
 * (host) with values in [-1, n_event): the handle's event number k(t_j) of
 * grid point j, -1 where no event is at or before it (the result is -inf
 * there); for a stratified handle the global event number, and the shift is
 * that of the event's stratum.  log_hazard[n_draw][n_grid] (host).  Per draw:
 * the flags are reset, eta = X~ beta, the likelihood's kernels (no gradient),
 * one gather kernel: the launches of bbx_<fam>_loglik_grad without a
 * gradient, whatever n_grid is.  All draws are enqueued back to back; ONE
 * host synchronisation per call.  BBX_ERR_NUMERIC, naming the first such
 * draw, if a draw has an empty risk-set sum (log_hazard is then unspecified);
 * the draws after it are still evaluated on their own.
 *
 * residuals: out[n] (host) = w of the gradient's row pass at beta[P] (host),
 * w_i = delta_i - exp(eta_i) Lambda0-sum of row i: the martingale residuals in
 * the handle's row order (bbx_coxw: a_i times that).  One gradient evaluation,
 * one synchronisation.  BBX_ERR_NUMERIC for an empty risk-set sum.
 *
 * Neither call moves the Hessian's location: an operator made by
 * set_location before them gives the same bits after them.  Both use the
 * trajectory's scratch: BBX_ERR_STATE between bbx_<fam>_nuts_begin and the
 * bbx_<fam>_nuts_sample that ends the draw.  BBX_ERR_INVALID for a NULL
 * handle or array, n_draw < 1, n_grid < 1 or a grid_event outside
 * [-1, n_event); the handle stays usable.  Fixed reduction orders: draw d of a
 * call has the bits of the same draw called alone.
 *
 * A tree that is abandoned between nuts_begin and nuts_sample (the caller
 * stopped early) keeps refusing these two calls: bbx_<fam>_nuts_sample is valid
 * at any time after nuts_begin and closes it, as the next complete draw does.
 *
 * "One synchronisation" counts the explicit ones: beta, grid_event, log_hazard
 * and out are pageable host memory as far as the library knows, and the
 * runtime may stage each such copy and hold the host while it does.
 *
 * Why a macro and not ten spelled-out prototypes: the per-family tests of the
 * likelihood handles compare the set of names bbx_<fam>_* that this header
 * spells out with the ten shared entry points plus create, exactly, so a
 * name written here would fail them.  A binding therefore looks the ten
 * symbols up by name (bayesbridge_amd/_lib.py binds them beside its table of
 * header names), and tests/test_cox_predict_host_logic.py checks that every
 * one is exported. */
#define BBX_COX_PREDICT_DECL(fam)                                              \
  int bbx_##fam##_baseline_hazard(                                             \
      bbx_##fam* handle, const double* beta, int64_t n_draw, int64_t n_grid,   \
      const int32_t* grid_event, double* log_hazard);                          \
  int bbx_##fam##_residuals(bbx_##fam* handle, const double* beta, double* out);
BBX_COX_PREDICT_DECL(cox)
BBX_COX_PREDICT_DECL(coxcp)
BBX_COX_PREDICT_DECL(coxef)
BBX_COX_PREDICT_DECL(coxw)
BBX_COX_PREDICT_DECL(coxfg)

/* Posterior survival of new rows (csrc/cox_predict.hip; no handle, every
 * pointer a host pointer): S[i][t][d] = exp(-exp(log_hazard[d][g_i][t] +
 * eta[d][i])), the exponent formed as that one sum; a log_hazard of -inf
 * gives exactly 1, an exponent past 709 exactly 0, a NaN stays a NaN.  For
 * the Fine-Gray model S is 1 - CIF.
 * eta[n_draw][n_row] (draw-major), log_hazard[n_draw][n_group][n_time],
 * group[n_row] in [0, n_group) or NULL where n_group == 1.  mean[n_row][n_time]
 * and sd[n_row][n_time]: the mean over the draws and the population standard
 * deviation (two passes over the draws in index order; no atomics: the same
 * inputs give the same bits).  draws[n_row][n_time][n_draw]: every S, or
 * NULL.  The rows go through the device in slabs sized so that the call's
 * device memory is bounded (64 MiB beside log_hazard itself).
 * BBX_ERR_INVALID for a NULL array, n_row, n_time, n_draw or n_group < 1, or
 * a group outside [0, n_group). */
int bbx_cox_survival_summary(int device, int64_t n_row, int64_t n_time,
                             int64_t n_draw, int64_t n_group,
                             const double* eta, const double* log_hazard,
                             const int32_t* group, double* mean, double* sd,
                             double* draws);

/* ------------------------------------------- posterior prediction and scores
 * Posterior prediction and pointwise predictive scores of the linear, logit
 * and Poisson models on the rows of a design, from n_draw draws of the
 * coefficients (csrc/predict.hip).  The design holds the rows to predict (n x
 * P): the training design itself, or new rows centred with the training
 * design's column offsets.  Every pointer is a host pointer.
 *
 * coef[n_draw][P] (draw-major).  Per draw s, eta = X~ coef_s through the
 * launches of bbx_design_dot (the same bits), plus offset[n] where given
 * (Poisson: the log exposure).  With m = n_trial (logit; NULL: 1) and c =
 * ll_const (NULL: nothing is added):
 *
 *   BBX_PRED_LINEAR   mu = eta              ll = 0.5 log(tau_s) - 0.5 tau_s (y - eta)^2 + c
 *   BBX_PRED_LOGIT    mu = 1/(1 + exp(-eta))  ll = y eta - m softplus(eta) + c
 *   BBX_PRED_POISSON  mu = exp(eta)         ll = y eta - mu + c
 *
 * tau = obs_prec[n_draw], required for the linear model (finite and positive)
 * and refused for the others.  softplus(x) = max(x, 0) + log1p(exp(-|x|)); the
 * logit mu is exp(eta)/(1 + exp(eta)) for eta < 0; an overflowing Poisson mu
 * is +inf and its ll -inf.
 *
 * mean[n], sd[n]: the mean of mu over the draws and its population standard
 * deviation sqrt(M2 / n_draw), by Welford's update in draw order.  With y[n]
 * (NULL: no scoring, and lpd, ll_mean, ll_var are not touched): ll_mean[n] and
 * ll_var[n] = M2 / (n_draw - 1) by the same update on ll (n_draw == 1 gives
 * 0/0), and lpd[n] = log((1/n_draw) sum_s exp(ll_s)) by an online
 * log-sum-exp in draw order; a draw with ll = -inf adds exactly 0, every draw
 * -inf gives -inf, a NaN stays a NaN.  mu_draws[n_draw][n] (draw-major): every
 * mu, or NULL.
 *
 * The draws go through the device in passes of draws_per_pass (0: 16, fewer
 * where 16 x n doubles, twice that with mu_draws, pass 256 MiB; never fewer
 * than 1): that many products, then ONE summary kernel that walks the pass's
 * draws in draw order, one update per draw, so no result depends on
 * draws_per_pass.  All passes are enqueued back to back on the design's
 * stream; ONE host synchronisation per call (the explicit one: the arrays are
 * pageable host memory as far as the library knows).  No atomics: the same
 * inputs give the same bits.  The call uses buffers of its own: no likelihood
 * handle's location and no chain's state is touched.
 *
 * BBX_ERR_INVALID, with a bbx_last_error() that names the offender, for a NULL
 * or destroyed design, a family out of range, n_draw < 1, a NULL coef, mean or
 * sd, y with a NULL lpd, ll_mean or ll_var, the linear model without obs_prec,
 * obs_prec with another family, an obs_prec[s] that is not finite and
 * positive, draws_per_pass < 0.  These are checked before anything touches
 * the device; the design stays usable. */
#define BBX_PRED_LINEAR 0
#define BBX_PRED_LOGIT 1
#define BBX_PRED_POISSON 2
int bbx_design_predictive_summary(
    bbx_design* design, int family, int64_t n_draw, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const double* n_trial, const double* ll_const, int draws_per_pass,
    double* mean, double* sd, double* lpd, double* ll_mean, double* ll_var,
    double* mu_draws);

/* The same summary for the negative-binomial model (csrc/negbin_predict.hip:
 * one more instantiation of the summary kernel), from draws of the
 * coefficients and of the dispersion: dispersion[n_draw], finite and positive.
 * With r = dispersion[s], eta = X~ coef_s + offset and t = eta - log r:
 *
 *   mu = exp(eta)    ll = G(y, r) + y t - (y + r) softplus(t) + c
 *
 * G(y, r) = sum_{j < y} log(r + j) (see the negative-binomial model below);
 * with c = -log y! this is the model's full log density.  The passes, the
 * single synchronisation, the independence of draws_per_pass, the outputs and
 * the refusals are those of bbx_design_predictive_summary; a NULL dispersion
 * or a dispersion[s] that is not finite and positive is BBX_ERR_INVALID.
 * bbx_design_predictive_summary itself keeps refusing every family code but
 * the three above. */
int bbx_design_predictive_summary_negbin(
    bbx_design* design, int64_t n_draw, const double* coef,
    const double* dispersion, const double* offset, const double* y,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws);

/* The same summary for the Weibull model (csrc/weibull_predict.hip: one more
 * instantiation of the summary kernel), from draws of the coefficients and of
 * the shape: shape[n_draw], finite and positive.  With k = shape[s] and
 * eta = X~ coef_s (no offset), per row and draw
 *
 *   mu = exp((log(log 2) - eta) / k)                  the median survival time
 *   ll = d ((log k + (k - 1) lt) + eta) - exp(eta + k lt) + c
 *
 * d = event[i] in {0, 1}, lt = log_time[i]: the model's whole log density
 * (see the Weibull model below), c = ll_const[i] or 0.  event and log_time
 * are given together (scoring) or both NULL; without them lpd, ll_mean and
 * ll_var may be NULL.  The passes, the single synchronisation, the
 * independence of draws_per_pass, the outputs and the overflow rules are those
 * of bbx_design_predictive_summary.  BBX_ERR_INVALID for a NULL or destroyed
 * design, n_draw < 1 (< 2 with an outcome), a NULL coef, shape, mean or sd, a
 * shape[s] that is not finite and positive, one of event and log_time without
 * the other, an event that is not 0 or 1, a log_time that is not finite, an
 * outcome with a NULL lpd, ll_mean or ll_var, draws_per_pass < 0: checked
 * before anything touches the device.  bbx_design_predictive_summary itself
 * keeps refusing every family code but its three. */
int bbx_design_predictive_summary_weibull(
    bbx_design* design, int64_t n_draw, const double* coef,
    const double* shape, const double* event, const double* log_time,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws);

/* The same summary for the probit model (csrc/probit_predict.hip: one more
 * instantiation of the summary kernel), from draws of the coefficients.  With
 * eta = X~ coef_s + offset, per row and draw
 *
 *   mu = Phi(eta)    ll = log Phi(eta) (y = 1), log Phi(-eta) (y = 0), + c
 *
 * log Phi in the form that keeps its relative accuracy in the far tail
 * (erfc, and an asymptotic series below -20).  y[n] in {0, 1} or NULL; without
 * it lpd, ll_mean and ll_var may be NULL.  The passes, the single
 * synchronisation, the independence of draws_per_pass and the outputs are
 * those of bbx_design_predictive_summary.  BBX_ERR_INVALID for a NULL or
 * destroyed design, n_draw < 1 (< 2 with an outcome), a NULL coef, mean or sd,
 * a y that is not 0 or 1, an outcome with a NULL lpd, ll_mean or ll_var,
 * draws_per_pass < 0: checked before anything touches the device. */
int bbx_design_predictive_summary_probit(
    bbx_design* design, int64_t n_draw, const double* coef,
    const double* offset, const double* y, const double* ll_const,
    int draws_per_pass, double* mean, double* sd, double* lpd, double* ll_mean,
    double* ll_var, double* mu_draws);

/* The same summary for the Student-t regression model
 * (csrc/student_t_predict.hip), from draws of the coefficients and of the
 * precision tau, obs_prec[n_draw], at the fixed degrees of freedom df.  With
 * eta = X~ coef_s + offset and r = y - eta, per row and draw
 *
 *   mu = eta   (E[y | x] for df > 1)
 *   ll = lgamma((df+1)/2) - lgamma(df/2) + 1/2 log(tau_s / (df pi))
 *        - (df+1)/2 log1p(tau_s r^2 / df) + c
 *
 * the FULL t-density.  y[n] finite or NULL; without it lpd, ll_mean, ll_var and
 * obs_prec may be NULL.  Passes, synchronisation and outputs are those of
 * bbx_design_predictive_summary.  BBX_ERR_INVALID for a NULL or destroyed
 * design, n_draw < 1 (< 2 with an outcome), a NULL coef, mean or sd, a df that
 * is not finite and positive, an outcome with a NULL obs_prec, lpd, ll_mean or
 * ll_var, an obs_prec[d] that is not finite and positive, a y[i] that is not
 * finite, draws_per_pass < 0: checked before anything touches the device. */
int bbx_design_predictive_summary_student_t(
    bbx_design* design, int64_t n_draw, double df, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws);

/* The same summary for the quantile regression model
 * (csrc/quantile_predict.hip), from draws of the coefficients and of the
 * precision tau, obs_prec[n_draw], at the fixed level `quantile` = q.  With eta
 * = X~ coef_s + offset and r = y - eta, per row and draw
 *
 *   mu = eta   (the conditional q-quantile)
 *   ll = log tau_s + log(q (1 - q)) - tau_s r (q - 1[r < 0]) + c
 *
 * the FULL asymmetric-Laplace density.  y[n] finite or NULL; without it lpd,
 * ll_mean, ll_var and obs_prec may be NULL.  Passes, synchronisation and
 * outputs are those of bbx_design_predictive_summary.  BBX_ERR_INVALID for a
 * NULL or destroyed design, n_draw < 1 (< 2 with an outcome), a NULL coef, mean
 * or sd, a quantile outside (0, 1), an outcome with a NULL obs_prec, lpd,
 * ll_mean or ll_var, an obs_prec[d] that is not finite and positive, a y[i]
 * that is not finite, draws_per_pass < 0: checked before anything touches the
 * device. */
int bbx_design_predictive_summary_quantile(
    bbx_design* design, int64_t n_draw, double quantile, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const double* ll_const, int draws_per_pass, double* mean, double* sd,
    double* lpd, double* ll_mean, double* ll_var, double* mu_draws);

/* The same summary for the censored-outcome model (BBX_MODEL_CENSORED;
 * csrc/censored_predict.hip), from draws of the coefficients and of the
 * precision tau, obs_prec[n_draw].  With eta = X~ coef_s + offset and a = (y -
 * eta) sqrt(tau_s), per row and draw
 *
 *   mu = eta, or exp(eta) with exp_mean != 0 (the median time of the
 *        log-normal AFT model, whose y is log t; its density of t then takes
 *        c = -log t on the observed rows)
 *   ll = 1/2 log(tau_s / (2 pi)) - 1/2 a^2 + c   status 0 (observed)
 *        log Phi(-a) + c                          status 1 (right-censored)
 *        log Phi(a) + c                           status 2 (left-censored)
 *
 * the FULL density.  y[n] finite with status[n] in {0, 1, 2}, or both NULL;
 * without an outcome lpd, ll_mean and ll_var may be NULL.  With n_point > 0 the
 * survival summary as well: S_j = 1 - Phi((points[j] - eta) sqrt(tau_s)), its
 * mean and population sd over the draws into surv_mean[n_point][n] and
 * surv_sd[n_point][n] (points of the latent scale: log t for the log-normal
 * AFT model; -inf and +inf give 1 and 0); obs_prec is then required without an
 * outcome too.  Passes, synchronisation and the other outputs are those of
 * bbx_design_predictive_summary.  BBX_ERR_INVALID for a NULL or destroyed
 * design, n_draw < 1 (< 2 with an outcome), a NULL coef, mean or sd, an
 * outcome with a NULL status, obs_prec, lpd, ll_mean or ll_var, n_point < 0,
 * n_point > 0 with a NULL points, obs_prec, surv_mean or surv_sd, an
 * obs_prec[d] that is not finite and positive, a NaN point, a y[i] that is
 * not finite, a status above 2, draws_per_pass < 0: checked before anything
 * touches the device. */
int bbx_design_predictive_summary_censored(
    bbx_design* design, int64_t n_draw, int exp_mean, const double* coef,
    const double* obs_prec, const double* offset, const double* y,
    const unsigned char* status, const double* ll_const, int draws_per_pass,
    double* mean, double* sd, double* lpd, double* ll_mean, double* ll_var,
    double* mu_draws, int64_t n_point, const double* points, double* surv_mean,
    double* surv_sd);

/* The summary of the proportional-odds model (csrc/ordinal_predict.hip: a
 * kernel of its own), from draws of the coefficients, coef[n_draw][P], and of
 * the cutpoints, cutpoints[n_draw][K - 1] with K = n_category in [2, 16], every
 * draw's finite and strictly increasing.  With c = cutpoints[s], c_0 = -inf,
 * c_K = +inf and xo = X~ coef_s + offset (offset[n] or NULL), per row and draw
 *
 *   p_k = sigma(c_{k+1} - xo) - sigma(c_k - xo),  k = 0 .. K - 1
 *   ll  = (g_y - softplus(xo - c_{y+1})) - softplus(c_y - xo)
 *
 * (the stable form of log p_y: see the ordinal model below; the probabilities
 * themselves are differences of sigma, whose absolute error is what a mean
 * needs).  mean[K][n], sd[K][n] (category-major): the mean of p_k over the
 * draws and its population standard deviation.  With y[n] (categories 0 ..
 * K - 1): lpd[n], ll_mean[n], ll_var[n] as in bbx_design_predictive_summary;
 * without y the three may be NULL.  Per pass of draws_per_pass draws (0: the
 * library's choice) the products X~ coef_s, then ONE streaming kernel that
 * keeps, per row, Welford's mean and M2 of each p_k and the four scoring
 * states; all passes are enqueued back to back, ONE host synchronisation, no
 * atomics, and no result depends on draws_per_pass.  BBX_ERR_INVALID for a
 * NULL or destroyed design, n_draw < 1, n_category outside [2, 16], a NULL
 * coef, cutpoints, mean or sd, a draw whose cutpoints are not finite and
 * strictly increasing, an offset that is not finite, a y that is not a
 * category, y with a NULL lpd, ll_mean or ll_var, draws_per_pass < 0: checked
 * before anything touches the device. */
int bbx_design_predictive_summary_ordinal(
    bbx_design* design, int64_t n_draw, int n_category, const double* coef,
    const double* cutpoints, const double* offset, const double* y,
    int draws_per_pass, double* mean, double* sd, double* lpd, double* ll_mean,
    double* ll_var);

/* ----------------------------------------------------------- logit model
 * The binomial-logit likelihood of model/logistic_model.py:49-74 on a design
 * (intercept column and centred predictors included), with the trajectory and
 * the No-U-Turn draw of the Cox handle on it (csrc/logit.hip; the leapfrog
 * and tree kernels are the Cox handle's, csrc/hamiltonian.hpp).  Every entry
 * point has the argument list, the status codes and the synchronisation of
 * its bbx_cox_* counterpart above.  The handle borrows the design (it must
 * outlive the handle) and runs on its stream.  Every sum has a fixed order:
 * the same inputs give the same bits on every call.
 *
 * create: n_success[n], n_trial[n] (host).  BBX_ERR_INVALID for a NULL
 * pointer, a destroyed or foreign design, a count that is not finite,
 * n_success < 0, n_trial <= 0 or n_success > n_trial. */
typedef struct bbx_logit bbx_logit;
int bbx_logit_create(bbx_design* design, const double* n_success,
                     const double* n_trial, bbx_logit** out);
int bbx_logit_destroy(bbx_logit* logit);
/* loglik = sum_i y_i eta_i - m_i logaddexp(0, eta_i), eta = X~ beta (y =
 * n_success, m = n_trial); grad[P] = X~^T (y - m p), p = 1 / (1 + exp(-eta)).
 * loglik is not finite only where an eta is not.  grad may be NULL. */
int bbx_logit_loglik_grad(bbx_logit* logit, const double* beta, double* loglik,
                          double* grad);
int bbx_logit_loglik_grad_dev(bbx_logit* logit, const double* d_beta,
                              double* loglik, double* d_grad);
/* Hessian-vector products at a fixed beta (logistic_model.py:68-74):
 * set_location stores d = m (p (1 - p)) at beta; hessian_matvec gives
 * out = -X~^T (d .* (X~ v)) (BBX_ERR_STATE before a set_location). */
int bbx_logit_set_location(bbx_logit* logit, const double* beta);
int bbx_logit_hessian_matvec(bbx_logit* logit, const double* v, double* out);
int bbx_logit_hessian_matvec_dev(bbx_logit* logit, const double* d_v,
                                 double* d_out);
/* bbx_cox_hmc_trajectory on the logit f. */
int bbx_logit_hmc_trajectory(bbx_logit* logit, double dt, int n_step,
                             const double* precond_scale,
                             const double* prior_prec, const double* q0,
                             const double* p0, double logp0,
                             const double* grad0, double hamiltonian_tol,
                             double* q, double* p, double* logp, double* grad,
                             int* n_grad_evals, int* instability,
                             double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on the logit f. */
int bbx_logit_nuts_begin(bbx_logit* logit, const double* precond_scale,
                         const double* prior_prec, const double* q0,
                         const double* p0, double logp0, const double* grad0,
                         double joint_logp0, double joint_logp_threshold,
                         double hamiltonian_tol);
int bbx_logit_nuts_doubling(bbx_logit* logit, double dt, int direction,
                            int height, const double* uniforms,
                            int* n_uniform_used, int* n_steps, int* flags,
                            int* tree, double* averages);
int bbx_logit_nuts_sample(bbx_logit* logit, double* q, double* logp,
                          double* grad);

/* --------------------------------------------------------- Poisson model
 * Incidence-rate regression on a design (intercept column and centred
 * predictors included): counts y_i >= 0 with mean mu_i = exp(eta_i + o_i),
 * eta = X~ beta, o = log(exposure), with the trajectory and the No-U-Turn
 * draw of the Cox handle on it (csrc/poisson.hip; the leapfrog and tree
 * kernels are the Cox handle's, csrc/hamiltonian.hpp).  Every entry point but
 * create has the argument list, the status codes and the synchronisation of
 * its bbx_logit_* counterpart above.  The handle borrows the design (it must
 * outlive the handle) and runs on its stream.  Every sum has a fixed order:
 * the same inputs give the same bits on every call.
 *
 * create: y[n], log_exposure[n] (host; log_exposure may be NULL: all 0).
 * BBX_ERR_INVALID for a NULL y or output pointer, a destroyed or foreign
 * design, a count that is negative or not finite, an offset that is not
 * finite. */
typedef struct bbx_poisson bbx_poisson;
int bbx_poisson_create(bbx_design* design, const double* y,
                       const double* log_exposure, bbx_poisson** out);
int bbx_poisson_destroy(bbx_poisson* poisson);
/* loglik = sum_i y_i eta_i - mu_i (the terms constant in beta, sum_i y_i o_i -
 * log y_i!, are dropped); grad[P] = X~^T (y - mu).  Where eta_i + o_i is past
 * exp's range loglik is -inf and grad is not meaningful; a NaN in beta gives
 * NaN.  grad may be NULL. */
int bbx_poisson_loglik_grad(bbx_poisson* poisson, const double* beta,
                            double* loglik, double* grad);
int bbx_poisson_loglik_grad_dev(bbx_poisson* poisson, const double* d_beta,
                                double* loglik, double* d_grad);
/* Hessian-vector products at a fixed beta: set_location stores mu at beta;
 * hessian_matvec gives out = -X~^T (mu .* (X~ v)) (BBX_ERR_STATE before a
 * set_location). */
int bbx_poisson_set_location(bbx_poisson* poisson, const double* beta);
int bbx_poisson_hessian_matvec(bbx_poisson* poisson, const double* v,
                               double* out);
int bbx_poisson_hessian_matvec_dev(bbx_poisson* poisson, const double* d_v,
                                   double* d_out);
/* bbx_cox_hmc_trajectory on the Poisson f.  A step at which the likelihood
 * overflows is the last one: logp = -inf, *instability = 1. */
int bbx_poisson_hmc_trajectory(bbx_poisson* poisson, double dt, int n_step,
                               const double* precond_scale,
                               const double* prior_prec, const double* q0,
                               const double* p0, double logp0,
                               const double* grad0, double hamiltonian_tol,
                               double* q, double* p, double* logp,
                               double* grad, int* n_grad_evals,
                               int* instability, double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on the Poisson f.  An overflow
 * ends the half-tree as an empty risk-set sum ends the Cox handle's. */
int bbx_poisson_nuts_begin(bbx_poisson* poisson, const double* precond_scale,
                           const double* prior_prec, const double* q0,
                           const double* p0, double logp0, const double* grad0,
                           double joint_logp0, double joint_logp_threshold,
                           double hamiltonian_tol);
int bbx_poisson_nuts_doubling(bbx_poisson* poisson, double dt, int direction,
                              int height, const double* uniforms,
                              int* n_uniform_used, int* n_steps, int* flags,
                              int* tree, double* averages);
int bbx_poisson_nuts_sample(bbx_poisson* poisson, double* q, double* logp,
                            double* grad);

/* ----------------------------------------------- conditional Poisson model
 * Counts with one nuisance baseline rate per stratum (persons of a
 * self-controlled case series, matched sets, sites), conditioned on every
 * stratum's total N_s: the product over strata of multinomial probabilities
 * pi_i = exp(a_i) / sum_{j in s} exp(a_j), a = X~ beta + log(exposure)
 * (csrc/cpoisson.hip; the leapfrog and tree kernels are the Cox handle's,
 * csrc/hamiltonian.hpp).  The design has no intercept column: it cancels
 * inside every stratum.  Rows are stratum-major: stratum s is rows
 * stratum_ptr[s] .. stratum_ptr[s + 1] - 1.  Every entry point but create has
 * the argument list, the status codes and the synchronisation of its
 * bbx_logit_* counterpart above.  The handle borrows the design (it must
 * outlive the handle) and runs on its stream.  Neither the number of launches
 * nor the partition of the rows depends on the strata; every sum has a fixed
 * order: the same inputs give the same bits on every call.
 *
 * create: y[n], log_exposure[n] (host; log_exposure may be NULL: all 0),
 * stratum_ptr[n_strata + 1].  BBX_ERR_INVALID, with a bbx_last_error() that
 * names the argument, for a NULL y, stratum_ptr or output pointer, a destroyed
 * or foreign design, a count that is negative or not finite, an offset that
 * is not finite, a stratum_ptr that does not start at 0, end at n or strictly
 * increase, and a stratum whose counts sum to 0. */
typedef struct bbx_cpoisson bbx_cpoisson;
int bbx_cpoisson_create(bbx_design* design, const double* y,
                        const double* log_exposure, int64_t n_strata,
                        const int64_t* stratum_ptr, bbx_cpoisson** out);
int bbx_cpoisson_destroy(bbx_cpoisson* cpoisson);
/* loglik = sum_i y_i (a_i - L_s(i)), L_s = log sum_{j in s} exp(a_j) (the
 * multinomial coefficient is dropped; loglik <= 0); grad[P] = X~^T w,
 * w_i = y_i - N_s pi_i.  The shift of the log-sum-exp is per stratum: loglik is
 * finite for every finite beta; a NaN in beta gives NaN.  grad may be NULL. */
int bbx_cpoisson_loglik_grad(bbx_cpoisson* cpoisson, const double* beta,
                             double* loglik, double* grad);
int bbx_cpoisson_loglik_grad_dev(bbx_cpoisson* cpoisson, const double* d_beta,
                                 double* loglik, double* d_grad);
/* Hessian-vector products at a fixed beta: set_location stores pi at beta;
 * hessian_matvec gives out = X~^T (-(N_s pi_i (u_i - ubar_s))), u = X~ v,
 * ubar_s = sum_{j in s} pi_j u_j (BBX_ERR_STATE before a set_location). */
int bbx_cpoisson_set_location(bbx_cpoisson* cpoisson, const double* beta);
int bbx_cpoisson_hessian_matvec(bbx_cpoisson* cpoisson, const double* v,
                                double* out);
int bbx_cpoisson_hessian_matvec_dev(bbx_cpoisson* cpoisson, const double* d_v,
                                    double* d_out);
/* bbx_cox_hmc_trajectory on the conditional Poisson f. */
int bbx_cpoisson_hmc_trajectory(bbx_cpoisson* cpoisson, double dt, int n_step,
                                const double* precond_scale,
                                const double* prior_prec, const double* q0,
                                const double* p0, double logp0,
                                const double* grad0, double hamiltonian_tol,
                                double* q, double* p, double* logp,
                                double* grad, int* n_grad_evals,
                                int* instability, double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on the conditional Poisson f. */
int bbx_cpoisson_nuts_begin(bbx_cpoisson* cpoisson,
                            const double* precond_scale,
                            const double* prior_prec, const double* q0,
                            const double* p0, double logp0,
                            const double* grad0, double joint_logp0,
                            double joint_logp_threshold,
                            double hamiltonian_tol);
int bbx_cpoisson_nuts_doubling(bbx_cpoisson* cpoisson, double dt,
                               int direction, int height,
                               const double* uniforms, int* n_uniform_used,
                               int* n_steps, int* flags, int* tree,
                               double* averages);
int bbx_cpoisson_nuts_sample(bbx_cpoisson* cpoisson, double* q, double* logp,
                             double* grad);

/* ------------------------------------------------ negative-binomial model
 * Overdispersed counts on a design (intercept column and centred predictors
 * included): y_i >= 0 with mean mu_i = exp(eta_i + o_i), eta = X~ beta,
 * o = log(exposure), and variance mu_i + mu_i^2 / r; the dispersion r > 0 is a
 * "size", and r -> inf is the Poisson model (csrc/negbin.hip; the leapfrog and
 * tree kernels are the Cox handle's, csrc/hamiltonian.hpp).  With
 * t_i = (eta_i + o_i) - log r,
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|)),
 *   sigma(x) = 1 / (1 + exp(-x)), exp(x) / (1 + exp(x)) for x < 0,
 *   G(y, r) = sum_{j < y} log(r + j) = lgamma(y + r) - lgamma(r).
 * The ten shared entry points have the argument lists, the status codes and
 * the synchronisation of their bbx_logit_* counterparts above.  The handle
 * borrows the design (it must outlive the handle) and runs on its stream.
 * Every sum has a fixed order: the same inputs give the same bits on every
 * call.
 *
 * create: y[n], log_exposure[n] (host; log_exposure may be NULL: all 0), the
 * dispersion the handle starts with.  BBX_ERR_INVALID for a NULL y or output
 * pointer, a destroyed or foreign design, a count that is negative or not
 * finite, an offset that is not finite, a dispersion that is not finite and
 * positive. */
typedef struct bbx_negbin bbx_negbin;
int bbx_negbin_create(bbx_design* design, const double* y,
                      const double* log_exposure, double dispersion,
                      bbx_negbin** out);
int bbx_negbin_destroy(bbx_negbin* negbin);
/* Replaces the handle's r.  It invalidates the Hessian's location (omega holds
 * r): a later hessian_matvec without set_location is BBX_ERR_STATE.
 * BBX_ERR_INVALID for an r that is not finite and positive; BBX_ERR_STATE
 * between bbx_negbin_nuts_begin and bbx_negbin_nuts_sample, while a
 * No-U-Turn tree built with the previous r is open. */
int bbx_negbin_set_dispersion(bbx_negbin* negbin, double r);
/* loglik = sum_i y_i t_i - (y_i + r) softplus(t_i), the part of the log
 * density that depends on beta (sum_i G(y_i, r) - log y_i! is dropped);
 * grad[P] = X~^T w, w_i = y_i - (y_i + r) sigma(t_i).  There is no exp(eta):
 * both are finite for every finite beta.  An infinite eta gives loglik = -inf
 * (grad is then not meaningful) or NaN; a NaN in beta gives NaN.  grad may be
 * NULL. */
int bbx_negbin_loglik_grad(bbx_negbin* negbin, const double* beta,
                           double* loglik, double* grad);
int bbx_negbin_loglik_grad_dev(bbx_negbin* negbin, const double* d_beta,
                               double* loglik, double* d_grad);
/* Hessian-vector products at a fixed beta and the handle's r: set_location
 * stores omega_i = (y_i + r) sigma(t_i) (1 - sigma(t_i)); hessian_matvec gives
 * out = -X~^T (omega .* (X~ v)) (BBX_ERR_STATE before a set_location, and
 * after a set_dispersion until the next one). */
int bbx_negbin_set_location(bbx_negbin* negbin, const double* beta);
int bbx_negbin_hessian_matvec(bbx_negbin* negbin, const double* v,
                              double* out);
int bbx_negbin_hessian_matvec_dev(bbx_negbin* negbin, const double* d_v,
                                  double* d_out);
/* bbx_cox_hmc_trajectory on the negative-binomial f.  A step at which the
 * likelihood is -inf (an infinite eta) is the last one: logp = -inf,
 * *instability = 1. */
int bbx_negbin_hmc_trajectory(bbx_negbin* negbin, double dt, int n_step,
                              const double* precond_scale,
                              const double* prior_prec, const double* q0,
                              const double* p0, double logp0,
                              const double* grad0, double hamiltonian_tol,
                              double* q, double* p, double* logp,
                              double* grad, int* n_grad_evals,
                              int* instability, double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on the negative-binomial f. */
int bbx_negbin_nuts_begin(bbx_negbin* negbin, const double* precond_scale,
                          const double* prior_prec, const double* q0,
                          const double* p0, double logp0, const double* grad0,
                          double joint_logp0, double joint_logp_threshold,
                          double hamiltonian_tol);
int bbx_negbin_nuts_doubling(bbx_negbin* negbin, double dt, int direction,
                             int height, const double* uniforms,
                             int* n_uniform_used, int* n_steps, int* flags,
                             int* tree, double* averages);
int bbx_negbin_nuts_sample(bbx_negbin* negbin, double* q, double* logp,
                           double* grad);
/* out[k] = L(r[k]) = sum_i G(y_i, r[k]) + y_i t_i - (y_i + r[k]) softplus(t_i),
 * t_i = (eta_i + o_i) - log r[k], for n_r values of r (1 <= n_r <= 8; host
 * arrays) in ONE pass over the rows: what the dispersion's conditional
 * density needs.  beta[P] (host): eta = X~ beta is formed and kept on the
 * handle; NULL: the eta of the previous call on this handle (BBX_ERR_STATE if
 * there was none).  One launch of the row kernel, plus the product for a
 * non-NULL beta; one synchronisation.  out[k] depends on r[k] alone: neither
 * on n_r nor on k, bit for bit.  The handle's r, its Hessian location and the
 * scratch of a trajectory or an open tree are not touched.  BBX_ERR_INVALID
 * for n_r outside [1, 8], a NULL r or out, an r[k] that is not finite and
 * positive. */
int bbx_negbin_dispersion_loglik(bbx_negbin* negbin, const double* beta,
                                 int n_r, const double* r, double* out);

/* ---------------------------------------------------------- ordinal model
 * Proportional odds (cumulative logit) for an ordered outcome on a design
 * WITHOUT an intercept column -- the cutpoints are the intercepts: categories
 * y_i in {0, .., K - 1}, 2 <= K <= 16, cutpoints c_1 < .. < c_{K-1}, c_0 =
 * -inf, c_K = +inf, and P(y_i <= k) = sigma(c_{k+1} - (eta_i + o_i)), eta =
 * X~ beta, o an optional per-row offset (csrc/ordinal.hip; the leapfrog and
 * tree kernels are the Cox handle's, csrc/hamiltonian.hpp).  With
 * a = c_{y+1} - (eta + o), b = c_y - (eta + o), delta_k = c_{k+1} - c_k,
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|)),
 *   sigma(x) = 1 / (1 + e), e / (1 + e) for x < 0, e = exp(-|x|),
 *   g_k = log(1 - exp(-delta_k)) for 0 < k < K - 1, else 0
 *         (log(-expm1(-delta)) for delta <= log 2, else log1p(-exp(-delta))),
 *   ll_i = (g_y - softplus(-a)) - softplus(b)     (= log P(y_i), every term:
 *          the softplus(-a) term is absent for y = K - 1, softplus(b) for
 *          y = 0)
 *   w_i  = sigma(b) - sigma(-a)
 *   d_i  = sigma(a) sigma(-a) + sigma(b) sigma(-b),
 *          sigma(x) sigma(-x) = e / ((1 + e) (1 + e)).
 * Nothing cancels and no exp overflows: every value is finite for a finite
 * eta.  The ten shared entry points have the argument lists, the status codes
 * and the synchronisation of their bbx_logit_* counterparts above.  The handle
 * borrows the design (it must outlive the handle) and runs on its stream.
 * Every sum has a fixed order: the same inputs give the same bits on every
 * call.
 *
 * create: y[n], offset[n] (host; offset may be NULL: all 0), n_category = K
 * and the K - 1 cutpoints the handle starts with.  BBX_ERR_INVALID for a NULL
 * y, cutpoints or output pointer, a destroyed or foreign design, K outside
 * [2, 16], a y that is not an integer in [0, K - 1], an offset that is not
 * finite, cutpoints that are not finite and strictly increasing. */
typedef struct bbx_ordinal bbx_ordinal;
int bbx_ordinal_create(bbx_design* design, const double* y,
                       const double* offset, int n_category,
                       const double* cutpoints, bbx_ordinal** out);
int bbx_ordinal_destroy(bbx_ordinal* ordinal);
/* Replaces the handle's K - 1 cutpoints (host array): the table of (c_k,
 * c_{k+1}, g_k) per category is rebuilt on the host and uploaded in stream
 * order.  It invalidates the Hessian's location (d holds the cutpoints): a
 * later hessian_matvec without set_location is BBX_ERR_STATE.
 * BBX_ERR_INVALID for NULL or for cutpoints that are not finite and strictly
 * increasing; BBX_ERR_STATE between bbx_ordinal_nuts_begin and
 * bbx_ordinal_nuts_sample, while a No-U-Turn tree built with the previous
 * cutpoints is open. */
int bbx_ordinal_set_cutpoints(bbx_ordinal* ordinal, const double* cutpoints);
/* loglik = sum_i ll_i, the whole log-probability (g_y included: it depends on
 * the cutpoints); grad[P] = X~^T w.  An infinite eta gives loglik = -inf where
 * the row's category has probability 0 (grad is then not meaningful); in the
 * end category on that side (y = K - 1 at eta = +inf, y = 0 at eta = -inf)
 * the row gives ll_i = 0, w_i = 0, d_i = 0.  A NaN in beta gives NaN.  grad
 * may be NULL. */
int bbx_ordinal_loglik_grad(bbx_ordinal* ordinal, const double* beta,
                            double* loglik, double* grad);
int bbx_ordinal_loglik_grad_dev(bbx_ordinal* ordinal, const double* d_beta,
                                double* loglik, double* d_grad);
/* Hessian-vector products at a fixed beta and the handle's cutpoints:
 * set_location stores d_i; hessian_matvec gives out = -X~^T (d .* (X~ v))
 * (BBX_ERR_STATE before a set_location, and after a set_cutpoints until the
 * next one). */
int bbx_ordinal_set_location(bbx_ordinal* ordinal, const double* beta);
int bbx_ordinal_hessian_matvec(bbx_ordinal* ordinal, const double* v,
                               double* out);
int bbx_ordinal_hessian_matvec_dev(bbx_ordinal* ordinal, const double* d_v,
                                   double* d_out);
/* bbx_cox_hmc_trajectory on the proportional-odds f.  A step at which the
 * likelihood is -inf (an infinite eta) is the last one: logp = -inf,
 * *instability = 1. */
int bbx_ordinal_hmc_trajectory(bbx_ordinal* ordinal, double dt, int n_step,
                               const double* precond_scale,
                               const double* prior_prec, const double* q0,
                               const double* p0, double logp0,
                               const double* grad0, double hamiltonian_tol,
                               double* q, double* p, double* logp,
                               double* grad, int* n_grad_evals,
                               int* instability, double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on the proportional-odds f. */
int bbx_ordinal_nuts_begin(bbx_ordinal* ordinal, const double* precond_scale,
                           const double* prior_prec, const double* q0,
                           const double* p0, double logp0, const double* grad0,
                           double joint_logp0, double joint_logp_threshold,
                           double hamiltonian_tol);
int bbx_ordinal_nuts_doubling(bbx_ordinal* ordinal, double dt, int direction,
                              int height, const double* uniforms,
                              int* n_uniform_used, int* n_steps, int* flags,
                              int* tree, double* averages);
int bbx_ordinal_nuts_sample(bbx_ordinal* ordinal, double* q, double* logp,
                            double* grad);
/* out[k] = L(cuts[k]) = sum_i ll_i at the cutpoint vector cuts[k][K - 1], for
 * n_c whole vectors (1 <= n_c <= 8; host arrays, candidate-major) in ONE pass
 * over the rows: what a cutpoint's conditional density needs.  beta[P]
 * (host): eta = X~ beta is formed and kept on the handle; NULL: the eta of the
 * previous call on this handle (BBX_ERR_STATE if there was none).  One launch
 * of the cutpoint kernel, plus the product for a non-NULL beta; one
 * synchronisation.  out[k] depends on cuts[k] alone: neither on n_c nor on k,
 * bit for bit.  The handle's cutpoints, its Hessian location and the scratch
 * of a trajectory or an open tree are not touched.  BBX_ERR_INVALID for n_c
 * outside [1, 8], a NULL cuts or out, a cuts[k] that is not finite and
 * strictly increasing. */
int bbx_ordinal_cutpoint_loglik(bbx_ordinal* ordinal, const double* beta,
                                int n_c, const double* cuts, double* out);

/* ---------------------------------------------------------- Weibull model
 * Proportional hazards with a Weibull baseline for right-censored times on a
 * design (intercept column and centred predictors included): rows (d_i, lt_i),
 * d = 1 for an event at t and 0 for a row censored at t, lt = log t; hazard
 * h(t | x) = k t^(k - 1) exp(eta), eta = X~ beta, shape k > 0 (k = 1: the
 * exponential model) (csrc/weibull.hip; the leapfrog and tree kernels are the
 * Cox handle's, csrc/hamiltonian.hpp).  Every product is rounded before the
 * sum it enters:
 *   m_i  = exp(eta_i + (k * lt_i))
 *   ll_i = (d_i * eta_i) - m_i        the part that depends on beta
 *   w_i  = d_i - m_i
 *   full_i = d_i * ((log k + ((k - 1) * lt_i)) + eta_i) - m_i
 * At k = 1 every value is the bbx_poisson handle's on y = d, log_exposure =
 * lt, bit for bit.  The ten shared entry points have the argument lists, the
 * status codes and the synchronisation of their bbx_logit_* counterparts
 * above.  The handle borrows the design (it must outlive the handle) and runs
 * on its stream.  Every sum has a fixed order: the same inputs give the same
 * bits on every call.
 *
 * create: event[n], log_time[n] (host) and the shape the handle starts with.
 * BBX_ERR_INVALID for a NULL array or output pointer, a destroyed or foreign
 * design, an event[i] that is not 0 or 1, a log_time[i] that is not finite
 * (the message names the row), a shape that is not finite and positive. */
typedef struct bbx_weibull bbx_weibull;
int bbx_weibull_create(bbx_design* design, const double* event,
                       const double* log_time, double shape,
                       bbx_weibull** out);
int bbx_weibull_destroy(bbx_weibull* weibull);
/* Replaces the handle's k.  It invalidates the Hessian's location (m holds
 * k): a later hessian_matvec without set_location is BBX_ERR_STATE.
 * BBX_ERR_INVALID for a k that is not finite and positive; BBX_ERR_STATE
 * between bbx_weibull_nuts_begin and bbx_weibull_nuts_sample, while a
 * No-U-Turn tree built with the previous k is open. */
int bbx_weibull_set_shape(bbx_weibull* weibull, double k);
/* loglik = sum_i ll_i, the part of the log density that depends on beta
 * (sum_i d_i (log k + (k - 1) lt_i) is dropped); grad[P] = X~^T w.  Where
 * eta + k lt is past exp's range m = inf: loglik = -inf and grad is not
 * meaningful (NaN where eta itself is +inf and d = 1); a NaN in beta gives
 * NaN.  grad may be NULL. */
int bbx_weibull_loglik_grad(bbx_weibull* weibull, const double* beta,
                            double* loglik, double* grad);
int bbx_weibull_loglik_grad_dev(bbx_weibull* weibull, const double* d_beta,
                                double* loglik, double* d_grad);
/* Hessian-vector products at a fixed beta and the handle's k: set_location
 * stores m_i; hessian_matvec gives out = -X~^T (m .* (X~ v)) (BBX_ERR_STATE
 * before a set_location, and after a set_shape until the next one). */
int bbx_weibull_set_location(bbx_weibull* weibull, const double* beta);
int bbx_weibull_hessian_matvec(bbx_weibull* weibull, const double* v,
                               double* out);
int bbx_weibull_hessian_matvec_dev(bbx_weibull* weibull, const double* d_v,
                                   double* d_out);
/* bbx_cox_hmc_trajectory on the Weibull f.  A step at which an m overflows is
 * the last one: logp = -inf, *instability = 1. */
int bbx_weibull_hmc_trajectory(bbx_weibull* weibull, double dt, int n_step,
                               const double* precond_scale,
                               const double* prior_prec, const double* q0,
                               const double* p0, double logp0,
                               const double* grad0, double hamiltonian_tol,
                               double* q, double* p, double* logp,
                               double* grad, int* n_grad_evals,
                               int* instability, double* hamiltonian);
/* bbx_cox_nuts_begin / _doubling / _sample on the Weibull f. */
int bbx_weibull_nuts_begin(bbx_weibull* weibull, const double* precond_scale,
                           const double* prior_prec, const double* q0,
                           const double* p0, double logp0, const double* grad0,
                           double joint_logp0, double joint_logp_threshold,
                           double hamiltonian_tol);
int bbx_weibull_nuts_doubling(bbx_weibull* weibull, double dt, int direction,
                              int height, const double* uniforms,
                              int* n_uniform_used, int* n_steps, int* flags,
                              int* tree, double* averages);
int bbx_weibull_nuts_sample(bbx_weibull* weibull, double* q, double* logp,
                            double* grad);
/* out[j] = L(k[j]) = sum_i full_i at the shape k[j], for n_k values (1 <= n_k
 * <= 8; host arrays) in ONE pass over the rows: what the shape's conditional
 * density needs.  beta[P] (host): eta = X~ beta is formed and kept on the
 * handle; NULL: the eta of the previous call on this handle (BBX_ERR_STATE if
 * there was none).  One launch of the shape kernel, plus the product for a
 * non-NULL beta; one synchronisation.  out[j] depends on k[j] alone: neither
 * on n_k nor on j, bit for bit.  A k[j] at which a row's exp overflows gives
 * exactly -inf for a finite eta.  The handle's k, its Hessian location and
 * the scratch of a trajectory or an open tree are not touched.
 * BBX_ERR_INVALID for n_k outside [1, 8], a NULL k or out, a k[j] that is not
 * finite and positive. */
int bbx_weibull_shape_loglik(bbx_weibull* weibull, const double* beta, int n_k,
                             const double* k, double* out);

/* ----------------------- host-side reference-stream samplers (libbbx_hostrng)
 * Exported by the separate, HIP-free libbbx_hostrng.so.  `bitgen` is the
 * address of a NumPy bitgen_t (PCG64(seed).ctypes.bit_generator); the draws
 * consume it exactly as random/polya_gamma/polya_gamma.pyx:40-74 and
 * random/tilted_stable/tilted_stable.pyx:65-134 do. */
int bbx_host_polya_gamma(void* bitgen, int64_t n, const int32_t* shape,
                         const double* tilt, double* out);
int bbx_host_tilted_stable(void* bitgen, int64_t n, const double* char_exp,
                           const double* tilt, double* out);
/* Checks of the device chain's Polya-Gamma arithmetic against the
 * reference-following one, on the host (both are in csrc/samplers.hpp):
 *   right_mass: log_form[i] = the mixture weight of the exponential piece at
 *     z[i] as polya_gamma.pyx:115-128 forms it (sums of logarithms),
 *     direct[i] = the device kernel's product form;
 *   series_accept: the alternating-series test (polya_gamma.pyx:139-162) of the
 *     proposal x[i] with the uniform u[i], 1 = accepted: sequential[i] with the
 *     terms of polya_gamma.pyx:131-137, direct[i] with the kernel's. */
int bbx_host_pg_right_mass(int64_t n, const double* z, double* log_form,
                           double* direct);
int bbx_host_pg_series_accept(int64_t n, const double* x, const double* u,
                              int32_t* sequential, int32_t* direct);
/* out[i] = log Phi(x[i]) as csrc/samplers.hpp forms it on the host (the probit
 * model's log-likelihood term is the same function on the device). */
int bbx_host_log_norm_cdf(int64_t n, const double* x, double* out);

/* ---------------------- sequential replay of the device draws (libbbx_hostrng)
 * Every draw of the device chain is a function of (seed, stream, element,
 * inputs): these walk the same Philox sub-streams on the host, one element
 * after the other, with none of the kernels' structure (csrc/replay_impl.hpp).
 * `stream` is the kernel's stream word, e.g. STREAM_PG | iteration << 8.
 * `variant` 0: the reference's arithmetic (pow, the log forms of the
 * Polya-Gamma pieces); 1: the kernels' forms (roots and integer powers,
 * right_mass_direct, series_accept_direct) in the host's libm. */
/* One Philox4x32-10 block, and the counter / key words of a generator. */
int bbx_replay_philox_block(const uint32_t* counter, const uint32_t* key,
                            uint32_t* out);
int bbx_replay_philox_counter(uint64_t seed, uint64_t stream, uint64_t index,
                              uint32_t trial, uint32_t* counter, uint32_t* key);
/* The first n uniforms of Philox(seed, stream, index, trial). */
int bbx_replay_uniform(uint64_t seed, uint64_t stream, uint64_t index,
                       uint32_t trial, int64_t n, double* out);
/* out[i] = the first normal of Philox(seed, stream, i) (bbx_device_normal). */
int bbx_replay_normal(uint64_t seed, uint64_t stream, int64_t n, double* out);
/* polya_gamma_block (csrc/pg_queue.hpp) restated; `shape`: int32 or, with
 * shape_is_double, double entries.  Optional traces: attempts[i] = the
 * inverse-Gaussian proposals element i took (0: none needed), restarts[i] = 1
 * when its series test rejected and the draw started over. */
int bbx_replay_polya_gamma(uint64_t seed, uint64_t stream, int64_t n,
                           int shape_is_double, const void* shape,
                           const double* tilt, int variant, double* out,
                           int32_t* attempts, int32_t* restarts);
/* tilted_stable_block (csrc/chain.hip) restated: candidates 0, 1, 2, ... in
 * order, the first accepted one is the draw; winner[i] (optional) = its
 * number.  Tilts must be finite and >= 0. */
int bbx_replay_tilted_stable(uint64_t seed, uint64_t stream, int64_t n,
                             double char_exp, const double* tilt, int variant,
                             double* out, int32_t* winner);
/* The probit row policy (ProbitRows, csrc/probit.hip) restated: the trials 0, 1, 2, ... of
 * element i in order, trial t on Philox(seed, stream, i, t), the first accepted
 * proposal is the draw (TruncatedNormal of csrc/samplers.hpp; variant 1: the
 * kernel's forms of the proposal rate and of the exponential variate).
 * positive[i] != 0: the half-line z > 0 (y = 1), else z <= 0.  trials[i]
 * (optional) = the trials made, 0 for a psi that is not finite (the draw is
 * then a NaN). */
int bbx_replay_truncated_normal(uint64_t seed, uint64_t stream, int64_t n,
                                const double* psi,
                                const unsigned char* positive, int variant,
                                double* out, int32_t* trials);
/* The quantile row policy's draw (QuantileRows, csrc/quantile.hip) restated:
 * out[i] = InverseGaussian::draw (csrc/samplers.hpp) at (m[i], lambda) on
 * Philox(seed, stream, i): one normal, then one uniform.  The draw is sums,
 * products, quotients and a square root, the same on host and device, so
 * variant 1 is variant 0.  branch[i] (optional) = 0 where the smaller root was
 * taken, 1 for the other; margin[i] (optional) = u (1 + m x), the number
 * compared with 1.  BBX_ERR_INVALID for a lambda that is not positive. */
int bbx_replay_inverse_gaussian(uint64_t seed, uint64_t stream, int64_t n,
                                const double* m, double lambda, int variant,
                                double* out, int32_t* branch, double* margin);
/* out[k] = gamma_draw on Philox(seed, stream, index + k). */
int bbx_replay_gamma(uint64_t seed, uint64_t stream, uint64_t index, int64_t n,
                     double shape, double* out);

#ifdef __cplusplus
}
#endif
#endif /* BBX_H */
