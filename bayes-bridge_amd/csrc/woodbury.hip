// Dense designs with more columns than rows: the transposed weighted Gram
// (dense_matrix.py:60-61, an empty `compute_transposed_fisher_info` in the
// reference) and the n-space ('woodbury') draw of the coefficients that the
// reference leaves as a TODO (gibbs_util.py:66-68).
//
// Why a file of its own and not next to gram_tiles_kernel: that kernel contracts
// over ROWS (its two operands are column segments, read across rows); this one
// contracts over COLUMNS (both operands are row segments), so the loads, the
// chunking and the bounds differ, and everything else here (the glue of the
// draw) belongs to this sampler alone.  The factorisation and the triangular
// solves ARE shared: cholesky.hip exports them (chol_factor_enqueue,
// chol_solve_enqueue).
//
//   G = X~ diag(d) X~^T      n x n, f64, d[P] >= 0       wb_gram_tiles_kernel
//   M = s_i G_ij s_j + [i == j],  s = sqrt(obs_prec)      wb_gram_reduce_kernel
//
// Gram.  The output is cut into 64 x 64 tiles, lower triangle only.  A workgroup
// (4 waves) owns one tile and one chunk of columns; wave q takes every fourth
// group of 16 columns and keeps 4 x 4 accumulators of v_mfma_f64_16x16x4_f64.
// Lane l (r = l & 15, k = l >> 4) loads FOUR adjacent entries of a row (16 bytes
// of f32 storage, 32 of f64): X~[I0 + 16 a + r][c0 + 4 k + t], t = 0..3, and
// the four MFMAs of a group use t = 0..3 in turn, so that MFMA t contracts the
// columns c0 + 4 k + t, k = 0..3:
//   A[i][k] = X~[I0 + 16 a + i][c0 + 4 k + t]             lane l: i = l & 15, k = l >> 4
//   B[k][j] = d[c0 + 4 k + t] X~[J0 + 16 b + j][c0 + 4 k + t]      k = l >> 4, j = l & 15
//   D row = (l >> 4) + 4 reg, col = l & 15      (cdna_hip_programming.md "f64 MFMA")
// (a sum over columns does not care in which order the k slots carry them, as
// long as A, B and d agree.)  The 16 lanes of a k read 16 rows, 64 bytes of f32
// each.  f32 storage is widened on load.  The four waves are added in LDS in a
// fixed order, every (chunk, tile) partial goes to its own slot of a slab and
// wb_gram_reduce_kernel adds the chunks in chunk order: no atomics, two calls
// give the same bits.  The slab is bounded as the P x P Gram's is
// (gram_slab_limit); when the lower triangle does not fit, tiles go in batches.
// Columns with d = 0 (the flat coefficients) drop out of the sum by themselves.
//
// The draw: Phi = diag(s) X~, alpha = s .* y, D = 1 / pps^2 on R
// = {pps > 0}, F = {pps == 0} (flat prior: the intercept and fixed effects under
// the default prior), q = |F| <= WB_QMAX:
//   u      = D_R^{1/2} xi_R
//   M      = Phi_R D_R Phi_R^T + I = L L^T
//   r      = Q (alpha - Phi_R u - delta),   Q = I - Phi_F (Phi_F^T Phi_F)^-1 Phi_F^T
//   Z      = M^-1 [r | Phi_F]               q + 1 solves with the one factor
//   lambda = -(Phi_F^T Z_F)^-1 Phi_F^T Z_r,     w = Z_r + Z_F lambda
//   beta_R = u + D_R Phi_R^T w
//   beta_F = C^-1 Phi_F^T (alpha - Phi_R beta_R) + chol(C)^-T xi_F,   C = Phi_F^T Phi_F
// The q x q systems are solved on the host (q is a handful); what crosses is
// O(q^2) numbers, four times per draw.  Everything of size n, P, n x n stays on
// the device.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.hpp"

namespace bbx {

typedef double wb_d4 __attribute__((ext_vector_type(4)));
constexpr int WB = 64;            // tile / block size (= cholesky.hip's CB)
constexpr int WB_QMAX = 32;       // most flat coefficients
constexpr int64_t WB_NMAX = 19200;  // as the 'cholesky' draw's bound on P
constexpr int WB_NO_FAIL = 0x7fffffff;

struct WbIdx {
  int v[WB_QMAX];
};
struct WbCoef {
  double v[WB_QMAX];
};

__device__ __forceinline__ void wb_tile_of(int t, int* bi, int* bj) {
  // t -> (bi, bj), bi >= bj, row-major over the lower triangle
  int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((int64_t)i * (i + 1) / 2 > t) --i;
  while ((int64_t)(i + 1) * (i + 2) / 2 <= t) ++i;
  *bi = i;
  *bj = t - i * (i + 1) / 2;
}

template <typename T>
struct WbQuad;
template <>
struct WbQuad<float> {
  using type = float4;
};
template <>
struct WbQuad<double> {
  using type = double4;
};

// ---------------------------------------------------------------------------
// Gram partials: slab[chunk][tile - t0][64][64].  d has >= ld entries (zero
// past P); ld is a multiple of 4 and every chunk starts at a multiple of 64.
template <typename T>
__global__ __launch_bounds__(256) void wb_gram_tiles_kernel(
    const T* __restrict__ X, int64_t ld, int64_t n, const double* __restrict__ d,
    int64_t cols_per_chunk, int t0, int nt, double* __restrict__ slab) {
  using V4 = typename WbQuad<T>::type;
  __shared__ double red[WB * WB];
  const int t = t0 + (int)blockIdx.x;
  int bi, bj;
  wb_tile_of(t, &bi, &bj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kk = lane >> 4;
  const int64_t c_lo = (int64_t)blockIdx.y * cols_per_chunk;
  const int64_t c_hi = min(ld, c_lo + cols_per_chunk);
  const T* rowA[4];
  const T* rowB[4];
  bool okA[4], okB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t ia = (int64_t)bi * WB + 16 * q + r;
    const int64_t ib = (int64_t)bj * WB + 16 * q + r;
    okA[q] = ia < n;
    okB[q] = ib < n;
    rowA[q] = X + (okA[q] ? ia : 0) * ld;
    rowB[q] = X + (okB[q] ? ib : 0) * ld;
  }
  wb_d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = wb_d4{0., 0., 0., 0.};
  for (int64_t c0 = c_lo + 16 * wave; c0 < c_hi; c0 += 64) {
    const int64_t col = c0 + 4 * kk;
    const bool cok = col < c_hi;     // whole quad in or out: c_hi % 4 == 0
    double av[4][4], bv[4][4];
    double dv[4] = {0., 0., 0., 0.};
    if (cok) {
      const double4 dd = *reinterpret_cast<const double4*>(d + col);
      dv[0] = dd.x;
      dv[1] = dd.y;
      dv[2] = dd.z;
      dv[3] = dd.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (cok && okA[q]) {
        const V4 x = *reinterpret_cast<const V4*>(rowA[q] + col);
        av[q][0] = (double)x.x;
        av[q][1] = (double)x.y;
        av[q][2] = (double)x.z;
        av[q][3] = (double)x.w;
      } else {
        av[q][0] = av[q][1] = av[q][2] = av[q][3] = 0.;
      }
      if (cok && okB[q]) {
        const V4 x = *reinterpret_cast<const V4*>(rowB[q] + col);
        bv[q][0] = dv[0] * (double)x.x;
        bv[q][1] = dv[1] * (double)x.y;
        bv[q][2] = dv[2] * (double)x.z;
        bv[q][3] = dv[3] * (double)x.w;
      } else {
        bv[q][0] = bv[q][1] = bv[q][2] = bv[q][3] = 0.;
      }
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a][tt], bv[b][tt],
                                                           acc[a][b], 0, 0, 0);
  }
  // waves 0, 1, 2, 3 added in this order
  for (int q = 0; q < 4; ++q) {
    if (wave == q) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int i = 16 * a + kk + 4 * g, j = 16 * b + r;
            red[i * WB + j] = q == 0 ? acc[a][b][g] : red[i * WB + j] + acc[a][b][g];
          }
    }
    __syncthreads();
  }
  double* out = slab + ((size_t)blockIdx.y * nt + blockIdx.x) * (WB * WB);
  for (int e = threadIdx.x; e < WB * WB; e += 256) out[e] = red[e];
}

// Tiles of one batch = sum over chunks (in chunk order), and their mirrors.
// s == nullptr: out = G (n_out x n_out entries, leading dimension ldo).
// s != nullptr: out = s_i G_ij s_j + [i == j] on all n_out = n_pad rows (the
// padding is the identity: G is zero there and s is zero-padded).
__global__ __launch_bounds__(256) void wb_gram_reduce_kernel(
    const double* __restrict__ slab, int chunks, int t0, int nt,
    const double* __restrict__ s, int64_t n_out, double* __restrict__ out,
    int64_t ldo) {
  const int t = t0 + (int)blockIdx.x;
  int bi, bj;
  wb_tile_of(t, &bi, &bj);
  for (int e = threadIdx.x; e < WB * WB; e += 256) {
    double g = 0.;
    for (int k = 0; k < chunks; ++k)
      g += slab[((size_t)k * nt + blockIdx.x) * (WB * WB) + e];
    // a diagonal tile keeps its lower half: the result is symmetric bit for bit
    if (bi == bj && e % WB > e / WB) continue;
    const int64_t i = (int64_t)bi * WB + e / WB, j = (int64_t)bj * WB + e % WB;
    if (i >= n_out || j >= n_out) continue;
    if (s) g = s[i] * g * s[j] + (i == j ? 1. : 0.);
    out[i * ldo + j] = g;
    out[j * ldo + i] = g;
  }
}

// ---------------------------------------------------------------------------
// d = 1 / pps^2, u = xi / pps on R; zero on F (pps == 0, listed in idx, in any
// order: the host sorts), on pps = inf and past P.
__global__ __launch_bounds__(256) void wb_prep_kernel(
    int64_t P, int64_t Pd, const double* __restrict__ pps,
    const double* __restrict__ xi, double* __restrict__ d,
    double* __restrict__ u, int* __restrict__ count_idx) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Pd) return;
  double dj = 0., uj = 0.;
  if (j < P) {
    const double p = pps[j];
    if (p > 0.) {
      if (isfinite(p)) {
        dj = 1. / (p * p);
        uj = xi[j] / p;
      }
    } else {
      // (a negative or NaN entry lands here too and is reported by the host
      // through the count of a second slot)
      const int k = atomicAdd(count_idx, 1);
      if (k < WB_QMAX) count_idx[2 + k] = (int)j;
      if (!(p == 0.)) atomicAdd(count_idx + 1, 1);
    }
  }
  d[j] = dj;
  u[j] = uj;
}

__global__ void wb_reset_kernel(int* count_idx, int* info) {
  count_idx[0] = 0;
  count_idx[1] = 0;
  *info = WB_NO_FAIL;
}

// s = sqrt(obs_prec), alpha = s y (y_is_wy: y holds obs_prec .* y, alpha = y / s)
__global__ __launch_bounds__(256) void wb_rows_kernel(
    int64_t n, int64_t n_pad, const double* __restrict__ obs_prec,
    double obs_scalar, const double* d_obs_scalar, const double* __restrict__ y,
    int y_is_wy, double* __restrict__ s, double* __restrict__ alpha) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  if (i >= n) {
    s[i] = 0.;
    alpha[i] = 0.;
    return;
  }
  const double om = obs_prec ? obs_prec[i] : (d_obs_scalar ? *d_obs_scalar : obs_scalar);
  const double si = sqrt(om);
  s[i] = si;
  alpha[i] = y_is_wy ? y[i] / si : si * y[i];
}

// phiF[k][i] = s_i X~[i][idx[k]]   (zero past n)
template <typename T>
__global__ __launch_bounds__(256) void wb_phif_kernel(
    const T* __restrict__ X, int64_t ld, int64_t n, int64_t n_pad, WbIdx idx,
    const double* __restrict__ s, double* __restrict__ phiF) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  const int k = blockIdx.y;
  phiF[(size_t)k * n_pad + i] = i < n ? s[i] * (double)X[i * ld + idx.v[k]] : 0.;
}

// out[i] = sign * (a[i] - b[i] - c[i])  on i < n (b, c may be null), zero past n
__global__ __launch_bounds__(256) void wb_resid_kernel(
    int64_t n, int64_t n_pad, const double* __restrict__ a,
    const double* __restrict__ b, const double* __restrict__ c,
    double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  double v = 0.;
  if (i < n) {
    v = a[i];
    if (b) v -= b[i];
    if (c) v -= c[i];
  }
  out[i] = v;
}

// out[i] = scale_i * (base[i] + sum_k coef[k] V[k][i]), k in order
__global__ __launch_bounds__(256) void wb_lincomb_kernel(
    int64_t len, int64_t stride, const double* __restrict__ base,
    const double* __restrict__ V, int m, WbCoef coef,
    const double* __restrict__ scale, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  double v = base[i];
  for (int k = 0; k < m; ++k) v += coef.v[k] * V[(size_t)k * stride + i];
  out[i] = scale ? scale[i] * v : v;
}

// out[a * mb + b] = <A[a], B[b]> over len entries: one workgroup per pair, each
// thread a strided share, then a fixed tree in LDS
__global__ __launch_bounds__(256) void wb_inner_kernel(
    int64_t len, int64_t stride, const double* __restrict__ A,
    const double* __restrict__ B, int mb, double* __restrict__ out) {
  __shared__ double part[256];
  const double* a = A + (size_t)blockIdx.x * stride;
  const double* b = B + (size_t)blockIdx.y * stride;
  double v = 0.;
  for (int64_t i = threadIdx.x; i < len; i += 256) v += a[i] * b[i];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x * mb + blockIdx.y] = part[0];
}

// coef = u + d .* g
__global__ __launch_bounds__(256) void wb_beta_r_kernel(
    int64_t P, const double* __restrict__ u, const double* __restrict__ d,
    const double* __restrict__ g, double* __restrict__ coef) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < P) coef[j] = u[j] + d[j] * g[j];
}

__global__ void wb_scatter_kernel(int q, WbIdx idx, WbCoef val, double* coef) {
  const int k = threadIdx.x;
  if (k < q) coef[idx.v[k]] = val.v[k];
}

// ---------------------------------------------------------------------------
static inline unsigned wb_blocks(int64_t m) { return (unsigned)((m + 255) / 256); }
static int64_t wb_npad(const bbx_design* h) { return (h->n + WB - 1) / WB * WB; }
static int64_t wb_pd(const bbx_design* h) { return (h->dense_ld + 63) / 64 * 64; }

// Column chunks of the Gram: enough workgroups for the device (>= ~2048 with
// the tiles), >= 1024 columns each (a multiple of 64: 4 waves x 16 columns),
// at most 64 partial slabs.
static int wb_gram_chunks(int64_t ld, int64_t tiles, int64_t* cols) {
  int64_t c = (2048 + tiles - 1) / tiles;
  c = std::min<int64_t>(c, std::max<int64_t>(1, ld / 1024));
  c = std::max<int64_t>(1, std::min<int64_t>(c, 64));
  int64_t per = (ld + c - 1) / c;
  per = (per + 63) / 64 * 64;
  *cols = per;
  return (int)((ld + per - 1) / per);
}

// G (s == nullptr; n x n into d_out, leading dimension ldo) or M (s given; n_pad
// x n_pad into d_out, ldo = n_pad).  d_d: wb_pd(h) doubles, zero past P.
static int wb_gram_device(bbx_design* h, const double* d_d, const double* d_s,
                          double* d_out, int64_t ldo) {
  const int64_t n_pad = wb_npad(h);
  const int nb = (int)(n_pad / WB);
  const int64_t tiles = (int64_t)nb * (nb + 1) / 2;
  int64_t cols = 0;
  const int chunks = wb_gram_chunks(h->dense_ld, tiles, &cols);
  const int64_t per_tile = (int64_t)chunks * WB * WB * sizeof(double);
  const int64_t batch = std::max<int64_t>(
      1, std::min<int64_t>(tiles, (int64_t)gram_slab_limit() / per_tile));
  const size_t need = (size_t)(batch * per_tile);
  if (h->chol_slab.bytes < need) {
    h->chol_slab.release();
    BBX_TRY(h->chol_slab.alloc(need));
  }
  double* slab = h->chol_slab.as<double>();
  const int64_t n_out = d_s ? n_pad : h->n;
  for (int64_t t0 = 0; t0 < tiles; t0 += batch) {
    const int nt = (int)std::min<int64_t>(batch, tiles - t0);
    if (h->dense_dtype == BBX_F32)
      BBX_LAUNCH(wb_gram_tiles_kernel<float>, dim3(nt, chunks), dim3(256), 0,
                 h->stream, h->dense.as<float>(), h->dense_ld, h->n, d_d, cols,
                 (int)t0, nt, slab);
    else
      BBX_LAUNCH(wb_gram_tiles_kernel<double>, dim3(nt, chunks), dim3(256), 0,
                 h->stream, h->dense.as<double>(), h->dense_ld, h->n, d_d, cols,
                 (int)t0, nt, slab);
    BBX_LAUNCH(wb_gram_reduce_kernel, dim3(nt), dim3(256), 0, h->stream, slab,
               chunks, (int)t0, nt, d_s, n_out, d_out, ldo);
  }
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// Work vectors of the draw, carved from h->wb_vec
struct WbWork {
  double *s, *alpha, *b, *y, *w, *t;   // n_pad each
  double* phiF;                         // (QMAX + 1) x n_pad: Phi_F, then r0
  double* Z;                            // (QMAX + 1) x n_pad
  double *d, *u, *g;                    // Pd each
  double* small;                        // (QMAX + 1)^2
  double* stage[6];                     // host entry: n, P, n, n, P, P
  int* count_idx;                       // count, bad count, QMAX indices
  int* info;
};

static size_t wb_vec_doubles(const bbx_design* h) {
  const size_t np = (size_t)wb_npad(h), pd = (size_t)wb_pd(h);
  return np * (6 + 2 * (WB_QMAX + 1) + 3) + pd * (3 + 3) +
         (size_t)(WB_QMAX + 1) * (WB_QMAX + 1) + WB_QMAX + 16;
}

static int wb_buffers(bbx_design* h, bool with_matrix, WbWork* wk) {
  if (h->n > WB_NMAX)
    return fail(BBX_ERR_INVALID,
                "the woodbury sampler factors an n x n matrix: more than 19200 "
                "rows (2.9 GB)");
  const int64_t n_pad = wb_npad(h);
  if (with_matrix) {
    const size_t mat = sizeof(double) * (size_t)n_pad * (size_t)n_pad;
    if (h->chol_A.bytes < mat) BBX_TRY(h->chol_A.alloc(mat));
  }
  const size_t need = sizeof(double) * wb_vec_doubles(h);
  if (h->wb_vec.bytes < need) BBX_TRY(h->wb_vec.alloc(need));
  const size_t np = (size_t)n_pad, pd = (size_t)wb_pd(h);
  double* p = h->wb_vec.as<double>();
  auto take = [&](size_t len) {
    double* r = p;
    p += len;
    return r;
  };
  wk->d = take(pd);           // 32-byte aligned loads: first
  wk->u = take(pd);
  wk->g = take(pd);
  wk->s = take(np);
  wk->alpha = take(np);
  wk->b = take(np);
  wk->y = take(np);
  wk->w = take(np);
  wk->t = take(np);
  wk->phiF = take(np * (WB_QMAX + 1));
  wk->Z = take(np * (WB_QMAX + 1));
  wk->stage[0] = take(np);
  wk->stage[1] = take(pd);
  wk->stage[2] = take(np);
  wk->stage[3] = take(np);
  wk->stage[4] = take(pd);
  wk->stage[5] = take(pd);
  wk->small = take((size_t)(WB_QMAX + 1) * (WB_QMAX + 1));
  wk->count_idx = reinterpret_cast<int*>(take(WB_QMAX / 2 + 2));
  wk->info = reinterpret_cast<int*>(take(1));
  return BBX_OK;
}

double* wb_stage(bbx_design* h, int k) {
  WbWork wk;
  if (h->sparse || wb_buffers(h, false, &wk) < 0) return nullptr;
  return wk.stage[k];
}

int transposed_fisher_info_device(bbx_design* h, const double* d_weight,
                                  double* d_out) {
  if (h->sparse)
    return fail(BBX_ERR_INVALID,
                "compute_transposed_fisher_info: dense designs only (this one "
                "is sparse)");
  BBX_HIP(hipSetDevice(h->device));
  WbWork wk;
  BBX_TRY(wb_buffers(h, false, &wk));
  // the weights with zeros past P (the kernel reads whole quads up to ld)
  BBX_HIP(hipMemsetAsync(wk.d, 0, sizeof(double) * (size_t)wb_pd(h), h->stream));
  BBX_HIP(hipMemcpyAsync(wk.d, d_weight, sizeof(double) * (size_t)h->P,
                         hipMemcpyDeviceToDevice, h->stream));
  return wb_gram_device(h, wk.d, nullptr, d_out, h->n);
}

// ---- q x q on the host ------------------------------------------------------
// lower Cholesky factor in place (row-major q x q); false when not > 0
static bool host_chol(std::vector<double>& a, int q) {
  for (int j = 0; j < q; ++j) {
    double p = a[j * q + j];
    for (int k = 0; k < j; ++k) p -= a[j * q + k] * a[j * q + k];
    if (!(p > 0.) || !std::isfinite(p)) return false;
    p = std::sqrt(p);
    a[j * q + j] = p;
    for (int i = j + 1; i < q; ++i) {
      double v = a[i * q + j];
      for (int k = 0; k < j; ++k) v -= a[i * q + k] * a[j * q + k];
      a[i * q + j] = v / p;
    }
  }
  return true;
}
static void host_fwd(const std::vector<double>& L, int q, double* x) {
  for (int i = 0; i < q; ++i) {
    double v = x[i];
    for (int k = 0; k < i; ++k) v -= L[i * q + k] * x[k];
    x[i] = v / L[i * q + i];
  }
}
static void host_bwd(const std::vector<double>& L, int q, double* x) {
  for (int i = q - 1; i >= 0; --i) {
    double v = x[i];
    for (int k = i + 1; k < q; ++k) v -= L[k * q + i] * x[k];
    x[i] = v / L[i * q + i];
  }
}

// The draw.  d_obs_prec[n], or nullptr: one number for every row, *d_obs_scalar
// when that device pointer is given, else obs_scalar.  d_pps[P]: 1 / prior sd,
// zeros marking the flat coefficients.  d_y[n]: the (pseudo-)outcome, or with
// y_is_wy != 0 obs_prec .* y (the logit chain's kappa).  d_delta[n], d_xi[P]:
// standard normals (xi[j] belongs to coefficient j).  Synchronises the stream.
int woodbury_sample_device(bbx_design* h, const double* d_obs_prec,
                           double obs_scalar, const double* d_obs_scalar,
                           const double* d_pps, const double* d_y, int y_is_wy,
                           const double* d_delta, const double* d_xi,
                           double* d_coef_out) {
  if (h->sparse)
    return fail(BBX_ERR_INVALID,
                "the woodbury sampler needs a dense design (this one is sparse)");
  BBX_HIP(hipSetDevice(h->device));
  WbWork wk;
  BBX_TRY(wb_buffers(h, true, &wk));
  const int64_t n = h->n, P = h->P, n_pad = wb_npad(h), Pd = wb_pd(h);
  const int nb = (int)(n_pad / WB);
  hipStream_t st = h->stream;
  double* M = h->chol_A.as<double>();
  const int* const saved_skip = h->skip_flag;
  h->skip_flag = nullptr;
  struct Restore {
    bbx_design* h;
    const int* f;
    ~Restore() { h->skip_flag = f; }
  } restore{h, saved_skip};

  BBX_LAUNCH(wb_reset_kernel, dim3(1), dim3(1), 0, st, wk.count_idx, wk.info);
  BBX_LAUNCH(wb_prep_kernel, dim3(wb_blocks(Pd)), dim3(256), 0, st, P, Pd, d_pps,
             d_xi, wk.d, wk.u, wk.count_idx);
  BBX_LAUNCH(wb_rows_kernel, dim3(wb_blocks(n_pad)), dim3(256), 0, st, n, n_pad,
             d_obs_prec, obs_scalar, d_obs_prec ? nullptr : d_obs_scalar, d_y,
             y_is_wy, wk.s, wk.alpha);
  int ci[2 + WB_QMAX];
  BBX_HIP(hipMemcpyAsync(ci, wk.count_idx, sizeof(ci), hipMemcpyDeviceToHost, st));
  // (the Gram does not depend on which coefficients are flat: enqueue it
  // before the host waits for the list)
  BBX_TRY(wb_gram_device(h, wk.d, wk.s, M, n_pad));
  BBX_TRY(chol_factor_enqueue(st, M, n_pad, nb, wk.info));
  BBX_HIP(hipStreamSynchronize(st));
  if (ci[1] > 0)
    return fail(BBX_ERR_INVALID,
                "woodbury: prior_prec_sqrt has a negative or NaN entry");
  const int q = ci[0];
  if (q > WB_QMAX)
    return fail(BBX_ERR_INVALID,
                "woodbury: more than " + std::to_string(WB_QMAX) +
                    " coefficients with a flat prior (prior_prec_sqrt == 0)");
  if (q > n)
    return fail(BBX_ERR_NUMERIC,
                "woodbury: more flat coefficients than observations");
  WbIdx idx{};
  std::sort(ci + 2, ci + 2 + q);
  for (int k = 0; k < q; ++k) idx.v[k] = ci[2 + k];
  double* r0 = wk.phiF + (size_t)q * n_pad;

  // r0 = alpha - Phi_R u - delta
  BBX_TRY(launch_dot_dense(h, wk.u, wk.s, wk.t));
  BBX_LAUNCH(wb_resid_kernel, dim3(wb_blocks(n_pad)), dim3(256), 0, st, n, n_pad,
             wk.alpha, wk.t, d_delta, r0);
  std::vector<double> C, LC;
  std::vector<double> sm((size_t)(WB_QMAX + 1) * (WB_QMAX + 1));
  WbCoef cf{};
  const double* rhs0 = r0;
  if (q > 0) {
    if (h->dense_dtype == BBX_F32)
      BBX_LAUNCH(wb_phif_kernel<float>, dim3(wb_blocks(n_pad), q), dim3(256), 0,
                 st, h->dense.as<float>(), h->dense_ld, n, n_pad, idx, wk.s,
                 wk.phiF);
    else
      BBX_LAUNCH(wb_phif_kernel<double>, dim3(wb_blocks(n_pad), q), dim3(256), 0,
                 st, h->dense.as<double>(), h->dense_ld, n, n_pad, idx, wk.s,
                 wk.phiF);
    // [C | g] = Phi_F^T [Phi_F | r0]
    BBX_LAUNCH(wb_inner_kernel, dim3(q, q + 1), dim3(256), 0, st, n_pad, n_pad,
               wk.phiF, wk.phiF, q + 1, wk.small);
    BBX_HIP(hipMemcpyAsync(sm.data(), wk.small, sizeof(double) * q * (q + 1),
                           hipMemcpyDeviceToHost, st));
    BBX_HIP(hipStreamSynchronize(st));
    LC.assign((size_t)q * q, 0.);
    std::vector<double> g(q);
    for (int a = 0; a < q; ++a) {
      for (int b = 0; b < q; ++b) LC[a * q + b] = sm[a * (q + 1) + b];
      g[a] = sm[a * (q + 1) + q];
    }
    if (!host_chol(LC, q))
      return fail(BBX_ERR_NUMERIC,
                  "woodbury: the columns with a flat prior are not linearly "
                  "independent (Phi_F^T Phi_F is not positive definite)");
    host_fwd(LC, q, g.data());
    host_bwd(LC, q, g.data());
    for (int k = 0; k < q; ++k) cf.v[k] = -g[k];
    // r = r0 - Phi_F C^-1 g  -> wk.w (a right-hand side; the solves destroy b)
    BBX_LAUNCH(wb_lincomb_kernel, dim3(wb_blocks(n_pad)), dim3(256), 0, st, n_pad,
               n_pad, r0, wk.phiF, q, cf, nullptr, wk.w);
    rhs0 = wk.w;
  }
  // Z = M^-1 [r | Phi_F]
  for (int c = 0; c <= q; ++c) {
    const double* src = c == 0 ? rhs0 : wk.phiF + (size_t)(c - 1) * n_pad;
    BBX_HIP(hipMemcpyAsync(wk.b, src, sizeof(double) * (size_t)n_pad,
                           hipMemcpyDeviceToDevice, st));
    BBX_TRY(chol_solve_enqueue(st, M, n_pad, nb, wk.b, wk.y,
                               wk.Z + (size_t)c * n_pad));
  }
  if (q > 0) {
    // [h | S] = Phi_F^T Z
    BBX_LAUNCH(wb_inner_kernel, dim3(q, q + 1), dim3(256), 0, st, n_pad, n_pad,
               wk.phiF, wk.Z, q + 1, wk.small);
    BBX_HIP(hipMemcpyAsync(sm.data(), wk.small, sizeof(double) * q * (q + 1),
                           hipMemcpyDeviceToHost, st));
    BBX_HIP(hipStreamSynchronize(st));
    std::vector<double> S((size_t)q * q), hv(q);
    for (int a = 0; a < q; ++a) {
      for (int b = 0; b < q; ++b)
        S[a * q + b] = .5 * (sm[a * (q + 1) + 1 + b] + sm[b * (q + 1) + 1 + a]);
      hv[a] = sm[a * (q + 1)];
    }
    if (!host_chol(S, q))
      return fail(BBX_ERR_NUMERIC,
                  "woodbury: Phi_F^T M^-1 Phi_F is not positive definite");
    host_fwd(S, q, hv.data());
    host_bwd(S, q, hv.data());
    for (int k = 0; k < q; ++k) cf.v[k] = -hv[k];
  }
  // w = Z_r + Z_F lambda, then s .* w for X~^T
  BBX_LAUNCH(wb_lincomb_kernel, dim3(wb_blocks(n)), dim3(256), 0, st, n, n_pad,
             wk.Z, wk.Z + n_pad, q, cf, wk.s, wk.t);
  TdotEpilogue ep;
  BBX_TRY(launch_tdot_dense(h, wk.t, nullptr, ep, wk.g));
  BBX_LAUNCH(wb_beta_r_kernel, dim3(wb_blocks(P)), dim3(256), 0, st, P, wk.u,
             wk.d, wk.g, d_coef_out);
  if (q > 0) {
    // beta_F = C^-1 Phi_F^T (alpha - Phi_R beta_R) + chol(C)^-T xi_F
    BBX_TRY(launch_dot_dense(h, d_coef_out, wk.s, wk.t));
    BBX_LAUNCH(wb_resid_kernel, dim3(wb_blocks(n_pad)), dim3(256), 0, st, n,
               n_pad, wk.alpha, wk.t, nullptr, wk.b);
    BBX_LAUNCH(wb_inner_kernel, dim3(q, 1), dim3(256), 0, st, n_pad, n_pad,
               wk.phiF, wk.b, 1, wk.small);
    std::vector<double> g2(q), xf(q);
    BBX_HIP(hipMemcpyAsync(g2.data(), wk.small, sizeof(double) * q,
                           hipMemcpyDeviceToHost, st));
    for (int k = 0; k < q; ++k)
      BBX_HIP(hipMemcpyAsync(&xf[k], d_xi + idx.v[k], sizeof(double),
                             hipMemcpyDeviceToHost, st));
    BBX_HIP(hipStreamSynchronize(st));
    host_fwd(LC, q, g2.data());
    host_bwd(LC, q, g2.data());
    host_bwd(LC, q, xf.data());
    for (int k = 0; k < q; ++k) cf.v[k] = g2[k] + xf[k];
    BBX_LAUNCH(wb_scatter_kernel, dim3(1), dim3(64), 0, st, q, idx, cf,
               d_coef_out);
  }
  BBX_HIP(hipGetLastError());
  int bad = WB_NO_FAIL;
  BBX_HIP(hipMemcpyAsync(&bad, wk.info, sizeof(int), hipMemcpyDeviceToHost, st));
  BBX_HIP(hipStreamSynchronize(st));
  if (bad != WB_NO_FAIL)
    return fail(BBX_ERR_NUMERIC,
                "woodbury: Phi D Phi^T + I is not positive definite (pivot " +
                    std::to_string(bad) + " is not > 0)");
  return BBX_OK;
}

void woodbury_release(bbx_design* h) { h->wb_vec.release(); }

}  // namespace bbx
