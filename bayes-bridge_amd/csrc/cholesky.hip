// Dense designs: the direct ('cholesky') draw of the coefficients
// (direct_gaussian_sampler.py:4-44) and the weighted Gram it needs
// (dense_matrix.py:54-58).
//
//   F    = X~^T diag(w) X~                    gram_tiles_kernel + gram_reduce_kernel
//   d    = pps^2 + diag(F),  s = 1/sqrt(d)    chol_scale_kernel
//   A    = diag(s) F diag(s) + diag((s pps)^2) chol_assemble_kernel (unit diagonal)
//   A    = L L^T   (L = U^T: the reference's upper factor, stored transposed)
//   y    = L^-1 (s .* v)                      trsv_fwd_kernel, one launch per block
//   x    = L^-T (y + g)                       trsv_bwd_kernel, one launch per block
//   coef = s .* x                             = s (A^-1 s v + U^-1 g)
//
// Everything is f64 and row-major with a leading dimension Pp = P rounded up to
// CB = 64; the padding of A is the identity, the padding of every vector zero, so
// no kernel of the factorisation or the solves needs a bound on P.
//
// Gram.  The output is cut into 64 x 64 tiles; only the tiles on and below the
// diagonal are computed (T = nb (nb + 1) / 2 of them).  A workgroup (4 waves)
// owns one tile and one chunk of rows; wave q takes every fourth group of four
// rows of the chunk and keeps 4 x 4 accumulators of v_mfma_f64_16x16x4_f64:
//   A[i][k] = X~[r + k][I0 + i]       lane l: X~[r + (l >> 4)][I0 + 16 ti + (l & 15)]
//   B[k][j] = w[r + k] X~[r + k][J0 + j]
//   D row = (l >> 4) + 4 reg, col = l & 15      (cdna_hip_programming.md "f64 MFMA")
// f32 storage is widened on load, so both storage types accumulate in f64.  The
// four waves are added in LDS in a fixed order and every (chunk, tile) partial
// goes to its own slot of a slab; gram_reduce_kernel adds the chunks in chunk
// order and writes the tile and its mirror.  No atomics: two calls on the same
// input give the same bits.  The slab is bounded (gram_slab_bytes): when the
// lower triangle does not fit, the tiles are processed in batches.
//
// Factorisation: right-looking, block 64.  Per block column k: chol_diag_kernel
// factors the diagonal block in LDS (one workgroup), chol_panel_kernel solves
// the panel below it (one workgroup per 64 rows) and chol_syrk_kernel subtracts
// L21 L21^T from the trailing lower tiles on the matrix cores (one workgroup per
// tile).  A pivot that is not > 0 (or is NaN) is recorded in `info` by atomicMin
// (integer: deterministic) and replaced by 1 so that nothing downstream faults;
// the caller reads `info` and reports the first such column.
//
// Solves.  Latency-bound: a single workgroup sweeping P would serialise P
// steps.  Instead every block step is one launch over many workgroups: each
// workgroup solves the 64 x 64 diagonal system in LDS (redundantly: 64 steps
// of LDS latency, cheaper than a second launch), workgroup 0 stores the block of
// the solution, and every workgroup subtracts that block's contribution from its
// own 64 rows of the remaining right-hand side -- forward: one wave per row,
// reading a row segment of L; backward: one thread per row, reading L^T's column
// segment, i.e. a contiguous row segment of L across the threads.
#include <math.h>

#include "common.hpp"

namespace bbx {

typedef double ch_d4 __attribute__((ext_vector_type(4)));
constexpr int CB = 64;                                     // tile / block size
// Bound of the Gram partials.  BBX_GRAM_SLAB_BYTES=<bytes> lowers it for the
// process (read per call; tests: the batched-tile path on a small design).
static size_t gram_slab_bytes() {
  const char* e = getenv("BBX_GRAM_SLAB_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? (size_t)v : size_t(256) << 20;
}
constexpr int CHOL_NO_FAIL = 0x7fffffff;

__device__ __forceinline__ ch_d4 ch_mfma(double a, double b, ch_d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void tile_of(int t, int* bi, int* bj) {
  // t -> (bi, bj), bi >= bj, row-major over the lower triangle
  int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((int64_t)i * (i + 1) / 2 > t) --i;
  while ((int64_t)(i + 1) * (i + 2) / 2 <= t) ++i;
  *bi = i;
  *bj = t - i * (i + 1) / 2;
}

// ---------------------------------------------------------------------------
// Gram partials: slab[chunk][tile - t0][64][64]
template <typename T>
__global__ __launch_bounds__(256) void gram_tiles_kernel(
    const T* __restrict__ X, int64_t ld, int64_t n, int64_t P,
    const double* __restrict__ w, int64_t rows_per_chunk, int t0, int nt,
    double* __restrict__ slab) {
  __shared__ double red[CB * CB];
  const int t = t0 + (int)blockIdx.x;
  int bi, bj;
  tile_of(t, &bi, &bj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, kk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = min(n, r0 + rows_per_chunk);
  int64_t colA[4], colB[4];
  bool okA[4], okB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    colA[q] = (int64_t)bi * CB + 16 * q + c;
    colB[q] = (int64_t)bj * CB + 16 * q + c;
    okA[q] = colA[q] < P;
    okB[q] = colB[q] < P;
  }
  ch_d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = ch_d4{0., 0., 0., 0.};
  for (int64_t r = r0 + 4 * wave; r < r1; r += 16) {
    const int64_t rr = r + kk;
    const bool rok = rr < r1;
    const double wr = rok ? (w ? w[rr] : 1.) : 0.;
    const T* row = X + rr * ld;
    double av[4], bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      av[q] = (rok && okA[q]) ? (double)row[colA[q]] : 0.;
      bv[q] = (rok && okB[q]) ? wr * (double)row[colB[q]] : 0.;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = ch_mfma(av[a], bv[b], acc[a][b]);
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
            const int i = 16 * a + kk + 4 * g, j = 16 * b + c;
            red[i * CB + j] = q == 0 ? acc[a][b][g] : red[i * CB + j] + acc[a][b][g];
          }
    }
    __syncthreads();
  }
  double* out = slab + ((size_t)blockIdx.y * nt + blockIdx.x) * (CB * CB);
  for (int e = threadIdx.x; e < CB * CB; e += 256) out[e] = red[e];
}

// F tiles of one batch = sum over chunks (in chunk order), and their mirrors
__global__ __launch_bounds__(256) void gram_reduce_kernel(
    const double* __restrict__ slab, int chunks, int t0, int nt,
    double* __restrict__ F, int64_t ldf) {
  const int t = t0 + (int)blockIdx.x;
  int bi, bj;
  tile_of(t, &bi, &bj);
  for (int e = threadIdx.x; e < CB * CB; e += 256) {
    double s = 0.;
    for (int k = 0; k < chunks; ++k)
      s += slab[((size_t)k * nt + blockIdx.x) * (CB * CB) + e];
    // a diagonal tile keeps its lower half: F is symmetric bit for bit
    if (bi == bj && e % CB > e / CB) continue;
    const int64_t i = (int64_t)bi * CB + e / CB, j = (int64_t)bj * CB + e % CB;
    F[i * ldf + j] = s;
    F[j * ldf + i] = s;
  }
}

// diag_only: slab[chunk][col] = sum over the chunk's rows of w x~^2
template <typename T>
__global__ __launch_bounds__(256) void gram_diag_kernel(
    const T* __restrict__ X, int64_t ld, int64_t n, int64_t P,
    const double* __restrict__ w, int64_t rows_per_chunk,
    double* __restrict__ slab) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = min(n, r0 + rows_per_chunk);
  double s = 0.;
  for (int64_t r = r0; r < r1; ++r) {
    const double x = (double)X[r * ld + j];
    s += (w ? w[r] : 1.) * x * x;
  }
  slab[(size_t)blockIdx.y * P + j] = s;
}

__global__ __launch_bounds__(256) void gram_diag_reduce_kernel(
    const double* __restrict__ slab, int chunks, int64_t P,
    double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  double s = 0.;
  for (int k = 0; k < chunks; ++k) s += slab[(size_t)k * P + j];
  out[j] = s;
}

// ---------------------------------------------------------------------------
// s = 1/sqrt(pps^2 + alpha F_ii), b = s .* v   (zero past P)
__global__ __launch_bounds__(256) void chol_scale_kernel(
    const double* __restrict__ F, int64_t ldf, double alpha,
    const double* d_alpha, int64_t P, int64_t Pp,
    const double* __restrict__ pps, const double* __restrict__ v,
    double* __restrict__ s, double* __restrict__ b) {
  if (d_alpha) alpha = *d_alpha;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Pp) return;
  if (i < P) {
    const double d = pps[i] * pps[i] + alpha * F[i * ldf + i];
    const double si = 1. / sqrt(d);
    s[i] = si;
    b[i] = si * v[i];
  } else {
    s[i] = 0.;
    b[i] = 0.;
  }
}

// lower triangle of A = s_i (alpha F_ij) s_j + [i == j] (s_i pps_i)^2; the
// padding is the identity.  F may alias A.
__global__ __launch_bounds__(256) void chol_assemble_kernel(
    const double* F, double alpha, const double* d_alpha, int64_t P,
    int64_t Pp, const double* __restrict__ pps, const double* __restrict__ s,
    double* A) {
  if (d_alpha) alpha = *d_alpha;
  const int64_t i = blockIdx.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= i;
       j += (int64_t)gridDim.x * 256) {
    double a;
    if (i < P) {
      a = s[i] * (alpha * F[i * Pp + j]) * s[j];
      if (i == j) {
        const double t = s[i] * pps[i];
        a += t * t;
      }
    } else {
      a = i == j ? 1. : 0.;
    }
    A[i * Pp + j] = a;
  }
}

__global__ void chol_info_reset_kernel(int* info) { *info = CHOL_NO_FAIL; }

// ---------------------------------------------------------------------------
// Diagonal block k, unblocked, in LDS
__global__ __launch_bounds__(256) void chol_diag_kernel(double* A, int64_t ld,
                                                        int k, int* info) {
  __shared__ double L[CB][CB + 1];
  __shared__ double piv;
  const int tid = threadIdx.x;
  double* blk = A + (int64_t)k * CB * ld + (int64_t)k * CB;
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e / CB, j = e % CB;
    L[i][j] = j <= i ? blk[i * ld + j] : 0.;
  }
  __syncthreads();
  for (int j = 0; j < CB; ++j) {
    if (tid == 0) {
      double p = L[j][j];
      if (!(p > 0.) || !isfinite(p)) {
        atomicMin(info, k * CB + j);
        p = 1.;
      }
      piv = sqrt(p);
      L[j][j] = piv;
    }
    __syncthreads();
    const double inv = 1. / piv;
    if (tid > j && tid < CB) L[tid][j] *= inv;
    __syncthreads();
    // trailing update of the columns j+1..63 (lower part)
    for (int e = tid; e < CB * CB; e += 256) {
      const int i = e / CB, m = e % CB;
      if (m > j && i >= m) L[i][m] -= L[i][j] * L[m][j];
    }
    __syncthreads();
  }
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e / CB, j = e % CB;
    if (j <= i) blk[i * ld + j] = L[i][j];
  }
}

// Panel below block k: rows of block (k + 1 + blockIdx.x), X L11^T = A21
__global__ __launch_bounds__(256) void chol_panel_kernel(double* A, int64_t ld,
                                                         int k) {
  __shared__ double L[CB][CB + 1];
  __shared__ double Xs[CB][CB + 1];
  const int tid = threadIdx.x;
  const double* d = A + (int64_t)k * CB * ld + (int64_t)k * CB;
  double* blk = A + (int64_t)(k + 1 + blockIdx.x) * CB * ld + (int64_t)k * CB;
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e / CB, j = e % CB;
    L[i][j] = d[i * ld + j];
    Xs[i][j] = blk[i * ld + j];
  }
  __syncthreads();
  for (int j = 0; j < CB; ++j) {
    if (tid < CB) Xs[tid][j] /= L[j][j];
    __syncthreads();
    for (int e = tid; e < CB * CB; e += 256) {
      const int i = e / CB, m = e % CB;
      if (m > j) Xs[i][m] -= Xs[i][j] * L[m][j];
    }
    __syncthreads();
  }
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e / CB, j = e % CB;
    blk[i * ld + j] = Xs[i][j];
  }
}

// Trailing update: tile (bi, bj) of the blocks after k, bi >= bj:
//   A[bi][bj] -= L[bi][k] L[bj][k]^T
// The two 64 x 64 panels pass through LDS in halves of 32 columns; wave q owns
// the 32 x 32 quadrant (q >> 1, q & 1) as 2 x 2 MFMA tiles.
__global__ __launch_bounds__(256) void chol_syrk_kernel(double* A, int64_t ld,
                                                        int k) {
  __shared__ double La[CB][33];
  __shared__ double Lb[CB][33];
  int ti, tj;
  tile_of((int)blockIdx.x, &ti, &tj);
  const int bi = k + 1 + ti, bj = k + 1 + tj;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, kk = lane >> 4;
  const int qi = (wave >> 1) * 32, qj = (wave & 1) * 32;
  const double* pa = A + (int64_t)bi * CB * ld + (int64_t)k * CB;
  const double* pb = A + (int64_t)bj * CB * ld + (int64_t)k * CB;
  ch_d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = ch_d4{0., 0., 0., 0.};
  for (int h = 0; h < 2; ++h) {
    for (int e = tid; e < CB * 32; e += 256) {
      const int i = e / 32, j = e % 32;
      La[i][j] = pa[i * ld + 32 * h + j];
      Lb[i][j] = pb[i * ld + 32 * h + j];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kx = 4 * ks + kk;
      double av[2], bv[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        av[q] = La[qi + 16 * q + c][kx];
        bv[q] = Lb[qj + 16 * q + c][kx];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ch_mfma(av[a], bv[b], acc[a][b]);
    }
    __syncthreads();
  }
  double* out = A + (int64_t)bi * CB * ld + (int64_t)bj * CB;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = qi + 16 * a + kk + 4 * g, j = qj + 16 * b + c;
        if (bi != bj || j <= i) out[i * ld + j] -= acc[a][b][g];
      }
}

// ---------------------------------------------------------------------------
// Forward step k of L y = b: y_k = L_kk^-1 b_k (every workgroup, LDS), then
// workgroup g subtracts L[rows of block k + 1 + g][block k] y_k from b.
__global__ __launch_bounds__(256) void trsv_fwd_kernel(const double* __restrict__ A,
                                                       int64_t ld, int k,
                                                       double* b, double* y) {
  __shared__ double L[CB][CB + 1];
  __shared__ double ys[CB];
  const int tid = threadIdx.x;
  const int64_t K0 = (int64_t)k * CB;
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e / CB, j = e % CB;
    L[i][j] = A[(K0 + i) * ld + K0 + j];
  }
  double acc = tid < CB ? b[K0 + tid] : 0.;
  __syncthreads();
  for (int j = 0; j < CB; ++j) {
    if (tid == j) ys[j] = acc / L[j][j];
    __syncthreads();
    if (tid > j && tid < CB) acc -= L[tid][j] * ys[j];
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < CB) y[K0 + tid] = ys[tid];
  const int64_t R0 = K0 + CB + (int64_t)blockIdx.x * CB;
  if (R0 >= ld) return;
  const int lane = tid & 63, wave = tid >> 6;
  const double yl = ys[lane];
  for (int r = wave; r < CB; r += 4) {
    const int64_t i = R0 + r;
    if (i >= ld) break;
    const double t = wave_allsum(A[i * ld + K0 + lane] * yl);
    if (lane == 0) b[i] -= t;
  }
}

// c = y + g (the normals enter the backward solve)
__global__ __launch_bounds__(256) void chol_add_kernel(const double* __restrict__ y,
                                                       const double* __restrict__ g,
                                                       int64_t P, int64_t Pp,
                                                       double* __restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < Pp) c[i] = y[i] + (i < P ? g[i] : 0.);
}

// Backward step k of L^T x = c: x_k = L_kk^-T c_k, then workgroup g subtracts
// L[block k][rows of block g]^T x_k from c (g < k).
__global__ __launch_bounds__(256) void trsv_bwd_kernel(const double* __restrict__ A,
                                                       int64_t ld, int k,
                                                       double* c, double* x) {
  __shared__ double L[CB][CB + 1];
  __shared__ double xs[CB];
  const int tid = threadIdx.x;
  const int64_t K0 = (int64_t)k * CB;
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e / CB, j = e % CB;
    L[i][j] = A[(K0 + i) * ld + K0 + j];
  }
  double acc = tid < CB ? c[K0 + tid] : 0.;
  __syncthreads();
  for (int j = CB - 1; j >= 0; --j) {
    if (tid == j) xs[j] = acc / L[j][j];
    __syncthreads();
    if (tid < j) acc -= L[j][tid] * xs[j];
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < CB) x[K0 + tid] = xs[tid];
  if ((int)blockIdx.x >= k) return;
  // 256 threads: 64 rows x 4 quarters of the block, added in a fixed order
  __shared__ double part[4][CB];
  const int r = tid & 63, qtr = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * CB + r;
  double s = 0.;
  for (int m = 16 * qtr; m < 16 * qtr + 16; ++m) s += A[(K0 + m) * ld + i] * xs[m];
  part[qtr][r] = s;
  __syncthreads();
  if (tid < CB)
    c[i] -= (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

__global__ __launch_bounds__(256) void chol_finish_kernel(
    const double* __restrict__ s, const double* __restrict__ x, int64_t P,
    double* __restrict__ coef) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < P) coef[i] = s[i] * x[i];
}

// ---------------------------------------------------------------------------
static inline unsigned blocks_of(int64_t m) { return (unsigned)((m + 255) / 256); }

static int64_t chol_ld(const bbx_design* h) { return (h->P + CB - 1) / CB * CB; }

// Row chunks of the Gram: enough workgroups for the device (>= ~2048 with the
// tiles), >= 512 rows each, at most 64 partial slabs.
static int gram_chunks(int64_t n, int64_t tiles) {
  int64_t c = (2048 + tiles - 1) / tiles;
  c = std::min<int64_t>(c, std::max<int64_t>(1, n / 512));
  return (int)std::max<int64_t>(1, std::min<int64_t>(c, 64));
}

// F = X~^T diag(w) X~ (w == nullptr: ones) into d_F, leading dimension ldf >= Pp;
// entries past P are zero.
static int gram_device(bbx_design* h, const double* d_w, double* d_F, int64_t ldf) {
  const int64_t Pp = chol_ld(h);
  const int nb = (int)(Pp / CB);
  const int64_t tiles = (int64_t)nb * (nb + 1) / 2;
  const int chunks = gram_chunks(h->n, tiles);
  const int64_t rows = (h->n + chunks - 1) / chunks;
  const int64_t per_tile = (int64_t)chunks * CB * CB * sizeof(double);
  const int64_t batch = std::max<int64_t>(
      1, std::min<int64_t>(tiles, (int64_t)gram_slab_bytes() / per_tile));
  const size_t need = (size_t)(batch * per_tile);
  if (h->chol_slab.bytes < need) {
    h->chol_slab.release();
    BBX_TRY(h->chol_slab.alloc(need));
  }
  double* slab = h->chol_slab.as<double>();
  for (int64_t t0 = 0; t0 < tiles; t0 += batch) {
    const int nt = (int)std::min<int64_t>(batch, tiles - t0);
    if (h->dense_dtype == BBX_F32)
      BBX_LAUNCH(gram_tiles_kernel<float>, dim3(nt, chunks), dim3(256), 0,
                 h->stream, h->dense.as<float>(), h->dense_ld, h->n, h->P, d_w,
                 rows, (int)t0, nt, slab);
    else
      BBX_LAUNCH(gram_tiles_kernel<double>, dim3(nt, chunks), dim3(256), 0,
                 h->stream, h->dense.as<double>(), h->dense_ld, h->n, h->P, d_w,
                 rows, (int)t0, nt, slab);
    BBX_LAUNCH(gram_reduce_kernel, dim3(nt), dim3(256), 0, h->stream, slab,
               chunks, (int)t0, nt, d_F, ldf);
  }
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

static int gram_diag_device(bbx_design* h, const double* d_w, double* d_out) {
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(64, h->n / 2048));
  const int64_t rows = (h->n + chunks - 1) / chunks;
  const size_t need = sizeof(double) * (size_t)chunks * (size_t)h->P;
  if (h->chol_slab.bytes < need) {
    h->chol_slab.release();
    BBX_TRY(h->chol_slab.alloc(need));
  }
  double* slab = h->chol_slab.as<double>();
  if (h->dense_dtype == BBX_F32)
    BBX_LAUNCH(gram_diag_kernel<float>, dim3(blocks_of(h->P), chunks), dim3(256),
               0, h->stream, h->dense.as<float>(), h->dense_ld, h->n, h->P, d_w,
               rows, slab);
  else
    BBX_LAUNCH(gram_diag_kernel<double>, dim3(blocks_of(h->P), chunks), dim3(256),
               0, h->stream, h->dense.as<double>(), h->dense_ld, h->n, h->P, d_w,
               rows, slab);
  BBX_LAUNCH(gram_diag_reduce_kernel, dim3(blocks_of(h->P)), dim3(256), 0,
             h->stream, slab, chunks, h->P, d_out);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

static int chol_buffers(bbx_design* h) {
  const int64_t Pp = chol_ld(h);
  const size_t mat = sizeof(double) * (size_t)Pp * (size_t)Pp;
  if (h->chol_A.bytes < mat) BBX_TRY(h->chol_A.alloc(mat));
  // s, b, y, c, x, then four staging vectors of the host entry point, then
  // the pivot flag
  if (h->chol_vec.bytes < sizeof(double) * 9 * (size_t)Pp + 64)
    BBX_TRY(h->chol_vec.alloc(sizeof(double) * 9 * (size_t)Pp + 64));
  return BBX_OK;
}

// staging vector k (0..3, Pp doubles each) of the host-pointer entry point
double* chol_stage(bbx_design* h, int k) {
  if (chol_buffers(h) < 0) return nullptr;
  return h->chol_vec.as<double>() + (size_t)(5 + k) * chol_ld(h);
}

int fisher_info_device(bbx_design* h, const double* d_w, int diag_only,
                       double* d_out) {
  if (h->sparse)
    return fail(BBX_ERR_INVALID,
                "compute_fisher_info: dense designs only (this one is sparse)");
  BBX_HIP(hipSetDevice(h->device));
  if (diag_only) return gram_diag_device(h, d_w, d_out);
  BBX_TRY(chol_buffers(h));
  const int64_t Pp = chol_ld(h);
  BBX_TRY(gram_device(h, d_w, h->chol_A.as<double>(), Pp));
  if (!d_out) return BBX_OK;   // the caller copies from chol_A
  BBX_HIP(hipMemcpy2DAsync(d_out, sizeof(double) * h->P, h->chol_A.ptr,
                           sizeof(double) * Pp, sizeof(double) * h->P, h->P,
                           hipMemcpyDeviceToDevice, h->stream));
  return BBX_OK;
}

// The draw.  d_obs_prec != nullptr: F = X~^T diag(obs_prec) X~ is formed for
// this call; else F = alpha (X~^T X~), the Gram cached on the handle (linear
// models; built on first use), with alpha = *d_obs_prec_scalar when that device
// pointer is given (the device chain's noise precision), else obs_prec_scalar.
// Synchronises the stream: on return d_coef_out is written, or the status says
// why not.
int chol_sample_device(bbx_design* h, const double* d_obs_prec,
                       double obs_prec_scalar, const double* d_obs_prec_scalar,
                       const double* d_pps,
                       const double* d_v, const double* d_normals,
                       double* d_coef_out) {
  if (h->sparse)
    return fail(BBX_ERR_INVALID,
                "the cholesky sampler needs a dense design (this one is sparse)");
  BBX_HIP(hipSetDevice(h->device));
  BBX_TRY(chol_buffers(h));
  const int64_t P = h->P, Pp = chol_ld(h);
  const int nb = (int)(Pp / CB);
  double* A = h->chol_A.as<double>();
  double* s = h->chol_vec.as<double>();
  double* b = s + Pp;
  double* y = b + Pp;
  double* c = y + Pp;
  double* x = c + Pp;
  int* info = reinterpret_cast<int*>(x + 5 * Pp);
  const double* F = A;
  double alpha = 1.;
  if (d_obs_prec) {
    BBX_TRY(gram_device(h, d_obs_prec, A, Pp));
  } else {
    if (!h->chol_gram_ready) {
      const size_t mat = sizeof(double) * (size_t)Pp * (size_t)Pp;
      if (h->chol_gram.bytes < mat) BBX_TRY(h->chol_gram.alloc(mat));
      BBX_TRY(gram_device(h, nullptr, h->chol_gram.as<double>(), Pp));
      h->chol_gram_ready = true;
    }
    F = h->chol_gram.as<double>();
    alpha = obs_prec_scalar;
  }
  BBX_LAUNCH(chol_info_reset_kernel, dim3(1), dim3(1), 0, h->stream, info);
  BBX_LAUNCH(chol_scale_kernel, dim3(blocks_of(Pp)), dim3(256), 0, h->stream,
             F, Pp, alpha, d_obs_prec ? nullptr : d_obs_prec_scalar, P, Pp,
             d_pps, d_v, s, b);
  BBX_LAUNCH(chol_assemble_kernel, dim3(blocks_of(Pp), (unsigned)Pp), dim3(256),
             0, h->stream, F, alpha, d_obs_prec ? nullptr : d_obs_prec_scalar,
             P, Pp, d_pps, s, A);
  for (int k = 0; k < nb; ++k) {
    BBX_LAUNCH(chol_diag_kernel, dim3(1), dim3(256), 0, h->stream, A, Pp, k, info);
    const int m = nb - k - 1;
    if (m > 0) {
      BBX_LAUNCH(chol_panel_kernel, dim3(m), dim3(256), 0, h->stream, A, Pp, k);
      BBX_LAUNCH(chol_syrk_kernel, dim3(m * (m + 1) / 2), dim3(256), 0,
                 h->stream, A, Pp, k);
    }
  }
  for (int k = 0; k < nb; ++k)
    BBX_LAUNCH(trsv_fwd_kernel, dim3(std::max(1, nb - k - 1)), dim3(256), 0,
               h->stream, A, Pp, k, b, y);
  BBX_LAUNCH(chol_add_kernel, dim3(blocks_of(Pp)), dim3(256), 0, h->stream, y,
             d_normals, P, Pp, c);
  for (int k = nb - 1; k >= 0; --k)
    BBX_LAUNCH(trsv_bwd_kernel, dim3(std::max(1, k)), dim3(256), 0, h->stream,
               A, Pp, k, c, x);
  BBX_LAUNCH(chol_finish_kernel, dim3(blocks_of(P)), dim3(256), 0, h->stream,
             s, x, P, d_coef_out);
  BBX_HIP(hipGetLastError());
  int bad = CHOL_NO_FAIL;
  BBX_HIP(hipMemcpyAsync(&bad, info, sizeof(int), hipMemcpyDeviceToHost,
                         h->stream));
  BBX_HIP(hipStreamSynchronize(h->stream));
  if (bad != CHOL_NO_FAIL)
    return fail(BBX_ERR_NUMERIC,
                "cholesky: the preconditioned precision matrix is not positive "
                "definite (pivot " + std::to_string(bad) + " is not > 0)");
  return BBX_OK;
}

// The factorisation and the solve for other callers (woodbury.hip), on a matrix
// of nb blocks of 64 with leading dimension ld whose padding is the identity.
// `info` must hold CHOL_NO_FAIL (0x7fffffff) before.
size_t gram_slab_limit() { return gram_slab_bytes(); }

int chol_factor_enqueue(hipStream_t st, double* A, int64_t ld, int nb, int* info) {
  for (int k = 0; k < nb; ++k) {
    BBX_LAUNCH(chol_diag_kernel, dim3(1), dim3(256), 0, st, A, ld, k, info);
    const int m = nb - k - 1;
    if (m > 0) {
      BBX_LAUNCH(chol_panel_kernel, dim3(m), dim3(256), 0, st, A, ld, k);
      BBX_LAUNCH(chol_syrk_kernel, dim3(m * (m + 1) / 2), dim3(256), 0, st, A,
                 ld, k);
    }
  }
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

// x = (L L^T)^-1 b; b is overwritten, y (ld doubles) is scratch, x != y != b
int chol_solve_enqueue(hipStream_t st, const double* A, int64_t ld, int nb,
                       double* b, double* y, double* x) {
  for (int k = 0; k < nb; ++k)
    BBX_LAUNCH(trsv_fwd_kernel, dim3(std::max(1, nb - k - 1)), dim3(256), 0, st,
               A, ld, k, b, y);
  for (int k = nb - 1; k >= 0; --k)
    BBX_LAUNCH(trsv_bwd_kernel, dim3(std::max(1, k)), dim3(256), 0, st, A, ld, k,
               y, x);
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

void chol_release(bbx_design* h) {
  woodbury_release(h);
  h->chol_A.release();
  h->chol_gram.release();
  h->chol_slab.release();
  h->chol_vec.release();
  h->chol_gram_ready = false;
}

}  // namespace bbx
