// The censored-outcome model's latent update (log-normal AFT, Tobit): each row
// has a value b_i and a status -- 0 observed (z_i = b_i), 1 right-censored
// (z_i > b_i), 2 left-censored (z_i <= b_i) -- and z_i ~ N(psi_i, 1 / tau).  A
// censored row's latent is a truncated normal (Chib 1992): with psi' = (psi_i -
// b_i) sqrt(tau), u ~ N(psi', 1) on u > 0 (status 1) or u <= 0 (status 2) by the
// rejection sampler TruncatedNormal (samplers.hpp), used as it is, and z_i =
// b_i + u / sqrt(tau).  The same pass collects the log-likelihood
//   observed        1/2 log tau - 1/2 tau (b - psi)^2     (-1/2 log 2 pi dropped)
//   right-censored  log Phi(psi')
//   left-censored   log Phi(-psi')
// and sum_i z_i, the centring term of X~^T z.  tau is drawn beforehand by the
// linear model's kernels with z for y (chain.hip).  The stand-alone sampler
// bbx_device_censored_normal lives here too.
//
// One lane per row.  An observed lane copies its value and takes no trial; a
// censored lane's trial is one Philox block, accepted with probability >= 1/2
// (psi' on the allowed side) or >= 0.76 (Robert's exponential), so a wave
// waits for its slowest censored lane while its observed lanes sit idle: the
// cost follows the waves that hold a censored row, not the censored share.
// Trial t of row i reads Philox(seed, stream, i, t): the draw is a function of
// (seed, stream, i, psi_i, b_i, status_i, tau) alone, whatever the grid.
#include <cmath>

#include "chain.hpp"
#include "philox.hpp"
#include "samplers.hpp"

namespace bbx {

namespace {

// The latent of one row and its log-likelihood term.  rt = sqrt(tau), hlt =
// 1/2 log tau.  A psi' that is not finite (psi_i not finite, or the product
// out of range) gives a NaN term and, on a censored row, a NaN latent; no row
// loops on one.
__device__ inline double censored_row(uint64_t seed, uint64_t stream, int64_t i,
                                      double psi, double b, unsigned status,
                                      double tau, double rt, double hlt,
                                      double* term) {
  const double p = (psi - b) * rt;
  const bool bad = !(fabs(p) <= 1.7e308);
  if (status == 0) {
    *term = bad ? p - p : hlt - 0.5 * (p * p);
    return b;
  }
  if (bad) {
    *term = p - p;
    return p - p;
  }
  const bool positive = status == 1;
  *term = log_norm_cdf(positive ? p : -p);
  const double u = TruncatedNormal::draw_trials(
      [&](uint32_t t) { return Philox(seed, stream, (uint64_t)i, t); }, p,
      positive, nullptr);
  return b + u / rt;
}

// block totals of two lane values (thread 0 holds them), fixed order
__device__ inline void block_totals(double& a, double& b) {
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

// ll_part[b], z_part[b]: block b's sums of the log-likelihood terms and of z_i,
// under the tau in sc->obs_prec.
__global__ __launch_bounds__(256) void chain_censored_kernel(
    int64_t n, uint64_t seed, uint64_t stream,
    const ChainScalars* __restrict__ sc, const double* __restrict__ bound,
    const unsigned char* __restrict__ status, const double* __restrict__ psi,
    double* __restrict__ latent, double* __restrict__ ll_part,
    double* __restrict__ z_part) {
  const double tau = sc->obs_prec;
  const double rt = sqrt(tau);
  const double hlt = 0.5 * log(tau);
  double ll = 0., zs = 0.;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    double term;
    const double z = censored_row(seed, stream, i, psi[i], bound[i], status[i],
                                  tau, rt, hlt, &term);
    latent[i] = z;
    zs += z;
    ll += term;
  }
  block_totals(ll, zs);
  if (threadIdx.x == 0) {
    ll_part[blockIdx.x] = ll;
    z_part[blockIdx.x] = zs;
  }
}

__global__ __launch_bounds__(256) void dev_censored_normal_kernel(
    int64_t n, uint64_t seed, double tau, const double* __restrict__ psi,
    const double* __restrict__ bound, const unsigned char* __restrict__ status,
    double* __restrict__ out) {
  const double rt = sqrt(tau);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    double term;
    out[i] = censored_row(seed, STREAM_LATENT, i, psi[i], bound[i], status[i],
                          tau, rt, 0., &term);
  }
}

int row_grid(int64_t n) {
  int64_t nb = (n + 255) / 256;
  if (nb > ROW_GRID) nb = ROW_GRID;
  if (nb < 1) nb = 1;
  return (int)nb;
}

}  // namespace

int launch_chain_censored(bbx_chain* c, uint64_t stream, int* row_blocks) {
  bbx_design* h = c->h;
  const int rg = row_grid(h->n);
  double* rp = c->row_part.as<double>();
  BBX_LAUNCH(chain_censored_kernel, dim3(rg), dim3(256), 0, h->stream, h->n,
             c->seed, stream, c->scalars.as<ChainScalars>(),
             c->outcome.as<double>(), c->status.as<unsigned char>(),
             c->psi.as<double>(), c->latent.as<double>(), rp, rp + ROW_GRID);
  BBX_HIP(hipGetLastError());
  BBX_TRY(launch_sumw_fold(h, rp + ROW_GRID, rg));
  if (row_blocks) *row_blocks = rg;
  return BBX_OK;
}

}  // namespace bbx

using namespace bbx;

static int device_censored_normal_impl(int device, uint64_t seed,
                                       int64_t n_draw, const double* psi,
                                       const double* bound,
                                       const unsigned char* status, double tau,
                                       double* out) {
  const char* who = "bbx_device_censored_normal: ";
  if (n_draw < 0) return fail(BBX_ERR_INVALID, std::string(who) + "n_draw < 0");
  if (!psi || !bound || !status || !out)
    return fail(BBX_ERR_INVALID, std::string(who) + "NULL argument");
  if (!(tau > 0.) || !std::isfinite(tau))
    return fail(BBX_ERR_INVALID,
                std::string(who) + "tau must be finite and positive");
  for (int64_t i = 0; i < n_draw; ++i) {
    if (status[i] > 2)
      return fail(BBX_ERR_INVALID, std::string(who) + "status[" +
                                       std::to_string(i) + "] is not 0, 1 or 2");
    if (!std::isfinite(bound[i]))
      return fail(BBX_ERR_INVALID, std::string(who) + "bound[" +
                                       std::to_string(i) + "] is not finite");
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(BBX_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= count)
    return fail(BBX_ERR_INVALID, std::string(who) + "device index out of range");
  if (n_draw == 0) return BBX_OK;
  BBX_HIP(hipSetDevice(device));
  const size_t nb = sizeof(double) * (size_t)n_draw;
  DevMem dp, db, ds, dout;
  BBX_TRY(dp.alloc(nb));
  BBX_TRY(db.alloc(nb));
  BBX_TRY(ds.alloc((size_t)n_draw));
  BBX_TRY(dout.alloc(nb));
  BBX_HIP(hipMemcpy(dp.ptr, psi, nb, hipMemcpyHostToDevice));
  BBX_HIP(hipMemcpy(db.ptr, bound, nb, hipMemcpyHostToDevice));
  BBX_HIP(hipMemcpy(ds.ptr, status, (size_t)n_draw, hipMemcpyHostToDevice));
  // (the chain's grid: from ROW_GRID x 256 rows on a lane takes a second row)
  BBX_LAUNCH(dev_censored_normal_kernel, dim3(row_grid(n_draw)), dim3(256), 0,
             0, n_draw, seed, tau, dp.as<double>(), db.as<double>(),
             ds.as<unsigned char>(), dout.as<double>());
  BBX_HIP(hipGetLastError());
  BBX_HIP(hipMemcpy(out, dout.ptr, nb, hipMemcpyDeviceToHost));
  return BBX_OK;
}

extern "C" int bbx_device_censored_normal(int device, uint64_t seed,
                                          int64_t n_draw, const double* psi,
                                          const double* bound,
                                          const unsigned char* status,
                                          double tau, double* out) {
  return no_throw([&]() -> int {
    return device_censored_normal_impl(device, seed, n_draw, psi, bound, status,
                                       tau, out);
  });
}
