// The probit model's latent update: z_i | beta ~ N(psi_i, 1) restricted to
// z > 0 (y_i = 1) or z <= 0 (y_i = 0) -- Albert & Chib (1993) -- drawn by the
// rejection sampler TruncatedNormal (samplers.hpp), with the log-likelihood
// sum_i log Phi(+-psi_i) and sum_i z_i, the centring term of X~^T z, collected
// on the way.  The stand-alone sampler bbx_device_truncated_normal lives here
// too.
//
// One lane per row.  A trial is one Philox block, one log and either a sqrt
// and a cospi or an exp; every trial is accepted with probability >= 1/2, so
// a wave of 64 rows waits ~7 trials for its slowest lane.  Trial t of element i
// reads Philox(seed, stream, i, t): the draw is a function of (seed, stream,
// i, psi_i, y_i) alone, whatever the grid.
#include <cmath>

#include "chain.hpp"
#include "philox.hpp"
#include "samplers.hpp"

namespace bbx {

namespace {

__device__ inline double probit_draw(uint64_t seed, uint64_t stream, int64_t i,
                                     double psi, bool positive) {
  if (!(fabs(psi) <= 1.7e308)) return psi - psi;
  return TruncatedNormal::draw_trials(
      [&](uint32_t t) { return Philox(seed, stream, (uint64_t)i, t); }, psi,
      positive, nullptr);
}

// block totals of two lane values (thread 0 holds them), fixed order
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

// ll_part[b], z_part[b]: block b's sums of log Phi(s_i psi_i) and of z_i.
__global__ __launch_bounds__(256) void chain_probit_kernel(
    int64_t n, uint64_t seed, uint64_t stream, const double* __restrict__ y,
    const double* __restrict__ psi, double* __restrict__ latent,
    double* __restrict__ ll_part, double* __restrict__ z_part) {
  double ll = 0., zs = 0.;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    const double eta = psi[i];
    const bool positive = y[i] != 0.;
    const double z = probit_draw(seed, stream, i, eta, positive);
    latent[i] = z;
    zs += z;
    ll += log_norm_cdf(positive ? eta : -eta);
  }
  block_totals_256(ll, zs);
  if (threadIdx.x == 0) {
    ll_part[blockIdx.x] = ll;
    z_part[blockIdx.x] = zs;
  }
}

__global__ __launch_bounds__(256) void dev_truncated_normal_kernel(
    int64_t n, uint64_t seed, const double* __restrict__ psi,
    const unsigned char* __restrict__ positive, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256)
    out[i] = probit_draw(seed, STREAM_LATENT, i, psi[i], positive[i] != 0);
}

int row_grid(int64_t n) {
  int64_t nb = (n + 255) / 256;
  if (nb > ROW_GRID) nb = ROW_GRID;
  if (nb < 1) nb = 1;
  return (int)nb;
}

}  // namespace

int launch_chain_probit(bbx_chain* c, uint64_t stream, int* row_blocks) {
  bbx_design* h = c->h;
  const int rg = row_grid(h->n);
  double* rp = c->row_part.as<double>();
  BBX_LAUNCH(chain_probit_kernel, dim3(rg), dim3(256), 0, h->stream, h->n,
             c->seed, stream, c->outcome.as<double>(), c->psi.as<double>(),
             c->latent.as<double>(), rp, rp + ROW_GRID);
  BBX_HIP(hipGetLastError());
  BBX_TRY(launch_sumw_fold(h, rp + ROW_GRID, rg));
  if (row_blocks) *row_blocks = rg;
  return BBX_OK;
}

}  // namespace bbx

using namespace bbx;

static int device_truncated_normal_impl(int device, uint64_t seed,
                                        int64_t n_draw, const double* psi,
                                        const unsigned char* positive,
                                        double* out) {
  const char* who = "bbx_device_truncated_normal: ";
  if (n_draw < 0) return fail(BBX_ERR_INVALID, std::string(who) + "n_draw < 0");
  if (!psi || !positive || !out)
    return fail(BBX_ERR_INVALID, std::string(who) + "NULL argument");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(BBX_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= count)
    return fail(BBX_ERR_INVALID, std::string(who) + "device index out of range");
  if (n_draw == 0) return BBX_OK;
  BBX_HIP(hipSetDevice(device));
  DevMem dp, ds, dout;
  BBX_TRY(dp.alloc(sizeof(double) * (size_t)n_draw));
  BBX_TRY(ds.alloc((size_t)n_draw));
  BBX_TRY(dout.alloc(sizeof(double) * (size_t)n_draw));
  BBX_HIP(hipMemcpy(dp.ptr, psi, sizeof(double) * (size_t)n_draw,
                    hipMemcpyHostToDevice));
  BBX_HIP(hipMemcpy(ds.ptr, positive, (size_t)n_draw, hipMemcpyHostToDevice));
  // (the chain's grid: from ROW_GRID x 256 rows on a lane takes a second row)
  BBX_LAUNCH(dev_truncated_normal_kernel, dim3(row_grid(n_draw)), dim3(256), 0,
             0, n_draw, seed, dp.as<double>(), ds.as<unsigned char>(),
             dout.as<double>());
  BBX_HIP(hipGetLastError());
  BBX_HIP(hipMemcpy(out, dout.ptr, sizeof(double) * (size_t)n_draw,
                    hipMemcpyDeviceToHost));
  return BBX_OK;
}

extern "C" int bbx_device_truncated_normal(int device, uint64_t seed,
                                           int64_t n_draw, const double* psi,
                                           const unsigned char* positive,
                                           double* out) {
  return no_throw([&]() -> int {
    return device_truncated_normal_impl(device, seed, n_draw, psi, positive,
                                        out);
  });
}
