// Posterior survival of new rows from draws of the linear predictor and of the
// log cumulative baseline hazard (bbx_<fam>_baseline_hazard, cox_family.hpp):
//
//   S[i][t][d] = exp(-exp(log_hazard[d][g_i][t] + eta[d][i]))
//   mean[i][t] = (sum_d S) / n_draw,  sd[i][t] = sqrt((sum_d (S - mean)^2) / n_draw)
//
// The exponent is formed as that one sum, so neither factor overflows alone:
// a log_hazard of -inf gives exp(-0) = 1 exactly, an exponent past 709 gives
// exp(-inf) = 0 exactly, a NaN stays a NaN.  Family-independent: no handle,
// host pointers only.
//
// One thread per (row, time): the rows of a workgroup along the lanes (eta is
// draw-major, so a wave reads 64 consecutive doubles per draw), the time point
// from blockIdx.y.  The draws are walked in index order, once for the mean and
// once for the squared deviations (S is formed again, with the same bits).  No
// atomics: the same inputs give the same bits.  mean and sd are written n_time
// doubles apart across the lanes; the optional draws (row-major n_row x n_time
// x n_draw, the layout the caller reads) n_time n_draw doubles apart: that
// store does NOT coalesce, every lane touches a cache line of its own per
// draw.  It is the price of asking for the draws of a few rows; the summaries
// alone never pay it.
//
// log_hazard.  Without groups the value of a draw is the same for the whole
// workgroup: its address holds kernel arguments, blockIdx and the loop counter
// only, so the compiler loads it into a scalar register.  With groups the
// workgroup stages the values of its time point, all groups of a run of
// draws, in LDS (SURV_LDS doubles) and every lane picks its row's group from
// there; more than SURV_LDS groups are read from global memory lane by lane.
//
// Rows go through the device in slabs, sized so that eta, group, mean, sd and
// draws of one slab stay within SURV_BUDGET bytes; log_hazard (n_draw x
// n_group x n_time) is resident whole.
#include <math.h>

#include <string>

#include "common.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

using namespace bbx;

namespace {

constexpr int SURV_BLOCK = 256;
constexpr int SURV_LDS = 2048;                  // doubles: 16 KiB
constexpr size_t SURV_BUDGET = size_t(64) << 20;
constexpr int SURV_MAX_Y = 65535;

// dc: draws per LDS stage (GROUPS and n_group <= SURV_LDS), or 0
template <bool GROUPS>
__global__ __launch_bounds__(SURV_BLOCK) void cox_survival_kernel(
    int64_t n_row, int64_t n_time, int64_t n_draw, int64_t n_group, int dc,
    const double* __restrict__ eta, const double* __restrict__ lh,
    const int32_t* __restrict__ group, double* __restrict__ mean,
    double* __restrict__ sd, double* __restrict__ draws) {
  __shared__ double s_l[GROUPS ? SURV_LDS : 1];
  const int64_t i = (int64_t)blockIdx.x * SURV_BLOCK + threadIdx.x;
  const bool active = i < n_row;
  const int64_t g = GROUPS && active ? group[i] : 0;
  const int64_t step = dc > 0 ? dc : n_draw;
  for (int64_t t = blockIdx.y; t < n_time; t += gridDim.y) {
    double m = 0.;
    for (int pass = 0; pass < 2; ++pass) {
      double acc = 0.;
      for (int64_t d0 = 0; d0 < n_draw; d0 += step) {
        const int64_t d1 = d0 + step < n_draw ? d0 + step : n_draw;
        if (GROUPS && dc > 0) {
          __syncthreads();   // the previous stage has been read
          const int64_t cnt = (d1 - d0) * n_group;
          for (int64_t e = threadIdx.x; e < cnt; e += SURV_BLOCK)
            s_l[e] = lh[(d0 * n_group + e) * n_time + t];
          __syncthreads();
        }
        if (!active) continue;
        for (int64_t d = d0; d < d1; ++d) {
          double l;
          if (!GROUPS) {
            l = lh[d * n_time + t];
          } else if (dc > 0) {
            l = s_l[(d - d0) * n_group + g];
          } else {
            l = lh[(d * n_group + g) * n_time + t];
          }
          const double s = exp(-exp(l + eta[d * n_row + i]));
          if (pass == 0) {
            acc += s;
            if (draws) draws[(i * n_time + t) * n_draw + d] = s;
          } else {
            const double dv = s - m;
            acc += dv * dv;
          }
        }
      }
      if (pass == 0) {
        m = acc / (double)n_draw;
        if (active) mean[i * n_time + t] = m;
      } else if (active) {
        sd[i * n_time + t] = sqrt(acc / (double)n_draw);
      }
    }
  }
}

int survival_summary_impl(int device, int64_t n_row, int64_t n_time,
                          int64_t n_draw, int64_t n_group, const double* eta,
                          const double* log_hazard, const int32_t* group,
                          double* mean, double* sd, double* draws) {
  if (!eta || !log_hazard || !mean || !sd)
    return fail(BBX_ERR_INVALID, "NULL argument");
  if (n_row < 1) return fail(BBX_ERR_INVALID, "n_row must be at least 1");
  if (n_time < 1) return fail(BBX_ERR_INVALID, "n_time must be at least 1");
  if (n_draw < 1) return fail(BBX_ERR_INVALID, "n_draw must be at least 1");
  if (n_group < 1) return fail(BBX_ERR_INVALID, "n_group must be at least 1");
  if (n_group > 1 && !group)
    return fail(BBX_ERR_INVALID, "NULL group with n_group > 1");
  if (group) {
    // the kernel indexes log_hazard by it: check them all
    for (int64_t i = 0; i < n_row; ++i) {
      if (group[i] < 0 || group[i] >= n_group)
        return fail(BBX_ERR_INVALID, "group[" + std::to_string(i) +
                                         "] outside [0, n_group)");
    }
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(BBX_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= count)
    return fail(BBX_ERR_INVALID, "device index out of range");
  BBX_HIP(hipSetDevice(device));

  const size_t d8 = sizeof(double);
  const size_t per_row = d8 * (size_t)n_draw + 2 * d8 * (size_t)n_time +
                         sizeof(int32_t) +
                         (draws ? d8 * (size_t)n_time * (size_t)n_draw : 0);
  int64_t slab = (int64_t)(SURV_BUDGET / per_row);
  if (slab > SURV_BLOCK) slab -= slab % SURV_BLOCK;
  if (slab < 1) slab = 1;
  if (slab > n_row) slab = n_row;

  DevMem d_lh, d_eta, d_group, d_mean, d_sd, d_draws;
  const size_t lh_bytes = d8 * (size_t)n_draw * (size_t)n_group * (size_t)n_time;
  BBX_TRY(d_lh.alloc(lh_bytes));
  BBX_TRY(d_eta.alloc(d8 * (size_t)n_draw * (size_t)slab));
  if (group) BBX_TRY(d_group.alloc(sizeof(int32_t) * (size_t)slab));
  BBX_TRY(d_mean.alloc(d8 * (size_t)slab * (size_t)n_time));
  BBX_TRY(d_sd.alloc(d8 * (size_t)slab * (size_t)n_time));
  if (draws)
    BBX_TRY(d_draws.alloc(d8 * (size_t)slab * (size_t)n_time * (size_t)n_draw));
  BBX_HIP(hipMemcpy(d_lh.ptr, log_hazard, lh_bytes, hipMemcpyHostToDevice));

  const bool groups = n_group > 1;
  const int dc = groups && n_group <= SURV_LDS ? (int)(SURV_LDS / n_group) : 0;
  const int gy = (int)(n_time < SURV_MAX_Y ? n_time : SURV_MAX_Y);
  for (int64_t r0 = 0; r0 < n_row; r0 += slab) {
    const int64_t len = r0 + slab < n_row ? slab : n_row - r0;
    // rows r0 .. r0 + len - 1 of every draw: the slab's eta is n_draw x len
    BBX_HIP(hipMemcpy2D(d_eta.ptr, d8 * (size_t)len, eta + r0,
                        d8 * (size_t)n_row, d8 * (size_t)len, (size_t)n_draw,
                        hipMemcpyHostToDevice));
    if (groups)
      BBX_HIP(hipMemcpy(d_group.ptr, group + r0, sizeof(int32_t) * (size_t)len,
                        hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((len + SURV_BLOCK - 1) / SURV_BLOCK), gy);
    if (groups) {
      BBX_LAUNCH(cox_survival_kernel<true>, grid, dim3(SURV_BLOCK), 0, 0, len,
                 n_time, n_draw, n_group, dc, d_eta.as<const double>(),
                 d_lh.as<const double>(), d_group.as<const int32_t>(),
                 d_mean.as<double>(), d_sd.as<double>(), d_draws.as<double>());
    } else {
      BBX_LAUNCH(cox_survival_kernel<false>, grid, dim3(SURV_BLOCK), 0, 0, len,
                 n_time, n_draw, n_group, 0, d_eta.as<const double>(),
                 d_lh.as<const double>(), nullptr, d_mean.as<double>(),
                 d_sd.as<double>(), d_draws.as<double>());
    }
    BBX_HIP(hipGetLastError());
    const size_t cells = (size_t)len * (size_t)n_time;
    const size_t at = (size_t)r0 * (size_t)n_time;
    BBX_HIP(hipMemcpy(mean + at, d_mean.ptr, d8 * cells, hipMemcpyDeviceToHost));
    BBX_HIP(hipMemcpy(sd + at, d_sd.ptr, d8 * cells, hipMemcpyDeviceToHost));
    if (draws)
      BBX_HIP(hipMemcpy(draws + at * (size_t)n_draw, d_draws.ptr,
                        d8 * cells * (size_t)n_draw, hipMemcpyDeviceToHost));
  }
  return BBX_OK;
}

}  // namespace

extern "C" int bbx_cox_survival_summary(int device, int64_t n_row,
                                        int64_t n_time, int64_t n_draw,
                                        int64_t n_group, const double* eta,
                                        const double* log_hazard,
                                        const int32_t* group, double* mean,
                                        double* sd, double* draws) {
  return no_throw([&]() -> int {
    return survival_summary_impl(device, n_row, n_time, n_draw, n_group, eta,
                                 log_hazard, group, mean, sd, draws);
  });
}
