// The quantile regression model's updates after the coefficient draw.  At a
// fixed level q the asymmetric-Laplace likelihood q (1 - q) tau exp(-tau
// rho_q(y - psi)), rho_q(u) = u (q - 1[u < 0]), is a scale mixture of normals
// (Kozumi & Kobayashi 2011, written in the precision tau): with theta = (1 -
// 2q) / (q (1 - q)), kappa2 = 2 / (q (1 - q)), v_i ~ Exp(rate tau) and y_i |
// v_i ~ N(psi_i + theta v_i, kappa2 v_i / tau).  The stored latent is w_i = 1 /
// v_i; with r = y - psi,
//
//   pass A   S = sum_i [1 / w_i + w_i (r_i - theta / w_i)^2 / (2 kappa2)] with
//            the OLD w (every term positive)
//   tau      gamma_draw(3n/2) / S on STREAM_OBSVAR (one block)
//   pass B   w_i ~ InverseGaussian(mean 1 / (q (1 - q) |r_i|), shape tau / (2 q
//            (1 - q))) on STREAM_QMIX with the NEW tau (samplers.hpp); Omega_i =
//            tau w_i / kappa2, kappa_i = Omega_i y_i - tau theta / kappa2 (that
//            is Omega_i (y_i - theta / w_i) without the division), the block
//            sums of kappa and of the log-likelihood terms log tau - tau
//            rho_q(r_i)
//   finish   the log-likelihood partials summed in fixed order, plus n times
//            the row constant log(q (1 - q)) (chain.hip's finish kernel)
//
// tau is drawn before w, as in student_t.hip and for its reason: what an
// iteration leaves is a function of (beta, tau, seed, iteration), and a refresh
// reproduces it without a redraw of tau.
//
// Pass B is latent_rows.hpp's row kernel with this file's per-row expression,
// one lane per row.  The draw has no loop: one normal, one uniform and one
// data-dependent select per row, the same Philox consumption in every lane, so
// no lane of a wave waits for another.
#include <cmath>

#include "latent_rows.hpp"

namespace bbx {

namespace {

// What the kernels need of the level q, computed once on the host
struct QuantileLevel {
  double q;       // the level
  double qq;      // q (1 - q)
  double theta;   // (1 - 2q) / qq
  double kappa2;  // 2 / qq
};

inline QuantileLevel quantile_level(double q) {
  const double qq = q * (1. - q);
  return {q, qq, (1. - 2. * q) / qq, 2. / qq};
}

// rho_q(r) = r (q - 1[r < 0]) >= 0
__device__ inline double check_loss(double q, double r) {
  return r * (r < 0. ? q - 1. : q);
}

// pass A: part[b] = block b's sum of 1 / w_i + w_i (r_i - theta / w_i)^2 /
// (2 kappa2); `init`: of rho_q(r_i) instead (bbx_chain_init_obs_prec)
__global__ __launch_bounds__(256) void quantile_sum_kernel(
    int64_t n, QuantileLevel lv, int init, const double* __restrict__ y,
    const double* __restrict__ psi, const double* __restrict__ w,
    double* __restrict__ part) {
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    const double r = y[i] - psi[i];
    if (init) {
      acc += check_loss(lv.q, r);
    } else {
      const double wi = w[i];
      const double v = 1. / wi;
      const double d = r - lv.theta * v;
      acc += v + wi * (d * d) / (2. * lv.kappa2);
    }
  }
  const double tot = block_total_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// tau | beta, w ~ Gamma(3n/2, rate S) under the prior 1 / tau (single block);
// `init`: tau = n / S, the asymmetric-Laplace law's maximum-likelihood scale
__global__ __launch_bounds__(256) void quantile_tau_kernel(
    int64_t n, int init, uint64_t seed, uint64_t stream,
    const double* __restrict__ part, int count, ChainScalars* __restrict__ sc) {
  const double S = sum_row_parts(part, count);
  if (threadIdx.x != 0) return;
  if (init) {
    sc->obs_prec = (double)n / S;
    return;
  }
  Philox g(seed, stream, 0);
  sc->obs_prec = gamma_draw(g, 1.5 * (double)n) / S;
}

// pass B.  A residual that is not finite gives a NaN weight and a NaN term;
// |r| up to 1e150 gives a finite positive weight (the draw forms no square of
// m; its product s m stays finite far beyond that).
struct QuantileRows {
  QuantileLevel lv;
  const double* __restrict__ y;
  const double* __restrict__ psi;
  double* __restrict__ latent;
  double* __restrict__ obs_prec;
  double* __restrict__ kappa;
  static constexpr bool reads_tau = true;
  struct Once {
    double tau, lambda, lt, tk, shift;
  };
  __device__ Once once(double tau) const {
    const double tk = tau / lv.kappa2;
    return {tau, tau / (2. * lv.qq), log(tau), tk, tk * lv.theta};
  }
  __device__ void row(const Once& c, uint64_t seed, uint64_t stream, int64_t i,
                      double& ll, double& ks) const {
    const double yi = y[i];
    const double r = yi - psi[i];
    Philox g(seed, stream, (uint64_t)i);
    double wi = InverseGaussian::draw(g, lv.qq * fabs(r), c.lambda);
    double term = c.lt - c.tau * check_loss(lv.q, r);
    if (!(fabs(r) <= 1.7e308)) {
      wi = r - r;
      term = wi;
    }
    const double om = c.tk * wi;
    const double k = om * yi - c.shift;
    latent[i] = wi;
    obs_prec[i] = om;
    kappa[i] = k;
    ks = k;
    ll = term;
  }
};

// The stand-alone sampler's policy: m given, lambda where a family's tau goes
struct InverseGaussianDraws {
  const double* __restrict__ m;
  struct Once {
    double lambda;
  };
  __device__ Once once(double lambda) const { return {lambda}; }
  __device__ double draw(const Once& k, uint64_t seed, uint64_t stream,
                         int64_t i) const {
    Philox g(seed, stream, (uint64_t)i);
    return InverseGaussian::draw(g, m[i], k.lambda);
  }
};

}  // namespace

double quantile_row_const(double q) { return std::log(q * (1. - q)); }

int launch_quantile_tau(bbx_chain* c, uint64_t stream, bool init) {
  bbx_design* h = c->h;
  const int rg = row_grid(h->n);
  double* rp = c->row_part.as<double>();
  BBX_LAUNCH(quantile_sum_kernel, dim3(rg), dim3(256), 0, h->stream, h->n,
             quantile_level(c->quantile), init ? 1 : 0,
             c->outcome.as<double>(), c->psi.as<double>(),
             c->latent.as<double>(), rp);
  BBX_LAUNCH(quantile_tau_kernel, dim3(1), dim3(256), 0, h->stream, h->n,
             init ? 1 : 0, c->seed, stream, rp, rg,
             c->scalars.as<ChainScalars>());
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <>
int launch_latent_rows<BBX_MODEL_QUANTILE>(bbx_chain* c, uint64_t stream,
                                           int* row_blocks) {
  return launch_rows(
      c, stream,
      QuantileRows{quantile_level(c->quantile), c->outcome.as<double>(),
                   c->psi.as<double>(), c->latent.as<double>(),
                   c->obs_prec.as<double>(), c->kappa.as<double>()},
      row_blocks);
}

}  // namespace bbx

using namespace bbx;

static int device_inverse_gaussian_impl(int device, uint64_t seed,
                                        int64_t n_draw, const double* m,
                                        double lambda, double* out) {
  const std::string who = "bbx_device_inverse_gaussian: ";
  if (n_draw < 0) return fail(BBX_ERR_INVALID, who + "n_draw < 0");
  if (!m || !out) return fail(BBX_ERR_INVALID, who + "NULL argument");
  if (!(lambda > 0.) || !std::isfinite(lambda))
    return fail(BBX_ERR_INVALID, who + "lambda must be finite and positive");
  for (int64_t i = 0; i < n_draw; ++i)
    if (!(m[i] >= 0.) || !std::isfinite(m[i]))
      return fail(BBX_ERR_INVALID, who + "m[" + std::to_string(i) +
                                       "] is not finite and non-negative");
  return device_latent_draw(
      who, device, seed, n_draw, lambda,
      {{m, sizeof(double) * (size_t)n_draw}},
      [](const DevMem* d) { return InverseGaussianDraws{d[0].as<double>()}; },
      out);
}

extern "C" int bbx_device_inverse_gaussian(int device, uint64_t seed,
                                           int64_t n_draw, const double* m,
                                           double lambda, double* out) {
  return no_throw([&]() -> int {
    return device_inverse_gaussian_impl(device, seed, n_draw, m, lambda, out);
  });
}
