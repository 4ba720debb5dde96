// The Student-t regression model's updates after the coefficient draw.  The
// t-density is a scale mixture of normals: with omega_i ~ Gamma(nu/2, rate
// nu/2) and y_i | beta, tau, omega ~ N(psi_i, 1 / (tau omega_i)),
//
//   pass A   S = sum_i omega_i r_i^2 with the OLD omega, r = y - psi
//   tau      gamma_draw(n/2) / (S/2) on STREAM_OBSVAR (one block)
//   pass B   omega_i = gamma_draw((nu+1)/2) / ((nu + tau r_i^2)/2) on
//            STREAM_MIX with the NEW tau; Omega_i = tau omega_i, kappa_i =
//            Omega_i y_i, the block sums of kappa and of the log-likelihood
//   finish   the log-likelihood partials summed in fixed order, plus n times
//            the row constant lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu/2)
//            (chain.hip's finish kernel)
//
// tau is drawn before omega so that what an iteration leaves -- (beta, tau,
// omega) with omega drawn under that beta and that tau -- is a function of
// (beta, tau, seed, iteration): a refresh reproduces it without a redraw of
// tau.
//
// Pass B is latent_rows.hpp's row kernel with this file's per-row expression.
// It is one lane per row.  gamma_draw accepts ~95 % of its proposals and
// branches on (seed, stream, row, nu) alone, never on the data: a wave of 64
// rows waits for its slowest lane (P(all 64 accept at once) ~ 4 %, two rounds
// nearly always), and the data-dependent rate divides the draw afterwards.
#include <cmath>

#include "latent_rows.hpp"

namespace bbx {

namespace {

// pass A: part[b] = block b's sum of omega_i (y_i - psi_i)^2
__global__ __launch_bounds__(256) void student_t_wrss_kernel(
    int64_t n, const double* __restrict__ y, const double* __restrict__ psi,
    const double* __restrict__ omega, double* __restrict__ part) {
  double acc = 0.;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    const double r = y[i] - psi[i];
    acc += omega[i] * (r * r);
  }
  const double tot = block_total_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// tau | beta, omega ~ Gamma(n/2, rate S/2): the linear model's rule with the
// weighted residual sum for the rss (single block)
__global__ __launch_bounds__(256) void student_t_tau_kernel(
    int64_t n, uint64_t seed, uint64_t stream, const double* __restrict__ part,
    int count, ChainScalars* __restrict__ sc) {
  const double S = sum_row_parts(part, count);
  if (threadIdx.x != 0) return;
  Philox g(seed, stream, 0);
  sc->obs_prec = gamma_draw(g, (double)n / 2.) / (S / 2.);
}

// pass B.  The sums are those of the log-likelihood terms 1/2 log tau -
// (nu+1)/2 log1p(tau r^2 / nu) and of kappa_i.  A residual that is not finite
// gives a NaN weight and a NaN term (the draw itself never looks at the data,
// so no row can loop on one).
struct StudentTRows {
  double nu;
  const double* __restrict__ y;
  const double* __restrict__ psi;
  double* __restrict__ latent;
  double* __restrict__ obs_prec;
  double* __restrict__ kappa;
  static constexpr bool reads_tau = true;
  struct Once {
    double tau, shape, hlt;
  };
  __device__ Once once(double tau) const {
    return {tau, (nu + 1.) / 2., 0.5 * log(tau)};
  }
  __device__ void row(const Once& c, uint64_t seed, uint64_t stream, int64_t i,
                      double& ll, double& ks) const {
    const double yi = y[i];
    const double r = yi - psi[i];
    const double q = c.tau * (r * r);
    Philox g(seed, stream, (uint64_t)i);
    double om = gamma_draw(g, c.shape) / ((nu + q) / 2.);
    double term = c.hlt - c.shape * log1p(q / nu);
    if (!(fabs(r) <= 1.7e308)) {
      om = r - r;
      term = om;
    }
    const double w = c.tau * om;
    const double k = w * yi;
    latent[i] = om;
    obs_prec[i] = w;
    kappa[i] = k;
    ks = k;
    ll = term;
  }
};

}  // namespace

double student_t_row_const(double nu) {
  return std::lgamma((nu + 1.) / 2.) - std::lgamma(nu / 2.) -
         0.5 * std::log(nu / 2.);
}

int launch_student_t_tau(bbx_chain* c, uint64_t stream) {
  bbx_design* h = c->h;
  const int rg = row_grid(h->n);
  double* rp = c->row_part.as<double>();
  BBX_LAUNCH(student_t_wrss_kernel, dim3(rg), dim3(256), 0, h->stream, h->n,
             c->outcome.as<double>(), c->psi.as<double>(),
             c->latent.as<double>(), rp);
  BBX_LAUNCH(student_t_tau_kernel, dim3(1), dim3(256), 0, h->stream, h->n,
             c->seed, stream, rp, rg, c->scalars.as<ChainScalars>());
  BBX_HIP(hipGetLastError());
  return BBX_OK;
}

template <>
int launch_latent_rows<BBX_MODEL_STUDENT_T>(bbx_chain* c, uint64_t stream,
                                            int* row_blocks) {
  return launch_rows(
      c, stream,
      StudentTRows{c->df, c->outcome.as<double>(), c->psi.as<double>(),
                   c->latent.as<double>(), c->obs_prec.as<double>(),
                   c->kappa.as<double>()},
      row_blocks);
}

}  // namespace bbx
