// Sequential host replay of the device chain's random draws (replay.cpp).
//
// Every device draw is a pure function of (seed, stream, element, inputs):
// Philox is counter-based and the kernels address each piece of randomness by
// (element, sub-stream).  The loops below walk the same sub-streams one element
// after the other, with none of the kernels' structure -- no lanes, no LDS
// lists, no speculation, no masks -- so that a bookkeeping slip in
// pg_queue.hpp or tilted_stable_block (chain.hip) shows as a different draw.
//
// This header is compiled twice into libbbx_hostrng.so:
//   replay.cpp               namespace bbx as every host file sees it: pos_pow
//                            is libm's pow, the reference's arithmetic; the
//                            replay uses right_mass / series_accept (variant 0)
//   replay_device_forms.cpp  samplers.hpp once more in a namespace of its own
//                            with pos_pow's device branch (roots, integer
//                            powers, exp(y log x)) and the replay on
//                            right_mass_direct / series_accept_direct: the
//                            kernels' arithmetic in host libm (variant 1)
// The two differ by rounding only; comparing them on the CPU says how often
// arithmetic alone moves a draw (tests/test_replay_cpu.py).
#pragma once

#if defined(BBX_REPLAY_DEVICE_FORMS)
#define bbx bbx_device_forms
#define __HIP_DEVICE_COMPILE__ 1   // selects pos_pow's device branch, nothing else
#define BBX_REPLAY_NS replay_device_forms
#else
#define BBX_REPLAY_NS replay_reference_forms
#endif

#include <math.h>
#include <stdint.h>

#include "samplers.hpp"

namespace BBX_REPLAY_NS {

using bbx::kPi;
using bbx::PolyaGamma;
using bbx::TiltedStable;

// Philox4x32-10 with the counter layout of philox.hpp (which needs the HIP
// headers and has a device-only normal()).
struct HostPhilox {
  uint32_t key[2];
  uint32_t ctr[4];
  uint32_t out[4];
  int have;

  HostPhilox(uint64_t seed, uint64_t stream, uint64_t index, uint32_t trial = 0) {
    key[0] = (uint32_t)seed;
    key[1] = (uint32_t)(seed >> 32);
    ctr[0] = trial << 20;
    ctr[1] = (uint32_t)stream;
    ctr[2] = (uint32_t)index;
    ctr[3] = (uint32_t)(index >> 32) ^ ((uint32_t)(stream >> 32) << 16);
    have = 0;
  }

  static inline void block(const uint32_t c[4], const uint32_t k[2],
                           uint32_t o[4]) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    uint32_t k0 = k[0], k1 = k[1];
    for (int round = 0; round < 10; ++round) {
      const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
      const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
      const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
      const uint32_t n1 = (uint32_t)p1;
      const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
      const uint32_t n3 = (uint32_t)p0;
      c0 = n0; c1 = n1; c2 = n2; c3 = n3;
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
  }

  inline uint32_t next_u32() {
    if (have == 0) {
      block(ctr, key, out);
      have = 4;
      ctr[0] += 1;
    }
    return out[--have];
  }

  inline double uniform() {
    const uint64_t hi = next_u32();
    const uint64_t lo = next_u32();
    const uint64_t bits = ((hi << 32) | lo) >> 11;
    return ((double)bits + 0.5) * (1.0 / 9007199254740992.0);
  }

  // cos(pi x), 0 < x < 2, to a few ulp RELATIVE everywhere: the argument is
  // folded into [0, 1/4] exactly (every subtraction below is exact in binary
  // floating point) before pi enters, so the zeros at 1/2 and 3/2 cost nothing.
  static inline double cospi_exact(double x) {
    if (x > 1.) x = 2. - x;                  // cos(pi (2 - x)) = cos(pi x)
    double sign = 1.;
    if (x > .5) {                            // cos(pi x) = -cos(pi (1 - x))
      x = 1. - x;
      sign = -1.;
    }
    return sign * (x <= .25 ? cos(kPi * x) : sin(kPi * (.5 - x)));
  }

  // the device's Box-Muller: sqrt(-2 log u1) cospi(2 u2)
  inline double normal() {
    const double u1 = uniform();
    const double u2 = uniform();
    return sqrt(-2.0 * log(u1)) * cospi_exact(2.0 * u2);
  }
};

#if defined(BBX_REPLAY_DEVICE_FORMS)
inline double pg_right_mass(double z, double rate) {
  return PolyaGamma::right_mass_direct(z, rate);
}
template <class G>
inline bool pg_series(G& g, double x) {
  return PolyaGamma::series_accept_direct(g, x);
}
#else
inline double pg_right_mass(double z, double rate) {
  return PolyaGamma::right_mass(z, rate);
}
template <class G>
inline bool pg_series(G& g, double x) {
  return PolyaGamma::series_accept(g, x);
}
#endif

inline void normal(uint64_t seed, uint64_t stream, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    HostPhilox g(seed, stream, (uint64_t)i);
    out[i] = g.normal();
  }
}

inline void uniforms(uint64_t seed, uint64_t stream, uint64_t index,
                     uint32_t trial, int64_t n, double* out) {
  HostPhilox g(seed, stream, index, trial);
  for (int64_t k = 0; k < n; ++k) out[k] = g.uniform();
}

// polya_gamma_block (pg_queue.hpp), one element after the other.
// attempts[i]: inverse-Gaussian proposals of element i (0: none was needed);
// restarts[i]: 1 when the series test rejected and the draw started over.
template <class Shape>
inline void polya_gamma(uint64_t seed, uint64_t stream, int64_t n,
                        const Shape* shape, const double* tilt, double* out,
                        int32_t* attempts, int32_t* restarts) {
  for (int64_t i = 0; i < n; ++i) {
    const double eta = tilt[i];
    const double nt = (double)shape[i];
    if (attempts) attempts[i] = 0;
    if (restarts) restarts[i] = 0;
    if (!(fabs(eta) <= 1.7e308)) {
      out[i] = eta - eta;
      continue;
    }
    if (nt != 1.) {
      HostPhilox g(seed, stream, (uint64_t)i);
      out[i] = PolyaGamma::draw(g, (int)nt, eta);
      continue;
    }
    const double z = 0.5 * fabs(eta);
    const double rate = 0.5 * z * z + 0.125 * kPi * kPi;
    double x;
    HostPhilox g0(seed, stream, (uint64_t)i, 0);
    if (g0.uniform() < pg_right_mass(z, rate)) {
      x = PolyaGamma::trunc_exp(g0, 1. / rate, PolyaGamma::kCut);
    } else {
      for (uint32_t att = 0;; ++att) {
        HostPhilox g(seed, stream, (uint64_t)i, 1u + (att < 125u ? att : 125u));
        if (att > 125u) g.ctr[0] += ((att - 125u) & 0x3FFFu) << 6;
        if (PolyaGamma::trunc_inv_gauss_attempt(g, z, PolyaGamma::kCut, x)) {
          if (attempts) attempts[i] = (int32_t)att + 1;
          break;
        }
      }
    }
    HostPhilox gs(seed, stream, (uint64_t)i, 127);
    if (pg_series(gs, x)) {
      out[i] = 0.25 * x;
    } else {
      HostPhilox gr(seed, stream, (uint64_t)i, 128);
      out[i] = 0.25 * PolyaGamma::jacobi(gr, z);
      if (restarts) restarts[i] = 1;
    }
  }
}

// tilted_stable_block (chain.hip): candidates 0, 1, 2, ... of element j in
// order, candidate t on sub-stream min(t, 4095); the first accepted one is the
// draw.  winner[j]: its number.
inline void tilted_stable(uint64_t seed, uint64_t stream, int64_t n, double a,
                          const double* tilt, double* out, int32_t* winner) {
  const double odds = (1. - a) / a;
  for (int64_t j = 0; j < n; ++j) {
    const double tilt_pow = bbx::pos_pow(tilt[j], a);
    const bool cheap = tilt_pow < TiltedStable::kCostThreshold;
    for (uint32_t t = 0;; ++t) {
      const uint32_t trial = t < 4095u ? t : 4095u;
      HostPhilox g(seed, stream, (uint64_t)j, trial);
      bool ok;
      double val;
      if (cheap) {
        ok = TiltedStable::dc_trial(g, a, tilt[j], 1., val);
      } else {
        double x = NAN;
        ok = TiltedStable::dr_trial_flat(g, a, tilt_pow, x);
        val = bbx::pos_pow(x, -odds);
      }
      if (trial >= 4095u) ok = true;   // the kernel's budget: unreachable honestly
      if (ok) {
        out[j] = val;
        if (winner) winner[j] = (int32_t)t;
        break;
      }
    }
  }
}

// latent_row_kernel / latent_draw_kernel<ProbitRows> (probit.hip): trials 0, 1,
// 2, ... of element i in order, trial t on sub-stream t; the first accepted
// proposal is the draw.  trials[i]: trials made (0: psi was not finite).
inline void truncated_normal(uint64_t seed, uint64_t stream, int64_t n,
                             const double* psi, const unsigned char* positive,
                             double* out, int32_t* trials) {
  using bbx::TruncatedNormal;
  for (int64_t i = 0; i < n; ++i) {
    const double p = psi[i];
    const bool pos = positive[i] != 0;
    if (trials) trials[i] = 0;
    if (!(fabs(p) <= 1.7e308)) {
      out[i] = p - p;
      continue;
    }
    int t = 0;
    double z = TruncatedNormal::at_cap(p, pos);
    for (; t < TruncatedNormal::kMaxTrials; ++t) {
      HostPhilox g(seed, stream, (uint64_t)i, (uint32_t)t);
      double prop;
      if (TruncatedNormal::trial(g, p, pos, prop)) {
        z = prop;
        ++t;
        break;
      }
    }
    out[i] = z;
    if (trials) trials[i] = t;
  }
}

// latent_row_kernel<QuantileRows> / latent_draw_kernel<InverseGaussianDraws>
// (quantile.hip): element i draws one normal and one uniform of Philox(seed,
// stream, i).  branch[i]: 0 the smaller root, 1 the other; margin[i]: the
// number compared with 1.
inline void inverse_gaussian(uint64_t seed, uint64_t stream, int64_t n,
                             const double* m, double lambda, double* out,
                             int32_t* branch, double* margin) {
  for (int64_t i = 0; i < n; ++i) {
    HostPhilox g(seed, stream, (uint64_t)i);
    int b = 0;
    double t = 0.;
    out[i] = bbx::InverseGaussian::draw(g, m[i], lambda, &b, &t);
    if (branch) branch[i] = b;
    if (margin) margin[i] = t;
  }
}

inline double gamma(uint64_t seed, uint64_t stream, uint64_t index,
                    double shape) {
  HostPhilox g(seed, stream, index);
  return bbx::gamma_draw(g, shape);
}

}  // namespace BBX_REPLAY_NS

#undef bbx
#if defined(BBX_REPLAY_DEVICE_FORMS)
#undef __HIP_DEVICE_COMPILE__
#endif
