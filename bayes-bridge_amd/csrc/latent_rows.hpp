// What the latent families of the Gaussian samplers share (probit.hip,
// student_t.hip, censored.hip, quantile.hip): the one row kernel of the update that follows
// the coefficient draw, its launch, and the stand-alone draw kernel with its
// C-ABI front.  Given psi = X~ beta, a family draws one value per row -- the
// probit and censored models' latent z_i, the Student-t model's mixing weight
// omega_i -- and collects two sums over the rows on the way: the
// log-likelihood, and the sum of the vector w whose product X~^T w is the next
// draw's zbase (w = z; Student-t, quantile: w = kappa), which centres that
// product.
//
// A family states a policy V, passed to the kernels by value (the row arrays
// it reads and writes, and the few numbers its expressions need):
//
//   reads_tau               static constexpr bool: the family has a precision
//                           tau, read once per kernel from ChainScalars::
//                           obs_prec (false: nothing is read)
//   struct Once, once(tau)  what a thread computes once from tau -- probit:
//                           nothing; Student-t: tau, (nu+1)/2, 1/2 log tau;
//                           censored: tau, sqrt(tau), 1/2 log tau
//   row(k, seed, stream, i, ll, w)
//                           row i: its draw and stores, its log-likelihood
//                           term and its w_i
//   draw(k, seed, stream, i)
//                           the row's draw alone (families with a stand-alone
//                           sampler)
//
// A policy method is the expression of its file's header, with that
// association and its non-finite guards; the kernels only loop, add, reduce
// and store.  Policies live in the unnamed namespace of their file and the
// kernels are static; a kernel trace names a launch by its policy
// (latent_row_kernel<...ProbitRows<double>>, ...StudentTRows, ...CensoredRows).
//
// The contract of the row kernel:
//  - One lane per row on row_grid(n) blocks of 256, grid-stride: from ROW_GRID
//    x 256 rows on a lane takes a second row.
//  - The draw of row i reads Philox(seed, stream, i[, trial]) and is a function
//    of the key, the row's data, psi_i and tau alone, whatever the grid: a
//    refresh with an iteration's stream reproduces that iteration's state bit
//    for bit.  `stream` carries the iteration (chain.hip's iter_stream; -1:
//    the reserved index of a chain that has not run).
//  - A lane adds its rows in index order; block totals in a fixed order
//    (block_totals_256: waves 0..3 added by thread 0), one partial per block:
//    the log-likelihood's into row_part[0 .. *row_blocks), for chain.hip's
//    finish kernel, the other's into row_part[ROW_GRID ..), folded by
//    launch_sumw_fold onto the NPART slots of the design's PS_SUMW, which
//    launch_tdot(w) re-adds.  No float atomics: the same inputs give the same
//    bits on every run.
//  - Everything runs on the design's stream.
//
// What a call leaves: probit, latent_i ~ N(psi_i, 1) on the half-line
// outcome_i selects; Student-t, under tau = scalars->obs_prec, latent_i =
// omega_i, obs_prec_i = tau latent_i and kappa_i = obs_prec_i y_i (the
// log-likelihood's row constant is added by the finish kernel); censored,
// under tau, latent_i = outcome_i on an observed row, else its truncated
// normal.  The expressions are in the headers of the three files.
//
// The stand-alone draw kernel is the same policy without the sums, on
// STREAM_LATENT with tau by value; device_latent_draw is the host front of its
// C-ABI entry points after their own argument checks.
#pragma once
#include <initializer_list>
#include <string>

#include "chain.hpp"
#include "philox.hpp"
#include "samplers.hpp"

namespace bbx {

template <class V>
static __global__ __launch_bounds__(256) void latent_row_kernel(
    int64_t n, uint64_t seed, uint64_t stream,
    const ChainScalars* __restrict__ sc, V v, double* __restrict__ ll_part,
    double* __restrict__ w_part) {
  const typename V::Once k = v.once(V::reads_tau ? sc->obs_prec : 0.);
  double ll = 0., ws = 0.;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    double term, w;
    v.row(k, seed, stream, i, term, w);
    ws += w;
    ll += term;
  }
  block_totals_256(ll, ws);
  if (threadIdx.x == 0) {
    ll_part[blockIdx.x] = ll;
    w_part[blockIdx.x] = ws;
  }
}

template <class V>
static __global__ __launch_bounds__(256) void latent_draw_kernel(
    int64_t n, uint64_t seed, double tau, V v, double* __restrict__ out) {
  const typename V::Once k = v.once(tau);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256)
    out[i] = v.draw(k, seed, STREAM_LATENT, i);
}

namespace {  // host side: internal, as the policies appear in the names

// The body of a family's launch_latent_rows
template <class V>
int launch_rows(bbx_chain* c, uint64_t stream, const V& v, int* row_blocks) {
  bbx_design* h = c->h;
  const int rg = row_grid(h->n);
  double* rp = c->row_part.as<double>();
  BBX_LAUNCH(latent_row_kernel<V>, dim3(rg), dim3(256), 0, h->stream, h->n,
             c->seed, stream, c->scalars.as<ChainScalars>(), v, rp,
             rp + ROW_GRID);
  BBX_HIP(hipGetLastError());
  BBX_TRY(launch_sumw_fold(h, rp + ROW_GRID, rg));
  if (row_blocks) *row_blocks = rg;
  return BBX_OK;
}

// n_draw draws on `device` into `out`: the caller's arrays `in` (at most
// DRAW_INPUTS) up, the policy make(d) of their device copies d[0], d[1], ...
// on stream 0 with the chain's grid, the draws back.
struct DrawInput {
  const void* host;
  size_t bytes;
};
constexpr int DRAW_INPUTS = 3;

template <class Make>
int device_latent_draw(const std::string& who, int device, uint64_t seed,
                       int64_t n_draw, double tau,
                       std::initializer_list<DrawInput> in, Make&& make,
                       double* out) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(BBX_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= count)
    return fail(BBX_ERR_INVALID, who + "device index out of range");
  if (n_draw == 0) return BBX_OK;
  BBX_HIP(hipSetDevice(device));
  const size_t nb = sizeof(double) * (size_t)n_draw;
  DevMem d[DRAW_INPUTS], dout;
  int j = 0;
  for (const DrawInput& a : in) BBX_TRY(d[j++].alloc(a.bytes));
  BBX_TRY(dout.alloc(nb));
  j = 0;
  for (const DrawInput& a : in)
    BBX_HIP(hipMemcpy(d[j++].ptr, a.host, a.bytes, hipMemcpyHostToDevice));
  auto v = make(d);
  BBX_LAUNCH(latent_draw_kernel<decltype(v)>, dim3(row_grid(n_draw)),
             dim3(256), 0, 0, n_draw, seed, tau, v, dout.as<double>());
  BBX_HIP(hipGetLastError());
  BBX_HIP(hipMemcpy(out, dout.ptr, nb, hipMemcpyDeviceToHost));
  return BBX_OK;
}

}  // namespace
}  // namespace bbx
