// The blocked two-pass scan of the Cox handles (cox_family.hpp): the segment
// descriptor, the max of eta and pass B.  Every scan runs over the fixed
// partition of seg_scan.hpp, whose header holds the contract, under the plain
// sum: each segment is cut into SCAN_G chunks; a pass A (cox_family.hpp's: it
// forms the values) writes one sum per chunk, pass B re-adds the sums of the
// chunks before its own in a fixed order and scans its chunk in tiles of
// SCAN_BLOCK x SCAN_E.  The kernels are static, as hamiltonian.hpp's are: each
// translation unit that includes this file gets its own copy.
#pragma once
#include <math.h>

#include "common.hpp"
#include "hamiltonian.hpp"
#include "seg_scan.hpp"

#pragma clang fp contract(off)  // a + b * c rounded as NumPy rounds it

namespace bbx {

// SCAN_G (hamiltonian.hpp): chunks per segment
constexpr int SCAN_BLOCK = 256;  // threads of the scan kernels
constexpr int SCAN_E = 8;        // elements per thread and tile
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_E;


// Up to two segments of one scan: elements base .. base+len-1, read forward
// (rev 0) or reversed (rev 1: a suffix sum is a prefix sum of the reversed
// segment; the chunks are cut from the far end).  rev 2 (pass B only) is a
// suffix sum over the FORWARD partition: chunk b of the scan is forward chunk
// SCAN_G - 1 - b read from its far end, so that a pass A which walked the
// segment forward for another scan has already left this one's chunk sums.
struct Segs {
  int64_t base[2];
  int64_t len[2];
  int rev[2];
};

__device__ inline int64_t seg_elem(const Segs& sg, int s, int64_t t) {
  return sg.rev[s] ? sg.base[s] + sg.len[s] - 1 - t : sg.base[s] + t;
}

__device__ inline double nanmax(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a > b ? a : b;
}

__device__ inline double wave_max(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = nanmax(x, __shfl_xor(x, off));
  return x;
}


// the max over the NPART partials, in every thread
__device__ inline double part_max(const double* part) {
  __shared__ double s_m;
  if (threadIdx.x < WAVE) {
    double a = part[threadIdx.x];
#pragma unroll
    for (int k = 1; k < NPART / WAVE; ++k)
      a = nanmax(a, part[threadIdx.x + k * WAVE]);
    a = wave_max(a);
    if (threadIdx.x == 0) s_m = a;
  }
  __syncthreads();
  const double r = s_m;
  __syncthreads();
  return r;
}

static __global__ __launch_bounds__(VEC_BLOCK) void cox_max_kernel(
    int64_t n, const double* __restrict__ eta, double* __restrict__ part,
    const int* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ double s_w[VEC_BLOCK / WAVE];
  double m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * VEC_BLOCK)
    m = nanmax(m, eta[i]);
  m = wave_max(m);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_w[threadIdx.x / WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = s_w[0];
#pragma unroll
    for (int k = 1; k < VEC_BLOCK / WAVE; ++k) r = nanmax(r, s_w[k]);
    part[blockIdx.x] = r;
  }
}

// Pass B: inclusive scan of the stored values of each chunk, offset by the
// sums of the chunks before it.
static __global__ __launch_bounds__(SCAN_BLOCK) void cox_scan_out_kernel(
    Segs sg, const double* __restrict__ val, double* __restrict__ out,
    const double* __restrict__ csum, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int s = blockIdx.x / SCAN_G, b = blockIdx.x % SCAN_G;
  // segment s, read once: with sg[s] read again at every element the compiler
  // carries its fields through the tile loop in 52 more vector registers
  const int64_t sbase = sg.base[s], slen = sg.len[s];
  const int rev = sg.rev[s];
  const bool mirror = rev == 2;
  const int fb = mirror ? SCAN_G - 1 - b : b;   // the chunk of the partition
  const ChunkRange ch = chunk_range<SCAN_G>(slen, fb);
  const int64_t t0 = ch.t0, t1 = ch.t1;
  if (t0 >= t1) return;
  // position t of the chunk's walk -> element (rev 0, 1: seg_elem's)
  auto elem = [&](int64_t t) {
    if (mirror) return sbase + (t0 + t1 - 1 - t);
    return rev ? sbase + slen - 1 - t : sbase + t;
  };
  __shared__ double s_off;
  __shared__ double s_wave[SCAN_BLOCK / WAVE];
  if (threadIdx.x < WAVE) {
    const int lane = threadIdx.x;
    double acc = 0.;
    for (int c = lane; c < b; c += WAVE)
      acc += csum[s * SCAN_G + (mirror ? SCAN_G - 1 - c : c)];
    acc = wave_allsum(acc);
    if (lane == 0) s_off = acc;
  }
  __syncthreads();
  double carry = s_off;
  for (int64_t tile = t0; tile < t1; tile += SCAN_TILE) {
    double x[SCAN_E];
    const int64_t tb = tile + (int64_t)threadIdx.x * SCAN_E;
    double run = 0.;
#pragma unroll
    for (int e = 0; e < SCAN_E; ++e) {
      const int64_t t = tb + e;
      run += t < t1 ? val[elem(t)] : 0.;
      x[e] = run;
    }
    double pre, tot;
    block_scan<Sum, SCAN_BLOCK>(run, s_wave, pre, tot);
    const double base = carry + pre;
#pragma unroll
    for (int e = 0; e < SCAN_E; ++e) {
      const int64_t t = tb + e;
      if (t < t1) out[elem(t)] = base + x[e];
    }
    carry += tot;
  }
}

}  // namespace bbx
