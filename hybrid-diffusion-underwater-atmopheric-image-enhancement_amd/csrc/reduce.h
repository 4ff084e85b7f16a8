// The fixed-order double sums of the score and loss kernels (msssim.hip, train_b_ops.hip, quality.hip, uciqe.hip, color_diff.hip,
// perceptual.hip, dino.hip, distribution.hip).  Beside device.h, this header, radix_select.h and lab.h are the only ones that hold device
// code; no kernel of profiles/roofline_traffic.json reaches any of them.
//
// THE ORDER OF THE ADDITIONS IS THE CONTRACT: results are pinned bit for bit, and every function here adds in exactly one order.
//   1. inside a wave, wave_sum's xor ladder (device.h: offsets 32, 16, 8, 4, 2, 1);
//   2. then ONE thread adds the THREADS / 64 wave sums in index order, starting from 0.0;
//   3. for partials, thread t first adds p[t], p[t + THREADS], p[t + 2 THREADS], ... in that order, starting from 0.0; then 1 and 2.
// No float atomics.  THREADS is the workgroup size the kernel is launched with (a multiple of 64); every thread must call.
// The sums of dino.hip's token_sum4 and tap kernels, of groupnorm*.hip and of optimizer.hip associate differently and stay their own.
#pragma once
#include "device.h"

namespace hdiff {

__device__ __forceinline__ bool non_finite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }

// Block-wide sum, returned to every thread; ends with a barrier, so calls may follow one another.
template <int THREADS>
__device__ double block_sum_all(double v) {
  __shared__ double part[THREADS / 64];
  __shared__ double total;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < THREADS / 64; ++i) s += part[i];
    total = s;
  }
  __syncthreads();
  const double r = total;
  __syncthreads();
  return r;
}

// Block-wide sum, valid in thread 0 only (0.0 elsewhere).  One barrier and none at the end: once per kernel, or a barrier between calls.
template <int THREADS>
__device__ double block_sum_to0(double v) {
  __shared__ double part[THREADS / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < THREADS / 64; ++i) s += part[i];
  return s;
}

// this thread's share of the n partials p[0], p[stride], ..., p[(n - 1) stride]
template <int THREADS>
__device__ __forceinline__ double strided_share(const double* __restrict__ p, int n, int stride) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += THREADS) acc += p[(int64_t)i * stride];
  return acc;
}

// The sum of n partials in index order by one workgroup: to every thread, or to thread 0 only.
template <int THREADS>
__device__ double sum_partials(const double* __restrict__ p, int n, int stride) {
  return block_sum_all<THREADS>(strided_share<THREADS>(p, n, stride));
}
template <int THREADS>
__device__ double sum_partials_to0(const double* __restrict__ p, int n, int stride) {
  return block_sum_to0<THREADS>(strided_share<THREADS>(p, n, stride));
}

}  // namespace hdiff
