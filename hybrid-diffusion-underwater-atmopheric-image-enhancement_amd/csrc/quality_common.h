// What the per-image quality scores share (quality.hip: PSNR / SSIM / UIQM; uciqe.hip: UCIQE): the workgroup size, the non-finite
// test, the fixed-order double sums and the argument checks.  Included inside each file's unnamed namespace.
#pragma once

constexpr int kThreads = 256;

__device__ __forceinline__ bool non_finite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }

// Block-wide sum in a fixed order (wave sums, then in index order), returned to every thread; ends with a barrier.
__device__ double block_sum_all(double v) {
  __shared__ double part[kThreads / 64];
  __shared__ double total;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) s += part[i];
    total = s;
  }
  __syncthreads();
  const double r = total;
  __syncthreads();
  return r;
}

__device__ double sum_partials(const double* __restrict__ p, int n, int stride) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) acc += p[(int64_t)i * stride];
  return block_sum_all(acc);
}

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

int check_sizes(const char* who, int N, int H, int W, int min_side) {
  HDIFF_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d; between 1 and 65535 images", who, N);
  HDIFF_CHECK_ARG(H >= min_side && W >= min_side, "%s: H = %d, W = %d; both sides must be at least %d", who, H, W, min_side);
  HDIFF_CHECK_ARG((int64_t)H * W <= (1ll << 30), "%s: H * W = %lld is too large; at most 2^30 pixels", who, (long long)H * W);
  return HDIFF_OK;
}
