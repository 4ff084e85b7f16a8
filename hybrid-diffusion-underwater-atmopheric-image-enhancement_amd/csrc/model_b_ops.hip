// The three model ops of the reference's second tree that are not a conv, a norm or attention (diffusion/Model.py:110-168,
// 446-515; diffusion/Diffusion.py:229,252): nearest-neighbour resize, the 3 + 3 channel concat and global average pooling.
// HBM-bound streaming kernels; compiled with -ffp-contract=off like the other elementwise files (the pooling's sum and division
// round as written).  The sampler's update kernels are in sampler_step.hip.
#include "common.h"
#include "device.h"

using namespace hdiff;

#pragma clang fp contract(off)

namespace {

// F.interpolate(mode="nearest"): src = min(floor(dst * (float)in / out), in - 1), computed in float like ATen does
__global__ void resize_nearest_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int OH, int OW,
                                      float sy, float sx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % OW);
    const int64_t r = i / OW;
    const int oy = (int)(r % OH);
    const int64_t bc = r / OH;
    const int iy = min((int)floorf(oy * sy), H - 1), ix = min((int)floorf(ox * sx), W - 1);
    y[i] = x[(bc * H + iy) * W + ix];
  }
}

// torch.cat([a, b], dim=1) of per-sample blocks of n0 and n1 floats (the 3 + 3 channel sampler input, Diffusion.py:229,252:
// the head conv's two-pointer input needs 4-channel-aligned halves, so this one seam is materialised -- 24 B per pixel)
__global__ void concat2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t n0,
                               int64_t n1, int64_t total) {
  const int64_t per = n0 + n1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = i / per, r = i - s * per;
    out[i] = r < n0 ? a[s * n0 + r] : b[s * n1 + (r - n0)];
  }
}

// nn.AdaptiveAvgPool2d((1, 1)): one wave per (sample, channel) plane
__global__ void avgpool_global_kernel(const float* __restrict__ x, float* __restrict__ y, int BC, int HW) {
  const int plane = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (plane >= BC) return;
  const float* p = x + (size_t)plane * HW;
  float s = 0.f;
  for (int i = threadIdx.x & 63; i < HW; i += 64) s += p[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) y[plane] = s / (float)HW;
}

}  // namespace

extern "C" {

int hdiff_resize_nearest(const float* x, float* y, int BC, int H, int W, int OH, int OW, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && y && BC > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "resize_nearest: bad arguments");
  (void)hipGetLastError();
  const int64_t n = (int64_t)BC * OH * OW;
  hipLaunchKernelGGL(resize_nearest_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, OH, OW,
                     (float)H / (float)OH, (float)W / (float)OW, n);
  HDIFF_CHECK_LAUNCH("resize_nearest_kernel");
  return HDIFF_OK;
}

int hdiff_concat2(const float* a, const float* b, float* out, int B, int64_t n0, int64_t n1, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(a && b && out && B > 0 && n0 > 0 && n1 > 0, "concat2: bad arguments");
  (void)hipGetLastError();
  const int64_t total = (int64_t)B * (n0 + n1);
  hipLaunchKernelGGL(concat2_kernel, dim3(grid_ceil_8k(total, 4)), dim3(256), 0, (hipStream_t)stream, a, b, out, n0, n1, total);
  HDIFF_CHECK_LAUNCH("concat2_kernel");
  return HDIFF_OK;
}

int hdiff_avgpool_global(const float* x, float* y, int BC, int HW, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && y && BC > 0 && HW > 0, "avgpool_global: bad arguments");
  (void)hipGetLastError();
  hipLaunchKernelGGL(avgpool_global_kernel, dim3(cdiv(BC, 4)), dim3(256), 0, (hipStream_t)stream, x, y, BC, HW);
  HDIFF_CHECK_LAUNCH("avgpool_global_kernel");
  return HDIFF_OK;
}

}  // extern "C"
