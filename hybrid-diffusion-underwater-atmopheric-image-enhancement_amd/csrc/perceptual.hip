// The pieces of a VGG feature trunk that the conv kernels do not cover, and the loss / score arithmetic that sits on its taps
// (hdiff_amd/perceptual.py is the caller; tests/_perceptual_def.py holds the definitions the kernels are held to):
//   ReLU and 2x2 / stride-2 max-pooling, forward and backward      bit for bit against their fp32 definitions
//   mean |a - b| and its backward                                  terms rounded to fp32, summed in double in a fixed order
//   the Charbonnier map sqrt(d^2 + 1) - 1 and its backward         one rounding per written operation
//   one layer of the LPIPS distance                                channel norms and sums in double, added to out[n]
//   the LPIPS input scaling ((x * mul + add) - shift[c]) / scale[c]
// The 3x3 convs of the trunk are autograd.fused_conv's: nothing here multiplies matrices.  Every entry validates on the host before
// a launch, allocates nothing, never synchronises, uses no float atomics and gives bitwise repeatable results; the reductions
// take their grid from the per-image (or per-call) element count alone, so a result does not depend on the batch it was computed in.
// Compiled with -ffp-contract=off: each written operation rounds once.
#include <math.h>

#include "common.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxParts = 256;            // partial sums per reduction (per image for the LPIPS layer)
constexpr int64_t kMaxElems = 1ll << 40;

// ------------------------------------------------------------------------------------------------------------------ ReLU
__global__ __launch_bounds__(kThreads) void relu_fwd_kernel(const float* x, float* y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float v = x[i];
    y[i] = v > 0.0f ? v : (v != v ? v : 0.0f);      // a NaN stays a NaN (as torch.relu): a spoiled input must not come out finite
  }
}

__global__ __launch_bounds__(kThreads) void relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                             float* __restrict__ dx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    dx[i] = y[i] > 0.0f ? dy[i] : 0.0f;
}

// --------------------------------------------------------------------------------------------------------------- pooling
// the first maximal element of the window in row-major order: a later element wins only when strictly greater.  A NaN counts as
// maximal (the first one wins), so the maximum of a window that holds one is NaN, as in torch
__device__ __forceinline__ int window_choice(float w0, float w1, float w2, float w3, float* top) {
  int k = 0;
  float m = w0;
  if (m == m && (w1 > m || w1 != w1)) { m = w1; k = 1; }
  if (m == m && (w2 > m || w2 != w2)) { m = w2; k = 2; }
  if (m == m && (w3 > m || w3 != w3)) { m = w3; k = 3; }
  *top = m;
  return k;
}

__global__ __launch_bounds__(kThreads) void maxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t planes,
                                                                 int H, int W) {
  const int OH = H >> 1, OW = W >> 1;
  const int64_t n = planes * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int ox = (int)(i % OW);
    const int64_t t = i / OW;
    const int oy = (int)(t % OH);
    const int64_t p = t / OH;
    const float* r0 = x + (p * H + 2 * oy) * W + 2 * ox;
    float m;
    window_choice(r0[0], r0[1], r0[W], r0[W + 1], &m);
    y[i] = m;
  }
}

// a gather: every INPUT element asks whether it is its window's choice; elements of a dropped last row / column get 0
__global__ __launch_bounds__(kThreads) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 float* __restrict__ dx, int64_t planes, int H, int W) {
  const int OH = H >> 1, OW = W >> 1;
  const int64_t n = planes * H * W;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % W);
    const int64_t t = i / W;
    const int r = (int)(t % H);
    const int64_t p = t / H;
    const int oy = r >> 1, ox = c >> 1;
    float g = 0.0f;
    if (oy < OH && ox < OW) {
      const float* r0 = x + (p * H + 2 * oy) * W + 2 * ox;
      float m;
      const int k = window_choice(r0[0], r0[1], r0[W], r0[W + 1], &m);
      if (k == ((r & 1) << 1 | (c & 1))) g = dy[(p * OH + oy) * OW + ox];
    }
    dx[i] = g;
  }
}

// --------------------------------------------------------------------------------------------------------------- L1 mean
__global__ __launch_bounds__(kThreads) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                               double* __restrict__ part) {
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float d = b ? a[i] - b[i] : a[i];
    acc += (double)fabsf(d);
  }
  const double s = block_sum_all<kThreads>(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void l1_finalize_kernel(const double* __restrict__ part, int parts, int64_t n,
                                                                float* __restrict__ out) {
  const double s = sum_partials<kThreads>(part, parts, 1);
  if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}

__global__ __launch_bounds__(kThreads) void l1_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ g, int64_t n, float* __restrict__ da) {
  const float c = g[0] / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float u = a[i], v = b ? b[i] : 0.0f;
    da[i] = u > v ? c : (u < v ? -c : 0.0f);
  }
}

// ----------------------------------------------------------------------------------------------------------- Charbonnier
__global__ __launch_bounds__(kThreads) void charbonnier_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float d = a[i] - b[i];
    y[i] = sqrtf(d * d + 1.0f) - 1.0f;
  }
}

__global__ __launch_bounds__(kThreads) void charbonnier_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    const float* __restrict__ dy, int dy_stride, float divisor,
                                                                    float* __restrict__ da, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float d = a[i] - b[i];
    const float g = dy[i * dy_stride] / divisor;          // divisor 1 (an elementwise dy, or a sum) divides exactly
    da[i] = g * d / sqrtf(d * d + 1.0f);
  }
}

// ----------------------------------------------------------------------------------------------------------------- LPIPS
// grid (parts, 1, N): one pixel per thread and trip; the channels of a pixel are HW apart, neighbouring threads read neighbouring words
__global__ __launch_bounds__(kThreads) void lpips_partial_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                  const float* __restrict__ w, int Cc, int64_t HW,
                                                                  double* __restrict__ part) {
  const int n = blockIdx.z;
  const float* p0 = f0 + (int64_t)n * Cc * HW;
  const float* p1 = f1 + (int64_t)n * Cc * HW;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    double s0 = 0.0, s1 = 0.0;
    for (int c = 0; c < Cc; ++c) {
      const double u = (double)p0[c * HW + i], v = (double)p1[c * HW + i];
      s0 += u * u;
      s1 += v * v;
    }
    const double n0 = sqrt(s0) + 1e-10, n1 = sqrt(s1) + 1e-10;
    double pix = 0.0;
    for (int c = 0; c < Cc; ++c) {
      const double d = (double)p0[c * HW + i] / n0 - (double)p1[c * HW + i] / n1;
      pix += (double)w[c] * (d * d);
    }
    acc += pix;
  }
  const double s = block_sum_all<kThreads>(acc);
  if (threadIdx.x == 0) part[(int64_t)n * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void lpips_finalize_kernel(const double* __restrict__ part, int parts, int64_t HW,
                                                                   double* __restrict__ out) {
  const int n = blockIdx.x;
  const double s = sum_partials<kThreads>(part + (int64_t)n * parts, parts, 1);
  if (threadIdx.x == 0) out[n] = out[n] + s / (double)HW;
}

__global__ __launch_bounds__(kThreads) void scale_input_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                                const float* __restrict__ scale, float mul, float add,
                                                                float* __restrict__ y, int Cc, int64_t HW, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)((i / HW) % Cc);
    y[i] = ((x[i] * mul + add) - shift[c]) / scale[c];
  }
}

int check_count(const char* who, int64_t n) {
  HDIFF_CHECK_ARG(n >= 1 && n <= kMaxElems, "%s: n = %lld; between 1 and 2^40 elements", who, (long long)n);
  return HDIFF_OK;
}

int check_planes(const char* who, int64_t planes, int H, int W) {
  HDIFF_CHECK_ARG(planes >= 1, "%s: planes = %lld; at least 1 plane", who, (long long)planes);
  HDIFF_CHECK_ARG(H >= 2 && W >= 2, "%s: H = %d, W = %d; both sides must be at least 2", who, H, W);
  HDIFF_CHECK_ARG((int64_t)H * W <= (1ll << 30) && planes <= kMaxElems / ((int64_t)H * W),
                  "%s: planes * H * W is too large; at most 2^40 elements", who);
  return HDIFF_OK;
}

int check_features(const char* who, int N, int Cc, int H, int W) {
  const int rc = check_sizes(who, N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(Cc >= 1 && Cc <= 65536, "%s: C = %d; between 1 and 65536 channels", who, Cc);
  HDIFF_CHECK_ARG((int64_t)N * Cc <= kMaxElems / ((int64_t)H * W), "%s: N * C * H * W is too large; at most 2^40 elements", who);
  return HDIFF_OK;
}

}  // namespace

extern "C" {

int hdiff_relu_fwd(const float* x, float* y, int64_t n, hdiff_stream_t stream) {
  const int rc = check_count("relu_fwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && y, "relu_fwd: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(relu_fwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, x, y, n);
  HDIFF_CHECK_LAUNCH("relu_fwd kernel");
  return HDIFF_OK;
}

int hdiff_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, hdiff_stream_t stream) {
  const int rc = check_count("relu_bwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(y && dy && dx, "relu_bwd: null pointer");
  HDIFF_CHECK_ARG(dx != y && dx != dy, "relu_bwd: dx must not alias y or dy");
  (void)hipGetLastError();
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, y, dy, dx, n);
  HDIFF_CHECK_LAUNCH("relu_bwd kernel");
  return HDIFF_OK;
}

int hdiff_maxpool2_fwd(const float* x, float* y, int64_t planes, int H, int W, hdiff_stream_t stream) {
  const int rc = check_planes("maxpool2_fwd", planes, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && y, "maxpool2_fwd: null pointer");
  (void)hipGetLastError();
  const int64_t n = planes * (H / 2) * (W / 2);
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(grid_ceil_8k(n, 2)), dim3(kThreads), 0, (hipStream_t)stream, x, y, planes, H, W);
  HDIFF_CHECK_LAUNCH("maxpool2_fwd kernel");
  return HDIFF_OK;
}

int hdiff_maxpool2_bwd(const float* x, const float* dy, float* dx, int64_t planes, int H, int W, hdiff_stream_t stream) {
  const int rc = check_planes("maxpool2_bwd", planes, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && dy && dx, "maxpool2_bwd: null pointer");
  (void)hipGetLastError();
  const int64_t n = planes * H * W;
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, x, dy, dx, planes, H, W);
  HDIFF_CHECK_LAUNCH("maxpool2_bwd kernel");
  return HDIFF_OK;
}

int hdiff_l1_mean_workspace(int64_t n, int64_t* bytes) {
  const int rc = check_count("l1_mean_workspace", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "l1_mean_workspace: null pointer");
  *bytes = align256((int64_t)parts_for(n, kThreads * 8, kMaxParts) * (int64_t)sizeof(double));
  return HDIFF_OK;
}

int hdiff_l1_mean_fwd(const float* a, const float* b, int64_t n, float* out, void* scratch, hdiff_stream_t stream) {
  const int rc = check_count("l1_mean_fwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && out && scratch, "l1_mean_fwd: null pointer");
  (void)hipGetLastError();
  const int parts = parts_for(n, kThreads * 8, kMaxParts);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(parts), dim3(kThreads), 0, (hipStream_t)stream, a, b, n, (double*)scratch);
  hipLaunchKernelGGL(l1_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)scratch, parts, n, out);
  HDIFF_CHECK_LAUNCH("l1_mean_fwd kernels");
  return HDIFF_OK;
}

int hdiff_l1_mean_bwd(const float* a, const float* b, const float* g, int64_t n, float* da, hdiff_stream_t stream) {
  const int rc = check_count("l1_mean_bwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && g && da, "l1_mean_bwd: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, a, b, g, n, da);
  HDIFF_CHECK_LAUNCH("l1_mean_bwd kernel");
  return HDIFF_OK;
}

int hdiff_charbonnier_fwd(const float* a, const float* b, float* y, int64_t n, hdiff_stream_t stream) {
  const int rc = check_count("charbonnier_fwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && b && y, "charbonnier_fwd: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(charbonnier_fwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, a, b, y, n);
  HDIFF_CHECK_LAUNCH("charbonnier_fwd kernel");
  return HDIFF_OK;
}

int hdiff_charbonnier_bwd(const float* a, const float* b, const float* dy, int dy_is_scalar, float divisor, float* da, int64_t n,
                          hdiff_stream_t stream) {
  const int rc = check_count("charbonnier_bwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && b && dy && da, "charbonnier_bwd: null pointer");
  HDIFF_CHECK_ARG(dy_is_scalar == 0 || dy_is_scalar == 1, "charbonnier_bwd: dy_is_scalar = %d; 0 or 1", dy_is_scalar);
  HDIFF_CHECK_ARG(divisor >= 1.0f && divisor <= 3.402823466e+38f, "charbonnier_bwd: divisor = %g; finite and at least 1",
                  (double)divisor);
  (void)hipGetLastError();
  hipLaunchKernelGGL(charbonnier_bwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, a, b, dy,
                     dy_is_scalar ? 0 : 1, divisor, da, n);
  HDIFF_CHECK_LAUNCH("charbonnier_bwd kernel");
  return HDIFF_OK;
}

int hdiff_lpips_layer_workspace(int N, int C, int H, int W, int64_t* bytes) {
  const int rc = check_features("lpips_layer_workspace", N, C, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "lpips_layer_workspace: null pointer");
  *bytes = align256((int64_t)N * parts_for((int64_t)H * W, kThreads, kMaxParts) * (int64_t)sizeof(double));
  return HDIFF_OK;
}

int hdiff_lpips_layer(const float* f0, const float* f1, const float* w, int N, int C, int H, int W, double* out, void* scratch,
                      hdiff_stream_t stream) {
  const int rc = check_features("lpips_layer", N, C, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(f0 && f1 && w && out && scratch, "lpips_layer: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  const int parts = parts_for(HW, kThreads, kMaxParts);
  hipLaunchKernelGGL(lpips_partial_kernel, dim3(parts, 1, N), dim3(kThreads), 0, (hipStream_t)stream, f0, f1, w, C, HW,
                     (double*)scratch);
  hipLaunchKernelGGL(lpips_finalize_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, (const double*)scratch, parts, HW, out);
  HDIFF_CHECK_LAUNCH("lpips_layer kernels");
  return HDIFF_OK;
}

int hdiff_scale_input(const float* x, const float* shift, const float* scale, float mul, float add, float* y, int N, int C, int H,
                      int W, hdiff_stream_t stream) {
  const int rc = check_features("scale_input", N, C, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && shift && scale && y, "scale_input: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W, n = (int64_t)N * C * HW;
  hipLaunchKernelGGL(scale_input_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, x, shift, scale, mul, add,
                     y, C, HW, n);
  HDIFF_CHECK_LAUNCH("scale_input kernel");
  return HDIFF_OK;
}

}  // extern "C"
