// The pieces of a DINOv2 ViT trunk that the conv and attention kernels do not cover, and the smooth-L1 arithmetic that sits on its
// taps (hdiff_amd/dino.py is the caller; tests/_dino_def.py holds the definitions the kernels are held to).  Activations are fp32,
// channel-major [B][C][L] with the class token at position 0; every kernel puts neighbouring lanes on neighbouring positions of L:
//   crop + 14x14 patch unfold and its adjoint (fold)                pure gathers, bit for bit
//   token assembly (class token, position embedding) and its slice  one fp32 add per element, bit for bit
//   LayerNorm over C per token, forward and input gradient          statistics in double, two passes over the row (below)
//   exact GELU, forward and backward                                evaluated in double through erfc, rounded once
//   LayerScale with the residual add, and its backward              one rounding per written operation
//   the smooth-L1 tap, the sum of the slots, and the tap's backward double sums in a fixed order; the gradient in fp32
// The dense layers of the trunk are autograd.fused_conv(k=1)'s and the attention core is hdiff_mha_flash_*: nothing here multiplies
// matrices.  Every entry validates on the host before a launch, allocates nothing, never synchronises, uses no float atomics and
// gives bitwise repeatable results; every grid is a function of the per-image sizes alone and no sum runs across images before the
// very last one, so an image's numbers do not depend on the batch it was computed in.  Compiled with -ffp-contract=off.
//
// LayerNorm statistics.  groupnorm.hip reads a (sample, group) slice of up to millions of elements ONCE and therefore sums
// d = x - K around a pivot K in fp32 (its comment explains how K is chosen so that the cancellation stays bounded).  A LayerNorm
// row here is C <= 4096 values that a workgroup reads again from cache, so the plain two-pass form is affordable: the mean first,
// then the squared deviations from it, both in double.  A row whose mean is 1e3 times its spread loses nothing (the deviations are
// exact differences of fp32 values in double), and a constant row has deviation exactly 0, so its output is beta exactly.
#include <math.h>

#include "common.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kPatch = 14;               // DINOv2's patch side
constexpr int kCrop = 2;                 // pixels removed from every edge before the patches are cut
constexpr int kTok = 64;                 // tokens per LayerNorm workgroup: one wave along L ...
constexpr int kGrp = kThreads / kTok;    // ... times 4 channel groups
constexpr int kMaxParts = 64;            // partial sums per image of one tap
constexpr int kMaxBatch = 256;           // images per call of the tap kernels
constexpr int64_t kMaxElems = 1ll << 31; // elements per tensor

// ---------------------------------------------------------------------------------------------------------- unfold / fold
// cols[b][(c*14 + ky)*14 + kx][py*w + px] = x[b][c][2 + 14 py + ky][2 + 14 px + kx]: the row order of Conv2d(3, C, 14, 14).weight
// flattened to [C][588].  One thread per OUTPUT element, consecutive threads on consecutive patches.
__global__ __launch_bounds__(kThreads) void unfold_kernel(const float* __restrict__ x, float* __restrict__ cols, int H, int W, int h,
                                                           int w, int64_t n) {
  const int hw = h * w;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int p = (int)(i % hw);
    const int64_t t = i / hw;
    const int r = (int)(t % (3 * kPatch * kPatch));
    const int64_t b = t / (3 * kPatch * kPatch);
    const int kx = r % kPatch, ky = (r / kPatch) % kPatch, c = r / (kPatch * kPatch);
    const int py = p / w, px = p % w;
    cols[i] = x[((b * 3 + c) * H + (kCrop + py * kPatch + ky)) * W + (kCrop + px * kPatch + kx)];
  }
}

// the adjoint as a gather: every pixel of the image asks which column element it fed; the 2-pixel border fed none and gets 0
__global__ __launch_bounds__(kThreads) void fold_kernel(const float* __restrict__ dcols, float* __restrict__ dx, int H, int W, int h,
                                                         int w, int64_t n) {
  const int hw = h * w;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int xx = (int)(i % W);
    const int64_t t = i / W;
    const int yy = (int)(t % H);
    const int64_t bc = t / H;                // b * 3 + c
    const int uy = yy - kCrop, ux = xx - kCrop;
    float g = 0.0f;
    if (uy >= 0 && ux >= 0 && uy < h * kPatch && ux < w * kPatch) {
      const int py = uy / kPatch, ky = uy % kPatch, px = ux / kPatch, kx = ux % kPatch;
      const int64_t b = bc / 3;
      const int c = (int)(bc % 3);
      g = dcols[((b * 3 + c) * (kPatch * kPatch) + ky * kPatch + kx) * hw + py * w + px];
    }
    dx[i] = g;
  }
}

// ------------------------------------------------------------------------------------------------------------ token assembly
// tok[b][c][0] = cls[c] + pos[c][0];  tok[b][c][l] = patch[b][c][l - 1] + pos[c][l]   (pos is [C][L], resized on the host)
__global__ __launch_bounds__(kThreads) void tokens_fwd_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                               const float* __restrict__ pos, float* __restrict__ tok, int Cc, int L,
                                                               int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int l = (int)(i % L);
    const int64_t bc = i / L;
    const int c = (int)(bc % Cc);
    const float v = l == 0 ? cls[c] : patch[bc * (L - 1) + (l - 1)];
    tok[i] = v + pos[(int64_t)c * L + l];
  }
}

__global__ __launch_bounds__(kThreads) void tokens_bwd_kernel(const float* __restrict__ dtok, float* __restrict__ dpatch, int L,
                                                               int64_t n) {
  const int P = L - 1;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t bc = i / P;
    dpatch[i] = dtok[bc * L + 1 + (i % P)];
  }
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm
// grid (ceil(L / 64), B); thread = (token lane, channel group g): group g owns channels g, g + 4, ...; the four group sums of a
// token meet in LDS and are added in group order by every thread alike.
__device__ __forceinline__ double token_sum4(double v, double (*sh)[kTok]) {
  const int lane = threadIdx.x & (kTok - 1), g = threadIdx.x / kTok;
  __syncthreads();                          // the previous use of sh is over
  sh[g][lane] = v;
  __syncthreads();
  double s = sh[0][lane];
#pragma unroll
  for (int k = 1; k < kGrp; ++k) s += sh[k][lane];
  return s;
}

__global__ __launch_bounds__(kThreads) void layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                                  double* __restrict__ mean_out, double* __restrict__ rstd_out, int Cc,
                                                                  int L) {
  __shared__ double sh[kGrp][kTok];
  const int lane = threadIdx.x & (kTok - 1), g = threadIdx.x / kTok;
  const int l = blockIdx.x * kTok + lane;
  const int b = blockIdx.y;
  const bool live = l < L;
  const float* xr = x + (int64_t)b * Cc * L + (live ? l : 0);
  double s = 0.0;
  if (live)
    for (int c = g; c < Cc; c += kGrp) s += (double)xr[(int64_t)c * L];
  const double mean = token_sum4(s, sh) / (double)Cc;
  double q = 0.0;
  if (live)
    for (int c = g; c < Cc; c += kGrp) {
      const double d = (double)xr[(int64_t)c * L] - mean;
      q += d * d;
    }
  const double var = token_sum4(q, sh) / (double)Cc;
  const double rstd = 1.0 / sqrt(var + (double)eps);
  if (!live) return;
  if (g == 0 && mean_out) {
    mean_out[(int64_t)b * L + l] = mean;
    rstd_out[(int64_t)b * L + l] = rstd;
  }
  float* yr = y + (int64_t)b * Cc * L + l;
  for (int c = g; c < Cc; c += kGrp) {
    const float xhat = (float)(((double)xr[(int64_t)c * L] - mean) * rstd);
    yr[(int64_t)c * L] = xhat * gamma[c] + beta[c];
  }
}

// dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) (+ add), g = dy * gamma, xhat = (x - mean) * rstd; sums in double
__global__ __launch_bounds__(kThreads) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                  const double* __restrict__ mean_in, const double* __restrict__ rstd_in,
                                                                  const float* __restrict__ dy, const float* add, float* dx, int Cc,
                                                                  int L) {
  __shared__ double sh[kGrp][kTok];
  const int lane = threadIdx.x & (kTok - 1), g = threadIdx.x / kTok;
  const int l = blockIdx.x * kTok + lane;
  const int b = blockIdx.y;
  const bool live = l < L;
  const int64_t base = (int64_t)b * Cc * L + (live ? l : 0);
  const double mean = live ? mean_in[(int64_t)b * L + l] : 0.0;
  const double rstd = live ? rstd_in[(int64_t)b * L + l] : 0.0;
  double s1 = 0.0, s2 = 0.0;
  if (live)
    for (int c = g; c < Cc; c += kGrp) {
      const int64_t o = base + (int64_t)c * L;
      const double gg = (double)dy[o] * (double)gamma[c];
      const double xhat = ((double)x[o] - mean) * rstd;
      s1 += gg;
      s2 += gg * xhat;
    }
  const double m1 = token_sum4(s1, sh) / (double)Cc;
  const double m2 = token_sum4(s2, sh) / (double)Cc;
  if (!live) return;
  for (int c = g; c < Cc; c += kGrp) {
    const int64_t o = base + (int64_t)c * L;
    const double gg = (double)dy[o] * (double)gamma[c];
    const double xhat = ((double)x[o] - mean) * rstd;
    const float v = (float)(rstd * ((gg - m1) - xhat * m2));
    dx[o] = add ? add[o] + v : v;           // (dx may be add itself: each element is read and written by one thread)
  }
}

// --------------------------------------------------------------------------------------------------------------------- GELU
// x * Phi(x) with Phi(x) = erfc(-x / sqrt 2) / 2 in double: no 1 + erf cancellation in the left tail, one rounding to fp32.
// The infinities take the limits, gelu(+inf) = +inf with slope 1 and gelu(-inf) = -0 with slope 0, where the formula itself would
// multiply an infinity by zero; a NaN goes through erfc and stays a NaN.
__device__ __forceinline__ float gelu_value(float x) {
  if (x == INFINITY) return INFINITY;
  if (x == -INFINITY) return -0.0f;
  const double v = (double)x;
  return (float)(v * (0.5 * erfc(-v * 0.70710678118654752440)));
}

__device__ __forceinline__ float gelu_slope(float x) {
  if (x == INFINITY) return 1.0f;
  if (x == -INFINITY) return 0.0f;
  const double v = (double)x;
  const double cdf = 0.5 * erfc(-v * 0.70710678118654752440);
  const double pdf = 0.39894228040143267794 * exp(-0.5 * v * v);
  return (float)(cdf + v * pdf);
}

__global__ __launch_bounds__(kThreads) void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) y[i] = gelu_value(x[i]);
}

__global__ __launch_bounds__(kThreads) void gelu_bwd_kernel(const float* __restrict__ x, const float* dy, float* dx,
                                                             int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    dx[i] = dy[i] * gelu_slope(x[i]);
}

// --------------------------------------------------------------------------------------------------------------- LayerScale
// s = gamma[c] * x (the LayerScale module's output, a tap; written when asked for) and y = res + s
__global__ __launch_bounds__(kThreads) void layerscale_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ res, float* __restrict__ s,
                                                                   float* __restrict__ y, int Cc, int L, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)((i / L) % Cc);
    const float v = gamma[c] * x[i];
    if (s) s[i] = v;
    y[i] = res[i] + v;
  }
}

__global__ __launch_bounds__(kThreads) void layerscale_bwd_kernel(const float* ds, const float* __restrict__ gamma,
                                                                   float* dx, int Cc, int L, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    dx[i] = gamma[(int)((i / L) % Cc)] * ds[i];
}

// ---------------------------------------------------------------------------------------------------------- smooth-L1 taps
// a tap is B images of n_img elements, element j of image b at a[b * img_stride + j * stride] (stride = L picks the class token
// of a [B][C][L] tensor).  grid (parts, B): part[b][p] = sum over the block's elements of smooth_l1(a - b), in double
__global__ __launch_bounds__(kThreads) void tap_partial_kernel(const float* __restrict__ a, const float* __restrict__ t, int64_t n_img,
                                                                int64_t stride, int64_t img_stride, double* __restrict__ part) {
  const float* pa = a + (int64_t)blockIdx.y * img_stride;
  const float* pt = t + (int64_t)blockIdx.y * img_stride;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_img; i += (int64_t)gridDim.x * kThreads) {
    const double d = (double)pa[i * stride] - (double)pt[i * stride];
    const double m = fabs(d);
    acc += m < 1.0 ? 0.5 * d * d : m - 0.5;        // a NaN difference takes the second branch and stays a NaN
  }
  const double s = block_sum_all<kThreads>(acc);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// grid (B), one wave: slot[b] = weight / n * (the image's parts in a fixed order)
__global__ __launch_bounds__(64) void tap_slot_kernel(const double* __restrict__ part, int parts, double coef, double* __restrict__ slot) {
  const int lane = threadIdx.x;
  const double v = lane < parts ? part[(int64_t)blockIdx.x * parts + lane] : 0.0;
  const double s = wave_sum(v);
  if (lane == 0) slot[blockIdx.x] = coef * s;
}

// one workgroup: thread b adds image b's slots in slot order; thread 0 adds the images in order and rounds once
__global__ __launch_bounds__(kThreads) void tap_total_kernel(const double* __restrict__ slots, int ntaps, int B, float* __restrict__ out,
                                                              float* __restrict__ per_image) {
  __shared__ double img[kMaxBatch];
  const int b = threadIdx.x;
  if (b < B) {
    double acc = 0.0;
    for (int k = 0; k < ntaps; ++k) acc += slots[(int64_t)k * B + b];
    img[b] = acc;
    if (per_image) per_image[b] = (float)acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int i = 0; i < B; ++i) acc += img[i];
    out[0] = (float)acc;
  }
}

// da_out = da_in + ((g * weight) / n) * clamp(a - t, -1, 1) in fp32, in that order; da_in may be NULL (0) or da_out itself
__global__ __launch_bounds__(kThreads) void tap_bwd_kernel(const float* __restrict__ a, const float* __restrict__ t,
                                                            const float* __restrict__ g, float weight, float count, const float* da_in,
                                                            float* da_out, int64_t n_img, int64_t stride, int64_t img_stride) {
  const float coef = g[0] * weight / count;
  const int64_t off = (int64_t)blockIdx.y * img_stride;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_img; i += (int64_t)gridDim.x * kThreads) {
    const int64_t o = off + i * stride;
    const float d = a[o] - t[o];
    const float cl = d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d);      // a NaN stays a NaN
    const float v = coef * cl;
    da_out[o] = da_in ? da_in[o] + v : v;
  }
}

// -------------------------------------------------------------------------------------------------------------------- checks
int check_count(const char* who, int64_t n) {
  HDIFF_CHECK_ARG(n >= 1 && n < kMaxElems, "%s: n = %lld; between 1 and 2^31 - 1 elements", who, (long long)n);
  return HDIFF_OK;
}

int check_bcl(const char* who, int B, int Cc, int L) {
  HDIFF_CHECK_ARG(B >= 1 && B <= 65535, "%s: B = %d; between 1 and 65535 images", who, B);
  HDIFF_CHECK_ARG(Cc >= 1 && Cc <= 4096, "%s: C = %d; between 1 and 4096 channels", who, Cc);
  HDIFF_CHECK_ARG(L >= 1 && L <= (1 << 20), "%s: L = %d; between 1 and 2^20 tokens", who, L);
  HDIFF_CHECK_ARG((int64_t)B * Cc * L < kMaxElems, "%s: B * C * L = %lld; fewer than 2^31 elements", who, (long long)B * Cc * L);
  return HDIFF_OK;
}

int check_image(const char* who, int B, int H, int W) {
  HDIFF_CHECK_ARG(B >= 1 && B <= 65535, "%s: B = %d; between 1 and 65535 images", who, B);
  HDIFF_CHECK_ARG(H > 2 * kCrop && W > 2 * kCrop && (H - 2 * kCrop) % kPatch == 0 && (W - 2 * kCrop) % kPatch == 0,
                  "%s: H = %d, W = %d; H - 4 and W - 4 must be positive multiples of 14", who, H, W);
  HDIFF_CHECK_ARG(H <= 16384 && W <= 16384 && (int64_t)B * 3 * H * W < kMaxElems, "%s: B * 3 * H * W = %lld is too large", who,
                  (long long)B * 3 * H * W);
  return HDIFF_OK;
}

int check_tap(const char* who, int B, int64_t n_img, int64_t stride, int64_t img_stride) {
  HDIFF_CHECK_ARG(B >= 1 && B <= kMaxBatch, "%s: B = %d; between 1 and %d images", who, B, kMaxBatch);
  HDIFF_CHECK_ARG(n_img >= 1 && stride >= 1 && n_img * stride < kMaxElems, "%s: n_img = %lld, stride = %lld; both at least 1, span below 2^31",
                  who, (long long)n_img, (long long)stride);
  HDIFF_CHECK_ARG(img_stride >= (n_img - 1) * stride + 1 && img_stride * B < kMaxElems * 2,
                  "%s: img_stride = %lld is shorter than an image's span", who, (long long)img_stride);
  return HDIFF_OK;
}

}  // namespace

extern "C" {

int hdiff_dino_unfold(const float* x, float* cols, int B, int H, int W, hdiff_stream_t stream) {
  const int rc = check_image("dino_unfold", B, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && cols, "dino_unfold: null pointer");
  (void)hipGetLastError();
  const int h = (H - 2 * kCrop) / kPatch, w = (W - 2 * kCrop) / kPatch;
  const int64_t n = (int64_t)B * 3 * kPatch * kPatch * h * w;
  hipLaunchKernelGGL(unfold_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, x, cols, H, W, h, w, n);
  HDIFF_CHECK_LAUNCH("dino_unfold kernel");
  return HDIFF_OK;
}

int hdiff_dino_fold(const float* dcols, float* dx, int B, int H, int W, hdiff_stream_t stream) {
  const int rc = check_image("dino_fold", B, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(dcols && dx, "dino_fold: null pointer");
  (void)hipGetLastError();
  const int h = (H - 2 * kCrop) / kPatch, w = (W - 2 * kCrop) / kPatch;
  const int64_t n = (int64_t)B * 3 * H * W;
  hipLaunchKernelGGL(fold_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, dcols, dx, H, W, h, w, n);
  HDIFF_CHECK_LAUNCH("dino_fold kernel");
  return HDIFF_OK;
}

int hdiff_dino_tokens_fwd(const float* patch, const float* cls, const float* pos, float* tok, int B, int C, int L,
                          hdiff_stream_t stream) {
  const int rc = check_bcl("dino_tokens_fwd", B, C, L);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(L >= 2, "dino_tokens_fwd: L = %d; the class token and at least one patch", L);
  HDIFF_CHECK_ARG(patch && cls && pos && tok, "dino_tokens_fwd: null pointer");
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * L;
  hipLaunchKernelGGL(tokens_fwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, patch, cls, pos, tok, C, L, n);
  HDIFF_CHECK_LAUNCH("dino_tokens_fwd kernel");
  return HDIFF_OK;
}

int hdiff_dino_tokens_bwd(const float* dtok, float* dpatch, int B, int C, int L, hdiff_stream_t stream) {
  const int rc = check_bcl("dino_tokens_bwd", B, C, L);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(L >= 2, "dino_tokens_bwd: L = %d; the class token and at least one patch", L);
  HDIFF_CHECK_ARG(dtok && dpatch, "dino_tokens_bwd: null pointer");
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * (L - 1);
  hipLaunchKernelGGL(tokens_bwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, dtok, dpatch, L, n);
  HDIFF_CHECK_LAUNCH("dino_tokens_bwd kernel");
  return HDIFF_OK;
}

int hdiff_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, double* mean, double* rstd, int B,
                        int C, int L, hdiff_stream_t stream) {
  const int rc = check_bcl("layernorm_fwd", B, C, L);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && gamma && beta && y, "layernorm_fwd: null pointer");
  HDIFF_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "layernorm_fwd: mean and rstd come together");
  HDIFF_CHECK_ARG(eps > 0.0f && eps < 1.0f, "layernorm_fwd: eps = %g; in (0, 1)", (double)eps);
  (void)hipGetLastError();
  hipLaunchKernelGGL(layernorm_fwd_kernel, dim3((L + kTok - 1) / kTok, B), dim3(kThreads), 0, (hipStream_t)stream, x, gamma, beta, eps,
                     y, mean, rstd, C, L);
  HDIFF_CHECK_LAUNCH("layernorm_fwd kernel");
  return HDIFF_OK;
}

int hdiff_layernorm_bwd(const float* x, const float* gamma, const double* mean, const double* rstd, const float* dy, const float* add,
                        float* dx, int B, int C, int L, hdiff_stream_t stream) {
  const int rc = check_bcl("layernorm_bwd", B, C, L);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && gamma && mean && rstd && dy && dx, "layernorm_bwd: null pointer");
  HDIFF_CHECK_ARG(dx != x && dx != dy, "layernorm_bwd: dx must not alias x or dy");
  (void)hipGetLastError();
  hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((L + kTok - 1) / kTok, B), dim3(kThreads), 0, (hipStream_t)stream, x, gamma, mean, rstd,
                     dy, add, dx, C, L);
  HDIFF_CHECK_LAUNCH("layernorm_bwd kernel");
  return HDIFF_OK;
}

int hdiff_gelu_fwd(const float* x, float* y, int64_t n, hdiff_stream_t stream) {
  const int rc = check_count("gelu_fwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && y, "gelu_fwd: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(grid_ceil_8k(n, 2)), dim3(kThreads), 0, (hipStream_t)stream, x, y, n);
  HDIFF_CHECK_LAUNCH("gelu_fwd kernel");
  return HDIFF_OK;
}

int hdiff_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, hdiff_stream_t stream) {
  const int rc = check_count("gelu_bwd", n);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && dy && dx, "gelu_bwd: null pointer");
  HDIFF_CHECK_ARG(dx != x, "gelu_bwd: dx must not alias x");
  (void)hipGetLastError();
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(grid_ceil_8k(n, 2)), dim3(kThreads), 0, (hipStream_t)stream, x, dy, dx, n);
  HDIFF_CHECK_LAUNCH("gelu_bwd kernel");
  return HDIFF_OK;
}

int hdiff_layerscale_fwd(const float* x, const float* gamma, const float* res, float* s, float* y, int B, int C, int L,
                         hdiff_stream_t stream) {
  const int rc = check_bcl("layerscale_fwd", B, C, L);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && gamma && res && y, "layerscale_fwd: null pointer");
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * L;
  hipLaunchKernelGGL(layerscale_fwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, x, gamma, res, s, y, C, L, n);
  HDIFF_CHECK_LAUNCH("layerscale_fwd kernel");
  return HDIFF_OK;
}

int hdiff_layerscale_bwd(const float* ds, const float* gamma, float* dx, int B, int C, int L, hdiff_stream_t stream) {
  const int rc = check_bcl("layerscale_bwd", B, C, L);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(ds && gamma && dx, "layerscale_bwd: null pointer");
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * L;
  hipLaunchKernelGGL(layerscale_bwd_kernel, dim3(grid_ceil_8k(n, 4)), dim3(kThreads), 0, (hipStream_t)stream, ds, gamma, dx, C, L, n);
  HDIFF_CHECK_LAUNCH("layerscale_bwd kernel");
  return HDIFF_OK;
}

int hdiff_smooth_l1_tap_workspace(int B, int64_t n_img, int64_t* bytes) {
  const int rc = check_tap("smooth_l1_tap_workspace", B, n_img, 1, n_img);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "smooth_l1_tap_workspace: null pointer");
  *bytes = align256((int64_t)B * parts_for(n_img, kThreads * 8, kMaxParts) * (int64_t)sizeof(double));
  return HDIFF_OK;
}

int hdiff_smooth_l1_tap_fwd(const float* a, const float* t, int B, int64_t n_img, int64_t stride, int64_t img_stride, double weight,
                            double* slot, void* scratch, hdiff_stream_t stream) {
  const int rc = check_tap("smooth_l1_tap_fwd", B, n_img, stride, img_stride);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && t && slot && scratch, "smooth_l1_tap_fwd: null pointer");
  HDIFF_CHECK_ARG(weight >= 0.0 && weight <= 1e30, "smooth_l1_tap_fwd: weight = %g; finite and not negative", weight);
  (void)hipGetLastError();
  const int parts = parts_for(n_img, kThreads * 8, kMaxParts);
  hipLaunchKernelGGL(tap_partial_kernel, dim3(parts, B), dim3(kThreads), 0, (hipStream_t)stream, a, t, n_img, stride, img_stride,
                     (double*)scratch);
  hipLaunchKernelGGL(tap_slot_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, parts,
                     weight / ((double)B * (double)n_img), slot);
  HDIFF_CHECK_LAUNCH("smooth_l1_tap_fwd kernels");
  return HDIFF_OK;
}

int hdiff_smooth_l1_tap_total(const double* slots, int ntaps, int B, float* out, float* per_image, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(ntaps >= 1 && ntaps <= 65536, "smooth_l1_tap_total: ntaps = %d; between 1 and 65536", ntaps);
  HDIFF_CHECK_ARG(B >= 1 && B <= kMaxBatch, "smooth_l1_tap_total: B = %d; between 1 and %d images", B, kMaxBatch);
  HDIFF_CHECK_ARG(slots && out, "smooth_l1_tap_total: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(tap_total_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, slots, ntaps, B, out, per_image);
  HDIFF_CHECK_LAUNCH("smooth_l1_tap_total kernel");
  return HDIFF_OK;
}

int hdiff_smooth_l1_tap_bwd(const float* a, const float* t, const float* g, int B, int64_t n_img, int64_t stride, int64_t img_stride,
                            float weight, const float* da_in, float* da_out, hdiff_stream_t stream) {
  const int rc = check_tap("smooth_l1_tap_bwd", B, n_img, stride, img_stride);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && t && g && da_out, "smooth_l1_tap_bwd: null pointer");
  HDIFF_CHECK_ARG(da_out != a && da_out != t, "smooth_l1_tap_bwd: da_out must not alias a or t");
  HDIFF_CHECK_ARG(weight >= 0.0f && weight <= 1e30f, "smooth_l1_tap_bwd: weight = %g; finite and not negative", (double)weight);
  (void)hipGetLastError();
  hipLaunchKernelGGL(tap_bwd_kernel, dim3(grid_ceil_8k(n_img, 4), B), dim3(kThreads), 0, (hipStream_t)stream, a, t, g, weight,
                     (float)((double)B * (double)n_img), da_in, da_out, n_img, stride, img_stride);
  HDIFF_CHECK_LAUNCH("smooth_l1_tap_bwd kernel");
  return HDIFF_OK;
}

}  // extern "C"
