// Training kernels of the reference's second tree (diffusion/Diffusion.py:26-180 GaussianDiffusionTrainer, diffusion/Model.py
// ConditionalEmbedding and the skip resize of DynamicUNet): the fused loss tail and the backward passes of the global average
// pool and the nearest resize.  All HBM-bound streaming kernels; compiled with -ffp-contract=off so that the forward rounds like
// the reference's separate tensor ops.  Every reduction is a fixed-order two-stage sum (no float atomics): bitwise reproducible.
// The loss tail takes what the network predicts (eps, or v of Salimans & Ho 2022), an optional min-SNR weight table for the squared
// error and the y0 divisor as launch-uniform arguments; the reference's tail is (eps, no table, 255).
#include "common.h"
#include "reduce.h"

using namespace hdiff;

#pragma clang fp contract(off)

namespace {

constexpr int kTailThreads = 256;      // workgroup of the two loss kernels: their block sums are instantiated for it
constexpr int kTailMaxBlocks = 1024;

__device__ __forceinline__ int clamp_t(int64_t t, int T) { return t < 0 ? 0 : (t >= T ? T - 1 : (int)t); }

// What the network's output `out` stands for (hdiff.h: HDIFF_PREDICT_*), with a = sa[t], s = s1m[t]:
//   eps:  target = noise              y0 = ((1 / a) * (y_t - s * out)) / div     dy0/dout = -(1 / a) * s / div
//   v:    target = a * noise - s * gt y0 = (a * y_t - s * out) / div             dy0/dout = -s / div       (Salimans & Ho 2022)

// One thread per pixel (b, p) of P = B * HW; channel c of pixel p of sample b sits at (b * 3 + c) * HW + p.
//   mse = [w[t] *] (out - target)^2                                 F.mse_loss(reduction='none')        (Diffusion.py:102)
//   y0  = as above; eps with div = 255 is the reference's own line, trailing / 255 and all (sic)        (Diffusion.py:106-107)
//   cos = <a, g> / (max(|a|, 1e-8) max(|g|, 1e-8)), a = y0 / max(|y0|, 1e-12), g = gt / max(|gt|, 1e-12)
//                                                                   F.normalize + F.cosine_similarity (Loss/loss.py:260-262)
// w_tab (may be NULL: no multiply is executed) weights the squared error alone.  `mode` and w_tab are uniform per launch.
// partial[block] = the block's sum of cos (double); the finaliser forms col = 1 - mean(cos).
__global__ void train_b_tail_fwd_kernel(const float* __restrict__ np_, const float* __restrict__ noise,
                                        const float* __restrict__ yt, const float* __restrict__ gt,
                                        const int64_t* __restrict__ t, const float* __restrict__ sa_tab,
                                        const float* __restrict__ s1m_tab, const float* __restrict__ w_tab, int mode, float div,
                                        int T, int HW, int64_t P, float* __restrict__ mse, float* __restrict__ y0,
                                        double* __restrict__ partial) {
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, p = q - b * HW;
    const int k = clamp_t(t[b], T);
    const float sa = sa_tab[k], s1m = s1m_tab[k];
    const float r = 1.0f / sa;
    const float w = w_tab ? w_tab[k] : 1.0f;
    float u[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t i = (b * 3 + c) * HW + p;
      const float e = np_[i];
      g[c] = gt[i];
      const float target = mode == HDIFF_PREDICT_V ? sa * noise[i] - s1m * g[c] : noise[i];
      const float d = e - target;
      mse[i] = w_tab ? w * (d * d) : d * d;
      const float v = mode == HDIFF_PREDICT_V ? (sa * yt[i] - s1m * e) / div : (r * (yt[i] - s1m * e)) / div;
      y0[i] = v;
      u[c] = v;
    }
    const float nu = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
    const float ng = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), 1e-12f);
    float a[3], bn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = u[c] / nu; bn[c] = g[c] / ng; }
    const float na = fmaxf(sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), 1e-8f);
    const float nb = fmaxf(sqrtf(bn[0] * bn[0] + bn[1] * bn[1] + bn[2] * bn[2]), 1e-8f);
    acc += (double)((a[0] / na) * (bn[0] / nb) + (a[1] / na) * (bn[1] / nb) + (a[2] / na) * (bn[2] / nb));
  }
  const double s = block_sum_to0<kTailThreads>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup: col[0] = 1 - (sum of the partials in index order) / P.
__global__ void train_b_loss_finalize_kernel(const double* __restrict__ partial, int nparts, int64_t P, float* __restrict__ col) {
  const double s = sum_partials_to0<kTailThreads>(partial, nparts, 1);
  if (threadIdx.x == 0) col[0] = 1.0f - (float)(s / (double)P);
}

// d out = d_mse * [w[t] *] 2 (out - target) + (d_y0 + d_col * dcol/dy0) * dy0/dout, target and dy0/dout as listed above.
// dcol/du (u = y0 of one pixel) is -1/P dcos/du, with torch's eps semantics:
//   dcos/da = g / (na_c nb_c) - cos / na_c * (|a| > 0 ? a / |a| : 0)          (the norm's backward uses the unclamped norm)
//   dcos/du = |u| >= 1e-12 ? (dcos/da) / |u| - u <u, dcos/da> / |u|^3 : (dcos/da) / 1e-12     (F.normalize's clamp_min)
// d_mse, d_y0 and d_col may each be NULL (no gradient flows into that output).
__global__ void train_b_tail_bwd_kernel(const float* __restrict__ np_, const float* __restrict__ noise,
                                        const float* __restrict__ y0, const float* __restrict__ gt,
                                        const int64_t* __restrict__ t, const float* __restrict__ sa_tab,
                                        const float* __restrict__ s1m_tab, const float* __restrict__ w_tab, int mode, float div,
                                        int T, int HW, int64_t P, const float* __restrict__ d_mse,
                                        const float* __restrict__ d_y0, const float* __restrict__ d_col,
                                        float* __restrict__ d_np) {
  const float dc = d_col ? -d_col[0] / (float)P : 0.0f;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, p = q - b * HW;
    const int k = clamp_t(t[b], T);
    const float sa = sa_tab[k], s1m = s1m_tab[k];
    const float chain = mode == HDIFF_PREDICT_V ? -s1m / div : -(1.0f / sa) * s1m / div;
    const float w = w_tab ? w_tab[k] : 1.0f;
    float u[3], g[3], gu[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t i = (b * 3 + c) * HW + p;
      u[c] = y0[i];
      g[c] = gt[i];
    }
    if (dc != 0.0f) {
      const float nu_raw = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
      const float nu = fmaxf(nu_raw, 1e-12f);
      const float ng = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), 1e-12f);
      float a[3], bn[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { a[c] = u[c] / nu; bn[c] = g[c] / ng; }
      const float na_raw = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
      const float na = fmaxf(na_raw, 1e-8f);
      const float nb = fmaxf(sqrtf(bn[0] * bn[0] + bn[1] * bn[1] + bn[2] * bn[2]), 1e-8f);
      const float cosv = (a[0] / na) * (bn[0] / nb) + (a[1] / na) * (bn[1] / nb) + (a[2] / na) * (bn[2] / nb);
      float ga[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        ga[c] = dc * (bn[c] / (na * nb) - (na_raw > 0.0f ? (cosv / na) * (a[c] / na_raw) : 0.0f));
      if (nu_raw >= 1e-12f) {
        const float dot = u[0] * ga[0] + u[1] * ga[1] + u[2] * ga[2];
        const float n3 = nu_raw * nu_raw * nu_raw;
#pragma unroll
        for (int c = 0; c < 3; ++c) gu[c] = ga[c] / nu_raw - u[c] * (dot / n3);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) gu[c] = ga[c] / 1e-12f;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t i = (b * 3 + c) * HW + p;
      float gy = gu[c];
      if (d_y0) gy += d_y0[i];
      float v = gy * chain;
      if (d_mse) {
        const float target = mode == HDIFF_PREDICT_V ? sa * noise[i] - s1m * g[c] : noise[i];
        const float d2 = 2.0f * (np_[i] - target);
        v += d_mse[i] * (w_tab ? w * d2 : d2);
      }
      d_np[i] = v;
    }
  }
}

// nn.AdaptiveAvgPool2d((1, 1)) backward: dx[bc][i] = dy[bc] / HW
__global__ void avgpool_global_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int HW, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dx[i] = dy[i / HW] / (float)HW;
}

// The forward's source index (model_b_ops.hip resize_nearest_kernel): min(floor(o * s), in - 1), s = (float)in / out.
__device__ __forceinline__ int nearest_src(int o, float s, int in) { return min((int)floorf(o * s), in - 1); }

// First output index o in [0, out) with nearest_src(o) >= i (out if none): the source map is non-decreasing in o.
__device__ int first_out_at_or_after(int i, float s, int in, int out) {
  int lo = 0, hi = out;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nearest_src(mid, s, in) >= i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// F.interpolate(mode="nearest") backward in gather form: each input element sums the outputs that read it, rows then
// columns in increasing order -- no atomics, so the result does not depend on scheduling.
__global__ void resize_nearest_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int H, int W, int OH, int OW,
                                          float sy, float sx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = (int)(i % W);
    const int64_t r = i / W;
    const int iy = (int)(r % H);
    const int64_t bc = r / H;
    const int oy0 = first_out_at_or_after(iy, sy, H, OH), oy1 = first_out_at_or_after(iy + 1, sy, H, OH);
    const int ox0 = first_out_at_or_after(ix, sx, W, OW), ox1 = first_out_at_or_after(ix + 1, sx, W, OW);
    const float* src = dy + bc * OH * OW;
    float s = 0.f;
    for (int oy = oy0; oy < oy1; ++oy)
      for (int ox = ox0; ox < ox1; ++ox) s += src[(int64_t)oy * OW + ox];
    dx[i] = s;
  }
}

}  // namespace

extern "C" {

int hdiff_train_b_loss_workspace(int64_t pixels, int64_t* bytes) {
  HDIFF_CHECK_ARG(bytes && pixels > 0, "train_b_loss_workspace: bad arguments");
  *bytes = (int64_t)parts_for(pixels, kTailThreads, kTailMaxBlocks) * (int64_t)sizeof(double);
  return HDIFF_OK;
}

int hdiff_train_b_tail_fwd(const float* out, const float* noise, const float* y_t, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, float* mse, float* y0_pred,
                           float* col, void* workspace, int prediction, const float* weight_tab, float y0_div,
                           hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(out && noise && y_t && gt && t && sqrt_ab && sqrt_1mab && mse && y0_pred && col && workspace,
                  "train_b_tail_fwd: null pointer");
  HDIFF_CHECK_ARG(T > 0 && B > 0 && HW > 0, "train_b_tail_fwd: bad sizes");
  HDIFF_CHECK_ARG(prediction == HDIFF_PREDICT_EPS || prediction == HDIFF_PREDICT_V, "train_b_tail_fwd: unknown prediction %d",
                  prediction);
  HDIFF_CHECK_ARG(y0_div == y0_div && y0_div != 0.0f, "train_b_tail_fwd: y0_div must be a number other than 0");
  (void)hipGetLastError();
  const int64_t P = (int64_t)B * HW;
  const int nb = parts_for(P, kTailThreads, kTailMaxBlocks);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(train_b_tail_fwd_kernel, dim3(nb), dim3(kTailThreads), 0, (hipStream_t)stream, out, noise, y_t, gt, t,
                     sqrt_ab, sqrt_1mab, weight_tab, prediction, y0_div, T, HW, P, mse, y0_pred, part);
  hipLaunchKernelGGL(train_b_loss_finalize_kernel, dim3(1), dim3(kTailThreads), 0, (hipStream_t)stream, part, nb, P, col);
  HDIFF_CHECK_LAUNCH("train_b_tail_fwd kernels");
  return HDIFF_OK;
}

int hdiff_train_b_tail_bwd(const float* out, const float* noise, const float* y0_pred, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, const float* d_mse,
                           const float* d_y0, const float* d_col, float* d_out, int prediction, const float* weight_tab,
                           float y0_div, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(out && noise && y0_pred && gt && t && sqrt_ab && sqrt_1mab && d_out, "train_b_tail_bwd: null pointer");
  HDIFF_CHECK_ARG(T > 0 && B > 0 && HW > 0, "train_b_tail_bwd: bad sizes");
  HDIFF_CHECK_ARG(prediction == HDIFF_PREDICT_EPS || prediction == HDIFF_PREDICT_V, "train_b_tail_bwd: unknown prediction %d",
                  prediction);
  HDIFF_CHECK_ARG(y0_div == y0_div && y0_div != 0.0f, "train_b_tail_bwd: y0_div must be a number other than 0");
  (void)hipGetLastError();
  const int64_t P = (int64_t)B * HW;
  hipLaunchKernelGGL(train_b_tail_bwd_kernel, dim3(grid_ceil_8k(P)), dim3(256), 0, (hipStream_t)stream, out, noise, y0_pred, gt,
                     t, sqrt_ab, sqrt_1mab, weight_tab, prediction, y0_div, T, HW, P, d_mse, d_y0, d_col, d_out);
  HDIFF_CHECK_LAUNCH("train_b_tail_bwd_kernel");
  return HDIFF_OK;
}

// the reference's own tail: eps-prediction, no weights, y0 / 255 -- the same kernels, the same bits as before they took arguments
int hdiff_train_b_loss_fwd(const float* noise_pred, const float* noise, const float* y_t, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, float* mse, float* y0_pred,
                           float* col, void* workspace, hdiff_stream_t stream) {
  return hdiff_train_b_tail_fwd(noise_pred, noise, y_t, gt, t, sqrt_ab, sqrt_1mab, T, B, HW, mse, y0_pred, col, workspace,
                                HDIFF_PREDICT_EPS, nullptr, 255.0f, stream);
}

int hdiff_train_b_loss_bwd(const float* noise_pred, const float* noise, const float* y0_pred, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, const float* d_mse,
                           const float* d_y0, const float* d_col, float* d_noise_pred, hdiff_stream_t stream) {
  return hdiff_train_b_tail_bwd(noise_pred, noise, y0_pred, gt, t, sqrt_ab, sqrt_1mab, T, B, HW, d_mse, d_y0, d_col, d_noise_pred,
                                HDIFF_PREDICT_EPS, nullptr, 255.0f, stream);
}

int hdiff_avgpool_global_bwd(const float* dy, float* dx, int BC, int HW, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(dy && dx && BC > 0 && HW > 0, "avgpool_global_bwd: bad arguments");
  (void)hipGetLastError();
  const int64_t n = (int64_t)BC * HW;
  hipLaunchKernelGGL(avgpool_global_bwd_kernel, dim3(grid_ceil_8k(n)), dim3(256), 0, (hipStream_t)stream, dy, dx, HW, n);
  HDIFF_CHECK_LAUNCH("avgpool_global_bwd_kernel");
  return HDIFF_OK;
}

int hdiff_resize_nearest_bwd(const float* dy, float* dx, int BC, int H, int W, int OH, int OW, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(dy && dx && BC > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "resize_nearest_bwd: bad arguments");
  (void)hipGetLastError();
  const int64_t n = (int64_t)BC * H * W;
  hipLaunchKernelGGL(resize_nearest_bwd_kernel, dim3(grid_ceil_8k(n)), dim3(256), 0, (hipStream_t)stream, dy, dx, H, W, OH, OW,
                     (float)H / (float)OH, (float)W / (float)OW, n);
  HDIFF_CHECK_LAUNCH("resize_nearest_bwd_kernel");
  return HDIFF_OK;
}

}  // extern "C"
