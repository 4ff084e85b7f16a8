// Guided full-resolution transfer: carry an enhancement that the model made at its own size to an image of any size (He et al.'s
// guided filter with a colour guide in its "fast" form; tests/_transfer_def.py is the definition the kernels are held to,
// hdiff_amd/transfer.py the caller).  Three steps, two entries each:
//   resample   uint8 [H][W][3] -> float [3][h][w] in [0, 255]: a triangle filter of support max(in / out, 1) per axis, horizontal pass
//              first, weights normalised in double, products added in tap order in double, the [H][w][3] intermediate kept in double,
//              one rounding to fp32 (Pillow's BILINEAR reduce without its 8-bit rounding between the passes).  Two launches.
//   fit        per pixel of the small pair (I, p): the affine colour map p ~ a I + b of its clipped (2r+1)^2 window, a = (cov(I) +
//              eps U)^-1 cov(I, p) by Cholesky, then the window mean of the twelve values.  Double from the loads to the one rounding;
//              every window sum is separable (x, then y) and a DIRECT sum in index order: no integral image, no sliding update (a
//              prefix over 65 536 values leaves 1e-11 in a mean, 1e-7 of the 1e-4-sized covariances the solve divides by).  Four launches.
//   apply      q_c = A_c0 F_0 + A_c1 F_1 + A_c2 F_2 + b_c at every pixel of the large image, the twelve planes interpolated bilinearly
//              (half-pixel centres, clamped; along x at both rows, then along y).  fp32; the feature's hot path.  One launch.
// Images on blockIdx.z; nothing is shared between images, so a non-finite value spoils its own image only and an image's numbers do not
// depend on N.  No allocation, no synchronisation, no atomics.
//
// The apply kernel.  A workgroup owns kTileRows rows of a strip of 256 lanes x 4 consecutive pixels.  Where the strip's coefficient
// columns fit (kStageCols; any magnification above about 2.7), the two coefficient rows of the current output row are staged in LDS,
// as many columns of 24 floats as the geometry needs (68 at 4032 from 256: 6.4 KiB), and staged again only when the row pair
// changes (every H / h rows): a pixel then costs twelve 16-byte LDS reads, not 48 loads.  Otherwise (equal size, reduction) the same
// pixel routine reads the planes in place.  The 256 quotients byte / 255 are divided once per workgroup and looked up.  The position
// of a pixel among the coefficient pixels is taken in integers, n = (2 X + 1) w - W over 2 W, so the tap is exact and its weight
// carries two roundings (the reciprocal of 2 W, the product with the remainder); a lerp is the convex form (1 - f) a + f b, whose
// error is relative to the interpolated magnitudes.
// A uint8 row is 3 W bytes and starts on any byte: the first (address mod 4) pixels of a row and its last (W - head) mod 4 are moved
// byte by byte, every group of four in between as three aligned words.  A lane reads all it needs of its pixels before it writes
// them and no two lanes share a pixel, so out == full is allowed.
#include <math.h>

#include "common.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------------------------ resample
struct Taps { int lo, hi; double centre, support; };

__device__ __forceinline__ Taps taps_of(int o, int in, int out) {
  Taps t;
  const double scale = (double)in / (double)out;
  t.support = scale > 1.0 ? scale : 1.0;
  t.centre = ((double)o + 0.5) * scale;
  const int lo = (int)(t.centre - t.support + 0.5), hi = (int)(t.centre + t.support + 0.5);
  t.lo = lo > 0 ? lo : 0;
  t.hi = hi < in ? hi : in;
  return t;
}
__device__ __forceinline__ double tap_weight(const Taps& t, int k) {
  const double v = 1.0 - fabs((((double)k + 0.5) - t.centre) / t.support);
  return v > 0.0 ? v : 0.0;
}
__device__ __forceinline__ double tap_total(const Taps& t) {
  double total = 0.0;
  for (int k = t.lo; k < t.hi; ++k) total += tap_weight(t, k);
  return total;
}

// tmp[Y][o][c] = sum_k weight(k) img[Y][k][c]
__global__ __launch_bounds__(kThreads) void resample_rows_kernel(const uint8_t* __restrict__ img, double* __restrict__ tmp, int H, int W,
                                                                 int w) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)H * w) return;
  const int Y = (int)(i / w), o = (int)(i % w);
  const Taps t = taps_of(o, W, w);
  const double total = tap_total(t);
  const uint8_t* row = img + (int64_t)Y * W * 3;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int k = t.lo; k < t.hi; ++k) {
    const double wk = tap_weight(t, k) / total;
    a0 += wk * (double)row[3 * k];
    a1 += wk * (double)row[3 * k + 1];
    a2 += wk * (double)row[3 * k + 2];
  }
  double* d = tmp + i * 3;
  d[0] = a0; d[1] = a1; d[2] = a2;
}

// out[c][o][x] = (float) sum_k weight(k) tmp[k][x][c]
__global__ __launch_bounds__(kThreads) void resample_cols_kernel(const double* __restrict__ tmp, float* __restrict__ out, int H, int h,
                                                                 int w) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= h * w) return;
  const int o = i / w, x = i % w;
  const Taps t = taps_of(o, H, h);
  const double total = tap_total(t);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int k = t.lo; k < t.hi; ++k) {
    const double wk = tap_weight(t, k) / total;
    const double* s = tmp + ((int64_t)k * w + x) * 3;
    a0 += wk * s[0];
    a1 += wk * s[1];
    a2 += wk * s[2];
  }
  const int64_t hw = (int64_t)h * w;
  out[i] = (float)a0;
  out[hw + i] = (float)a1;
  out[2 * hw + i] = (float)a2;
}

// ------------------------------------------------------------------------------------------------------------------ fit
// the 21 planes whose window means the solve needs: I_j (0-2), p_c (3-5), I_i I_j for i <= j (6-11: 00 01 02 11 12 22), I_j p_c (12 + 3 j + c)
constexpr int kMoments = 21;
constexpr int kCoefs = 12;

struct FitParams { int N, h, w, r; double eps; };

__device__ __forceinline__ bool fit_pixel(const FitParams& P, int& x, int& y) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= P.h * P.w) return false;
  y = i / P.w;
  x = i % P.w;
  return true;
}

// sums along x of the 21 products, in index order
__global__ __launch_bounds__(kThreads) void fit_moments_x_kernel(const FitParams P, const float* __restrict__ I, const float* __restrict__ p,
                                                                 double* __restrict__ mx) {
  int x, y;
  if (!fit_pixel(P, x, y)) return;
  const int64_t hw = (int64_t)P.h * P.w, n = blockIdx.z;
  const float* Ir = I + n * 3 * hw + (int64_t)y * P.w;
  const float* pr = p + n * 3 * hw + (int64_t)y * P.w;
  const int lo = x - P.r > 0 ? x - P.r : 0, hi = x + P.r < P.w - 1 ? x + P.r : P.w - 1;
  double s[kMoments];
#pragma unroll
  for (int k = 0; k < kMoments; ++k) s[k] = 0.0;
  for (int k = lo; k <= hi; ++k) {
    const double i0 = Ir[k], i1 = Ir[hw + k], i2 = Ir[2 * hw + k];
    const double p0 = pr[k], p1 = pr[hw + k], p2 = pr[2 * hw + k];
    s[0] += i0; s[1] += i1; s[2] += i2;
    s[3] += p0; s[4] += p1; s[5] += p2;
    s[6] += i0 * i0; s[7] += i0 * i1; s[8] += i0 * i2; s[9] += i1 * i1; s[10] += i1 * i2; s[11] += i2 * i2;
    s[12] += i0 * p0; s[13] += i0 * p1; s[14] += i0 * p2;
    s[15] += i1 * p0; s[16] += i1 * p1; s[17] += i1 * p2;
    s[18] += i2 * p0; s[19] += i2 * p1; s[20] += i2 * p2;
  }
  double* o = mx + n * kMoments * hw + (int64_t)y * P.w + x;
#pragma unroll
  for (int k = 0; k < kMoments; ++k) o[k * hw] = s[k];
}

// sums along y, the means, the 3x3 solve: a[c][0..2], b[c] before the second window mean, planes a00 a01 a02 a10 .. a22 b0 b1 b2
__global__ __launch_bounds__(kThreads) void fit_solve_kernel(const FitParams P, const double* __restrict__ mx, double* __restrict__ ab) {
  int x, y;
  if (!fit_pixel(P, x, y)) return;
  const int64_t hw = (int64_t)P.h * P.w, n = blockIdx.z;
  const int ylo = y - P.r > 0 ? y - P.r : 0, yhi = y + P.r < P.h - 1 ? y + P.r : P.h - 1;
  const int xlo = x - P.r > 0 ? x - P.r : 0, xhi = x + P.r < P.w - 1 ? x + P.r : P.w - 1;
  const double count = (double)((xhi - xlo + 1) * (yhi - ylo + 1));
  const double* src = mx + n * kMoments * hw + x;
  double m[kMoments];
#pragma unroll
  for (int k = 0; k < kMoments; ++k) {
    double s = 0.0;
    for (int j = ylo; j <= yhi; ++j) s += src[k * hw + (int64_t)j * P.w];
    m[k] = s / count;
  }
  // Sigma = mean(I I^T) - mean(I) mean(I)^T + eps U, symmetric positive definite: Cholesky, L L^T
  const double s00 = m[6] - m[0] * m[0] + P.eps, s01 = m[7] - m[0] * m[1], s02 = m[8] - m[0] * m[2];
  const double s11 = m[9] - m[1] * m[1] + P.eps, s12 = m[10] - m[1] * m[2], s22 = m[11] - m[2] * m[2] + P.eps;
  const double l00 = sqrt(s00), l10 = s01 / l00, l20 = s02 / l00;
  const double l11 = sqrt(s11 - l10 * l10), l21 = (s12 - l20 * l10) / l11;
  const double l22 = sqrt(s22 - l20 * l20 - l21 * l21);
  double* o = ab + n * kCoefs * hw + (int64_t)y * P.w + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double c0 = m[12 + c] - m[0] * m[3 + c], c1 = m[15 + c] - m[1] * m[3 + c], c2 = m[18 + c] - m[2] * m[3 + c];
    const double z0 = c0 / l00, z1 = (c1 - l10 * z0) / l11, z2 = (c2 - l20 * z0 - l21 * z1) / l22;
    const double a2 = z2 / l22, a1 = (z1 - l21 * a2) / l11, a0 = (z0 - l10 * a1 - l20 * a2) / l00;
    o[(3 * c) * hw] = a0;
    o[(3 * c + 1) * hw] = a1;
    o[(3 * c + 2) * hw] = a2;
    o[(9 + c) * hw] = m[3 + c] - (a0 * m[0] + a1 * m[1] + a2 * m[2]);
  }
}

// the second window mean: sums along x of the twelve planes ...
__global__ __launch_bounds__(kThreads) void fit_coef_x_kernel(const FitParams P, const double* __restrict__ ab, double* __restrict__ cx) {
  int x, y;
  if (!fit_pixel(P, x, y)) return;
  const int64_t hw = (int64_t)P.h * P.w, n = blockIdx.z;
  const int lo = x - P.r > 0 ? x - P.r : 0, hi = x + P.r < P.w - 1 ? x + P.r : P.w - 1;
  const double* src = ab + n * kCoefs * hw + (int64_t)y * P.w;
  double* o = cx + n * kCoefs * hw + (int64_t)y * P.w + x;
#pragma unroll
  for (int k = 0; k < kCoefs; ++k) {
    double s = 0.0;
    for (int j = lo; j <= hi; ++j) s += src[k * hw + j];
    o[k * hw] = s;
  }
}

// ... then along y, the division by the pixel count and the one rounding
__global__ __launch_bounds__(kThreads) void fit_coef_y_kernel(const FitParams P, const double* __restrict__ cx, float* __restrict__ coef) {
  int x, y;
  if (!fit_pixel(P, x, y)) return;
  const int64_t hw = (int64_t)P.h * P.w, n = blockIdx.z;
  const int ylo = y - P.r > 0 ? y - P.r : 0, yhi = y + P.r < P.h - 1 ? y + P.r : P.h - 1;
  const int xlo = x - P.r > 0 ? x - P.r : 0, xhi = x + P.r < P.w - 1 ? x + P.r : P.w - 1;
  const double count = (double)((xhi - xlo + 1) * (yhi - ylo + 1));
  const double* src = cx + n * kCoefs * hw + x;
  float* o = coef + n * kCoefs * hw + (int64_t)y * P.w + x;
#pragma unroll
  for (int k = 0; k < kCoefs; ++k) {
    double s = 0.0;
    for (int j = ylo; j <= yhi; ++j) s += src[k * hw + (int64_t)j * P.w];
    o[k * hw] = (float)(s / count);
  }
}

struct FitWs { double* mx; double* ab; };      // mx: [N][21][h][w], and again for the x sums of the coefficients; ab: [N][12][h][w]

int64_t fit_layout(void* base, int N, int64_t hw, FitWs* ws) {
  Carver c(base);
  ws->mx = c.take<double>((int64_t)N * kMoments * hw);
  ws->ab = c.take<double>((int64_t)N * kCoefs * hw);
  return c.total();
}

// ------------------------------------------------------------------------------------------------------------------ apply
constexpr int kLanePix = 4;                        // consecutive pixels of a row per lane
constexpr int kStripPix = kThreads * kLanePix;     // pixels of a row per workgroup
constexpr int kTileRows = 8;
constexpr int kStageCols = 384;                    // coefficient columns a workgroup may stage: 2 rows x 12 planes x 384 floats = 36 KiB

struct ApplyParams {
  int h, w, H, W;
  int clamp;
  int vec;              // rows can be moved as aligned words (uint8: full and out agree mod 4; fp32: 16-byte rows)
  int stage;            // columns of a staged segment (the launch's dynamic LDS is 24 of them): what this geometry needs, <= kStageCols
  float inv2W, inv2H;
};

// where an output index sits among the coefficient pixels: s = clamp((X + 0.5) in / out - 0.5, 0, in - 1) = n / (2 out) in integers
__device__ __forceinline__ void source_of(int X, int in, int out2, float inv_out2, int& i0, float& f) {
  int n = (2 * X + 1) * in - (out2 >> 1);
  const int top = (in - 1) * out2;
  n = n < 0 ? 0 : (n > top ? top : n);
  int q = (int)((float)n * inv_out2);           // within one of n / out2: the quotient is at most 4095
  int r = n - q * out2;
  if (r < 0) { --q; r += out2; } else if (r >= out2) { ++q; r -= out2; }
  i0 = q;
  f = (float)r * inv_out2;
}

// the coefficient planes read in place: rows y0, y1 of every plane, columns clamped
struct PlaneSource {
  const float* row0; const float* row1;
  int64_t plane;
  int w;
  __device__ __forceinline__ void taps(int p, int x0, float& a0, float& a1, float& b0, float& b1) const {
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1;
    const float* r0 = row0 + p * plane;
    const float* r1 = row1 + p * plane;
    a0 = r0[x0]; a1 = r0[x1]; b0 = r1[x0]; b1 = r1[x1];
  }
};
// the staged copy: [column][row][plane], column j holding coefficient column min(first + j, w - 1).  The 48 values of a pixel -- both
// rows of its column and of the next -- are 48 consecutive floats on a 32-byte boundary: twelve 16-byte LDS reads at constant offsets
struct StagedSource {
  const float* lds;
  int first;
  __device__ __forceinline__ void taps(int p, int x0, float& a0, float& a1, float& b0, float& b1) const {
    const float* s = (const float*)__builtin_assume_aligned(lds + (x0 - first) * (2 * kCoefs), 16);
    a0 = s[p]; b0 = s[kCoefs + p]; a1 = s[2 * kCoefs + p]; b1 = s[3 * kCoefs + p];
  }
};

template <class Source>
__device__ __forceinline__ void transfer_pixel(const Source& src, const ApplyParams& P, int X, float fy, float F0, float F1, float F2,
                                               float& q0, float& q1, float& q2) {
  int x0;
  float fx;
  source_of(X, P.w, 2 * P.W, P.inv2W, x0, fx);
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  float v[kCoefs];
#pragma unroll
  for (int p = 0; p < kCoefs; ++p) {
    float a0, a1, b0, b1;
    src.taps(p, x0, a0, a1, b0, b1);
    const float top = fmaf(fx, a1, gx * a0), bot = fmaf(fx, b1, gx * b0);
    v[p] = fmaf(fy, bot, gy * top);
  }
  q0 = fmaf(v[2], F2, fmaf(v[1], F1, v[0] * F0)) + v[9];
  q1 = fmaf(v[5], F2, fmaf(v[4], F1, v[3] * F0)) + v[10];
  q2 = fmaf(v[8], F2, fmaf(v[7], F1, v[6] * F0)) + v[11];
  if (P.clamp) {
    q0 = fminf(fmaxf(q0, 0.0f), 1.0f);
    q1 = fminf(fmaxf(q1, 0.0f), 1.0f);
    q2 = fminf(fmaxf(q2, 0.0f), 1.0f);
  }
}

__device__ __forceinline__ unsigned to_byte(float q01) { return (unsigned)rintf(255.0f * q01); }      // q01 in [0, 1]: P.clamp is 1

// one row of the uint8 form: this lane's group of four pixels behind the row's head, and one head pixel for the first lanes.
// unit[b] = (float)b / 255.0f, the 256 quotients divided once per workgroup
template <class Source>
__device__ __forceinline__ void row_u8(const Source& src, const ApplyParams& P, int Y, float fy, const uint8_t* full, uint8_t* out,
                                       const float* unit) {
  const int64_t at = (int64_t)Y * P.W * 3;
  const uint8_t* in_row = full + at;
  uint8_t* out_row = out + at;
  const int head = P.vec ? (int)((uintptr_t)in_row & 3) : 0;      // 3 * head = -address (mod 4): the first aligned pixel
  const int group = blockIdx.x * kThreads + threadIdx.x;
  const int X0 = head + group * kLanePix;
  if (P.vec && X0 + kLanePix <= P.W) {
    const uint32_t* in32 = (const uint32_t*)(in_row + 3 * X0);
    const uint32_t w0 = in32[0], w1 = in32[1], w2 = in32[2];
    unsigned b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[k] = (w0 >> (8 * k)) & 255u;
      b[4 + k] = (w1 >> (8 * k)) & 255u;
      b[8 + k] = (w2 >> (8 * k)) & 255u;
    }
#pragma unroll
    for (int k = 0; k < kLanePix; ++k) {
      float q0, q1, q2;
      transfer_pixel(src, P, X0 + k, fy, unit[b[3 * k]], unit[b[3 * k + 1]], unit[b[3 * k + 2]], q0, q1, q2);
      b[3 * k] = to_byte(q0); b[3 * k + 1] = to_byte(q1); b[3 * k + 2] = to_byte(q2);
    }
    uint32_t* out32 = (uint32_t*)(out_row + 3 * X0);
    out32[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    out32[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    out32[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
  } else {
    for (int X = X0; X < X0 + kLanePix && X < P.W; ++X) {
      const unsigned r = in_row[3 * X], g = in_row[3 * X + 1], bl = in_row[3 * X + 2];
      float q0, q1, q2;
      transfer_pixel(src, P, X, fy, unit[r], unit[g], unit[bl], q0, q1, q2);
      out_row[3 * X] = (uint8_t)to_byte(q0); out_row[3 * X + 1] = (uint8_t)to_byte(q1); out_row[3 * X + 2] = (uint8_t)to_byte(q2);
    }
  }
  if (group < head && group < P.W) {
    const int X = group;
    const unsigned r = in_row[3 * X], g = in_row[3 * X + 1], bl = in_row[3 * X + 2];
    float q0, q1, q2;
    transfer_pixel(src, P, X, fy, unit[r], unit[g], unit[bl], q0, q1, q2);
    out_row[3 * X] = (uint8_t)to_byte(q0); out_row[3 * X + 1] = (uint8_t)to_byte(q1); out_row[3 * X + 2] = (uint8_t)to_byte(q2);
  }
}

// one row of the fp32 form: full and out are this image's three planes
template <class Source>
__device__ __forceinline__ void row_f32(const Source& src, const ApplyParams& P, int Y, float fy, const float* full, float* out) {
  const int64_t HW = (int64_t)P.H * P.W, at = (int64_t)Y * P.W;
  const int X0 = (blockIdx.x * kThreads + threadIdx.x) * kLanePix;
  if (X0 >= P.W) return;
  if (P.vec) {                                                     // W % 4 == 0: the group is whole
    const float4 f0 = *(const float4*)(full + at + X0), f1 = *(const float4*)(full + HW + at + X0);
    const float4 f2 = *(const float4*)(full + 2 * HW + at + X0);
    float4 q0, q1, q2;
    transfer_pixel(src, P, X0, fy, f0.x, f1.x, f2.x, q0.x, q1.x, q2.x);
    transfer_pixel(src, P, X0 + 1, fy, f0.y, f1.y, f2.y, q0.y, q1.y, q2.y);
    transfer_pixel(src, P, X0 + 2, fy, f0.z, f1.z, f2.z, q0.z, q1.z, q2.z);
    transfer_pixel(src, P, X0 + 3, fy, f0.w, f1.w, f2.w, q0.w, q1.w, q2.w);
    *(float4*)(out + at + X0) = q0;
    *(float4*)(out + HW + at + X0) = q1;
    *(float4*)(out + 2 * HW + at + X0) = q2;
  } else {
    for (int X = X0; X < X0 + kLanePix && X < P.W; ++X) {
      float q0, q1, q2;
      transfer_pixel(src, P, X, fy, full[at + X], full[HW + at + X], full[2 * HW + at + X], q0, q1, q2);
      out[at + X] = q0; out[HW + at + X] = q1; out[2 * HW + at + X] = q2;
    }
  }
}

template <bool kBytes, class Source, class T>
__device__ __forceinline__ void transfer_row(const Source& src, const ApplyParams& P, int Y, float fy, const T* full, T* out,
                                             const float* unit) {
  if constexpr (kBytes) row_u8(src, P, Y, fy, full, out, unit);
  else row_f32(src, P, Y, fy, full, out);
}

// grid (strips, row tiles, N).  coef: [N][12][h][w]; full, out: uint8 [H][W][3] (N = 1) or float [N][3][H][W]
template <bool kBytes, bool kStaged, class T>
__global__ __launch_bounds__(kThreads) void guided_apply_kernel(const ApplyParams P, const float* __restrict__ coef, const T* full, T* out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];      // staged: [P.stage][2][12]
  __shared__ float unit[kBytes ? 256 : 1];
  static_assert(kThreads == 256, "one quotient per thread");
  const int64_t hw = (int64_t)P.h * P.w, n = blockIdx.z;
  const float* cf = coef + n * kCoefs * hw;
  const int64_t image = (int64_t)P.H * P.W * 3;
  full += n * image;
  out += n * image;
  const int Yend = (blockIdx.y + 1) * kTileRows < P.H ? (blockIdx.y + 1) * kTileRows : P.H;
  // the coefficient columns of the strip: a uint8 row may start up to three pixels in, and its head pixels belong to strip 0
  int first = 0, cols = 0;
  if constexpr (kStaged) {
    const int Xlo = blockIdx.x * kStripPix;
    const int Xhi = Xlo + kStripPix + 2 < P.W - 1 ? Xlo + kStripPix + 2 : P.W - 1;
    if (Xlo >= P.W) return;
    int last;
    float unused;
    source_of(Xlo, P.w, 2 * P.W, P.inv2W, first, unused);
    source_of(Xhi, P.w, 2 * P.W, P.inv2W, last, unused);
    cols = last + 2 - first;
    cols = cols < P.stage ? cols : P.stage;            // the launcher sized the segment so that they fit
  }
  if constexpr (kBytes) {
    unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
  }
  int staged_row = -1;
  for (int Y = blockIdx.y * kTileRows; Y < Yend; ++Y) {
    int y0;
    float fy;
    source_of(Y, P.h, 2 * P.H, P.inv2H, y0, fy);
    const int y1 = y0 + 1 < P.h ? y0 + 1 : P.h - 1;
    if constexpr (kStaged) {
      if (y0 != staged_row) {                            // uniform over the workgroup
        __syncthreads();                                 // the previous rows' reads are done
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int pr = wave; pr < kCoefs * 2; pr += kThreads / 64) {
          const float* g = cf + (pr >> 1) * hw + (int64_t)((pr & 1) ? y1 : y0) * P.w;
          for (int j = lane; j < cols; j += 64) {
            const int x = first + j < P.w ? first + j : P.w - 1;
            lds[j * (2 * kCoefs) + (pr & 1) * kCoefs + (pr >> 1)] = g[x];
          }
        }
        __syncthreads();
        staged_row = y0;
      }
      const StagedSource src{lds, first};
      transfer_row<kBytes>(src, P, Y, fy, full, out, unit);
    } else {
      const PlaneSource src{cf + (int64_t)y0 * P.w, cf + (int64_t)y1 * P.w, hw, P.w};
      transfer_row<kBytes>(src, P, Y, fy, full, out, unit);
    }
  }
}

int check_apply(const char* who, int h, int w, int H, int W) {
  HDIFF_CHECK_ARG(h >= 1 && h <= 4096 && w >= 1 && w <= 4096, "%s: h = %d, w = %d; the coefficient planes are between 1 and 4096 a side",
                  who, h, w);
  HDIFF_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "%s: H = %d, W = %d; the image is between 1 and 16384 a side", who, H, W);
  HDIFF_CHECK_ARG((int64_t)H * W <= (1ll << 30), "%s: H * W = %lld is too large; at most 2^30 pixels", who, (long long)H * W);
  return HDIFF_OK;
}

template <bool kBytes, class T>
void launch_apply(const float* coef, int h, int w, const T* full, T* out, int N, int H, int W, int clamp, int vec, hipStream_t s) {
  ApplyParams P;
  P.h = h; P.w = w; P.H = H; P.W = W;
  P.clamp = clamp;
  P.vec = vec;
  P.inv2W = 1.0f / (float)(2 * W);
  P.inv2H = 1.0f / (float)(2 * H);
  // groups of four per row: a uint8 row's head moves the groups by up to three pixels, so one more may be begun
  const int groups = (W + kLanePix - 1) / kLanePix + (kBytes ? 1 : 0);
  const dim3 grid(cdiv(groups, kThreads), cdiv(H, kTileRows), N);
  // a strip reaches over at most (kStripPix + 2) w / W coefficient pixels; with the tap to the right and both ends, three more columns
  const int64_t need = ((int64_t)(kStripPix + 2) * w) / W + 3;
  P.stage = need <= kStageCols ? (int)need : 0;
  const size_t lds = (size_t)kCoefs * 2 * P.stage * sizeof(float);
  if (P.stage) hipLaunchKernelGGL((guided_apply_kernel<kBytes, true, T>), grid, dim3(kThreads), lds, s, P, coef, full, out);
  else hipLaunchKernelGGL((guided_apply_kernel<kBytes, false, T>), grid, dim3(kThreads), 0, s, P, coef, full, out);
}

}  // namespace

extern "C" {

int hdiff_resample_workspace(int H, int W, int h, int w, int64_t* bytes) {
  HDIFF_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "resample_workspace: H = %d, W = %d; the image is between 1 and 16384 a side",
                  H, W);
  HDIFF_CHECK_ARG(h >= 1 && h <= 4096 && w >= 1 && w <= 4096, "resample_workspace: h = %d, w = %d; the output is between 1 and 4096 a side",
                  h, w);
  HDIFF_CHECK_ARG(bytes, "resample_workspace: null pointer");
  *bytes = align256((int64_t)H * w * 3 * (int64_t)sizeof(double));
  return HDIFF_OK;
}

int hdiff_resample_u8(const uint8_t* img, int H, int W, float* out, int h, int w, void* scratch, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "resample_u8: H = %d, W = %d; the image is between 1 and 16384 a side", H, W);
  HDIFF_CHECK_ARG(h >= 1 && h <= 4096 && w >= 1 && w <= 4096, "resample_u8: h = %d, w = %d; the output is between 1 and 4096 a side", h, w);
  HDIFF_CHECK_ARG(img && out && scratch, "resample_u8: null pointer");
  (void)hipGetLastError();
  hipStream_t s = (hipStream_t)stream;
  double* tmp = (double*)scratch;
  const int64_t rows = (int64_t)H * w;
  hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, img, tmp, H, W, w);
  hipLaunchKernelGGL(resample_cols_kernel, dim3(cdiv(h * w, kThreads)), dim3(kThreads), 0, s, tmp, out, H, h, w);
  HDIFF_CHECK_LAUNCH("resample kernels");
  return HDIFF_OK;
}

static int check_fit(const char* who, int N, int h, int w) {
  HDIFF_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d; between 1 and 65535 images", who, N);
  HDIFF_CHECK_ARG(h >= 1 && h <= 4096 && w >= 1 && w <= 4096, "%s: h = %d, w = %d; the images are between 1 and 4096 a side", who, h, w);
  return HDIFF_OK;
}

int hdiff_guided_workspace(int N, int h, int w, int64_t* bytes) {
  const int rc = check_fit("guided_workspace", N, h, w);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "guided_workspace: null pointer");
  FitWs ws;
  *bytes = fit_layout(nullptr, N, (int64_t)h * w, &ws);
  return HDIFF_OK;
}

int hdiff_guided_fit(const float* I, const float* p, int N, int h, int w, int r, double eps, float* coef, void* scratch,
                     hdiff_stream_t stream) {
  const int rc = check_fit("guided_fit", N, h, w);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(r >= 1 && r <= 128, "guided_fit: r = %d; the radius is between 1 and 128", r);
  HDIFF_CHECK_ARG(eps > 0.0 && eps <= 1.7976931348623157e308, "guided_fit: eps = %g; it must be finite and positive", eps);
  HDIFF_CHECK_ARG(I && p && coef && scratch, "guided_fit: null pointer");
  (void)hipGetLastError();
  FitParams P;
  P.N = N; P.h = h; P.w = w; P.r = r; P.eps = eps;
  FitWs ws;
  fit_layout(scratch, N, (int64_t)h * w, &ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(h * w, kThreads), 1, N), blk(kThreads);
  hipLaunchKernelGGL(fit_moments_x_kernel, grid, blk, 0, s, P, I, p, ws.mx);
  hipLaunchKernelGGL(fit_solve_kernel, grid, blk, 0, s, P, ws.mx, ws.ab);
  hipLaunchKernelGGL(fit_coef_x_kernel, grid, blk, 0, s, P, ws.ab, ws.mx);      // the moments are spent: their region takes the x sums
  hipLaunchKernelGGL(fit_coef_y_kernel, grid, blk, 0, s, P, ws.mx, coef);
  HDIFF_CHECK_LAUNCH("guided_fit kernels");
  return HDIFF_OK;
}

int hdiff_guided_apply_f32(const float* coef, int h, int w, const float* full, float* out, int N, int H, int W, int clamp,
                           hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(N >= 1 && N <= 65535, "guided_apply_f32: N = %d; between 1 and 65535 images", N);
  const int rc = check_apply("guided_apply_f32", h, w, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(coef && full && out, "guided_apply_f32: null pointer");
  (void)hipGetLastError();
  const int vec = W % 4 == 0 && (((uintptr_t)full | (uintptr_t)out) & 15) == 0;
  launch_apply<false, float>(coef, h, w, full, out, N, H, W, clamp != 0, vec, (hipStream_t)stream);
  HDIFF_CHECK_LAUNCH("guided_apply_f32 kernel");
  return HDIFF_OK;
}

int hdiff_guided_apply_u8(const float* coef, int h, int w, const uint8_t* full, uint8_t* out, int H, int W, hdiff_stream_t stream) {
  const int rc = check_apply("guided_apply_u8", h, w, H, W);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(coef && full && out, "guided_apply_u8: null pointer");
  (void)hipGetLastError();
  const int vec = (((uintptr_t)full ^ (uintptr_t)out) & 3) == 0;
  launch_apply<true, uint8_t>(coef, h, w, full, out, 1, H, W, 1, vec, (hipStream_t)stream);
  HDIFF_CHECK_LAUNCH("guided_apply_u8 kernel");
  return HDIFF_OK;
}

}  // extern "C"
