// MS-SSIM + L1 loss (the mix of Zhao et al., "Loss Functions for Image Restoration with Neural Networks", as the reference's
// Loss/loss.py:269-283 uses it through kornia's MS_SSIMLoss) and its gradient with respect to the prediction.  fp32 stencils.
//
// For a pair (colour channel c, scale sigma) the loss needs five zero-padded Gaussian moments of the two planes x_c, y_c:
//   G*x, G*y, G*(x^2), G*(y^2), G*(xy); the L1 part needs G_{sigma_max} * |x_c - y_c| per channel.
// Forward, three launches:
//   1. msssim_moments_kernel   grid (32x32 tiles, jobs, B).  One job = one distinct pair (five products) or one channel of the L1
//                              part (one product).  The 64x64 input tiles of x_c and y_c are staged in LDS once; every product is
//                              filtered separably (row pass into LDS, column pass into registers) and written to the moment
//                              buffer, which the backward reads again.
//   2. msssim_pixel_kernel     per pixel: l and cs of every pair, their products with the table's multiplicities, the pixel loss;
//                              float64 block sums in a fixed order into one partial per block.
//   3. msssim_finalize_kernel  one block adds the partials in index order (no float atomics: bitwise repeatable).
// Backward, two launches:
//   1. msssim_pixel_kernel<true>   the coefficient maps a, b, c of every pair (partials of the pixel loss with respect to G*x,
//                              G*(x^2), G*(xy), times the upstream gradient) from the saved moments.
//   2. msssim_adjoint_kernel   grid (tiles, 3, B): dx_c = sum over the pairs of channel c of [G*a + 2 x_c (G*b) + y_c (G*c)] (the
//                              window is symmetric: the adjoint is the same zero-padded filter) plus the L1 part, whose filtered
//                              upstream map is the upstream scalar times the separable border mass of the window.
//
// LDS layout (bank rule: ds_read_b32 / ds_write_b32 conflict within a 32-lane half, bank = word address mod 32):
//   input tiles  [64][65]  the row pass gives one tile ROW to each lane (8 adjacent outputs per thread slide along it, so each
//                          staged value is read once per 8 outputs); with the odd pitch lane r reads bank (r + col) mod 32
//   row-filtered [64][33]  written by lane = row (odd pitch again), read by the column pass with lane = column (consecutive
//                          banks); 4 vertically adjacent outputs per thread slide down the column
// 2 x 16.25 KiB + 8.25 KiB = 40.8 KiB per workgroup: three workgroups per CU.
//
// Taps: the 1-D weights come from the host (float64, normalised, rounded to fp32).  A scale is filtered with radius 4, 8 or 16,
// the smallest that holds every weight above 1e-12: at the default sigmas, sigma 0.5 skips the taps |k| >= 5 (weights below
// 2e-22) and sigma 1 the taps |k| >= 9 (below 2e-18); sigma 2, 4 and 8 use all 33.
//
// Contraction: the file is compiled WITHOUT -ffp-contract=off, unlike the other loss kernels -- there is no torch program whose
// rounding the filters must repeat (the gate is the float64 definition), and fma only removes roundings from the sums.  The
// per-pixel formulas alone switch contraction off, so that identical images give l = cs = 1 and a loss of exactly 0: with fma,
// 2 mu_x mu_y + C1 and mu_x^2 + mu_y^2 + C1 would round differently for mu_x == mu_y.
#include "common.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;        // output tile edge
constexpr int kHalo = 16;        // largest radius
constexpr int kIn = 64;          // staged tile edge
constexpr int kPitchIn = 65;
constexpr int kPitchRow = 33;
constexpr int kMaxPairs = HDIFF_MSSSIM_MAX_PAIRS;
constexpr int kMaxScales = HDIFF_MSSSIM_MAX_SCALES;
constexpr int kMaxWin = HDIFF_MSSSIM_MAX_WINDOW;
constexpr int kMaxJobs = kMaxPairs + 3;
constexpr int kPixMaxBlocks = 1024;

enum { kA = 0, kB, kAA, kBB, kAB, kAbsD };

struct Params {
  int B, H, W, tiles_x;
  int nscales, npairs, l1_scale;
  int radius[kMaxScales];            // 4, 8 or 16
  float w[kMaxScales][kMaxWin];      // centre at [16]
  int chan[kMaxPairs], scale[kMaxPairs], cs_pow[kMaxPairs], l_pow[kMaxPairs];
  float C1, C2, alpha, comp, inv_range;
  double red_scale;                  // 1 / (B H W) for 'mean', 1 for 'sum'
};

template <int KIND>
__device__ __forceinline__ float prod(float a, float b) {
  if (KIND == kA) return a;
  if (KIND == kB) return b;
  if (KIND == kAA) return a * a;
  if (KIND == kBB) return b * b;
  if (KIND == kAB) return a * b;
  return fabsf(a - b);
}

// Rows and columns [16 - R, 48 + R) of the 64x64 tile whose element (16, 16) is the image pixel (ty0, tx0); 0 outside the image.
__device__ void stage_tile(float* s, const float* __restrict__ plane, int H, int W, int ty0, int tx0, int R) {
  const int lo = kHalo - R, hi = kHalo + kTile + R;
  for (int i = threadIdx.x; i < kIn * kIn; i += kThreads) {
    const int r = i >> 6, c = i & 63;
    if (r < lo || r >= hi || c < lo || c >= hi) continue;
    const int gy = ty0 - kHalo + r, gx = tx0 - kHalo + c;
    s[r * kPitchIn + c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? plane[(int64_t)gy * W + gx] : 0.0f;
  }
}

// Horizontal pass: thread = (tile row, 8 adjacent output columns); sw points at the centre weight.
template <int R, int KIND>
__device__ __forceinline__ void row_pass(const float* sA, const float* sB, float* sRow, const float* sw) {
  const int r = threadIdx.x & 63, c0 = (threadIdx.x >> 6) * 8;
  if (r < kHalo - R || r >= kHalo + kTile + R) return;
  float wv[2 * R + 1];
#pragma unroll
  for (int i = 0; i <= 2 * R; ++i) wv[i] = sw[i - R];
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int base = r * kPitchIn + c0 + kHalo - R;
#pragma unroll
  for (int k = 0; k < 2 * R + 8; ++k) {
    const float a = (KIND != kB) ? sA[base + k] : 0.f;
    const float b = (KIND != kA && KIND != kAA) ? sB[base + k] : 0.f;
    const float v = prod<KIND>(a, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int wi = k - j;
      if (wi >= 0 && wi <= 2 * R) acc[j] += wv[wi] * v;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sRow[r * kPitchRow + c0 + j] = acc[j];
}

// Vertical pass: thread = (column, 4 adjacent output rows): out[j] is output pixel (4 * (tid / 32) + j, tid % 32) of the tile.
template <int R>
__device__ __forceinline__ void col_pass(const float* sRow, const float* sw, float out[4]) {
  const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
  float wv[2 * R + 1];
#pragma unroll
  for (int i = 0; i <= 2 * R; ++i) wv[i] = sw[i - R];
  out[0] = out[1] = out[2] = out[3] = 0.f;
  const int base = (r0 + kHalo - R) * kPitchRow + c;
#pragma unroll
  for (int k = 0; k < 2 * R + 4; ++k) {
    const float v = sRow[base + k * kPitchRow];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int wi = k - j;
      if (wi >= 0 && wi <= 2 * R) out[j] += wv[wi] * v;
    }
  }
}

// One separable product of the staged tiles; ends with a barrier, so sRow may be overwritten at once.
template <int R, int KIND>
__device__ __forceinline__ void filter_product(const float* sA, const float* sB, float* sRow, const float* sw, float out[4]) {
  row_pass<R, KIND>(sA, sB, sRow, sw);
  __syncthreads();
  col_pass<R>(sRow, sw, out);
  __syncthreads();
}

__device__ __forceinline__ void store4(float* __restrict__ plane, const float v[4], int H, int W, int ty0, int tx0) {
  const int gx = tx0 + (threadIdx.x & 31), gy0 = ty0 + (threadIdx.x >> 5) * 4;
  if (gx >= W) return;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (gy0 + j < H) plane[(int64_t)(gy0 + j) * W + gx] = v[j];
}

template <int R>
__device__ void moments_job(const float* sA, const float* sB, float* sRow, const float* sw, float* __restrict__ dst, int64_t HW,
                            int H, int W, int ty0, int tx0, bool l1) {
  float o[4];
  if (l1) {
    filter_product<R, kAbsD>(sA, sB, sRow, sw, o);
    store4(dst, o, H, W, ty0, tx0);
    return;
  }
  filter_product<R, kA>(sA, sB, sRow, sw, o);
  store4(dst, o, H, W, ty0, tx0);
  filter_product<R, kB>(sA, sB, sRow, sw, o);
  store4(dst + HW, o, H, W, ty0, tx0);
  filter_product<R, kAA>(sA, sB, sRow, sw, o);
  store4(dst + 2 * HW, o, H, W, ty0, tx0);
  filter_product<R, kBB>(sA, sB, sRow, sw, o);
  store4(dst + 3 * HW, o, H, W, ty0, tx0);
  filter_product<R, kAB>(sA, sB, sRow, sw, o);
  store4(dst + 4 * HW, o, H, W, ty0, tx0);
}

// mom: [B][npairs][5][H][W]; l1f: [B][3][H][W].  Jobs 0 .. npairs-1 are the pairs, npairs .. npairs+2 the L1 channels.
__global__ __launch_bounds__(kThreads) void msssim_moments_kernel(const Params P, const float* __restrict__ x,
                                                                   const float* __restrict__ y, float* __restrict__ mom,
                                                                   float* __restrict__ l1f) {
  __shared__ float sA[kIn * kPitchIn];
  __shared__ float sB[kIn * kPitchIn];
  __shared__ float sRow[kIn * kPitchRow];
  __shared__ float sW[kMaxWin];
  const int job = blockIdx.y, b = blockIdx.z;
  const bool l1 = job >= P.npairs;
  const int c = l1 ? job - P.npairs : P.chan[job];
  const int s = l1 ? P.l1_scale : P.scale[job];
  const int R = P.radius[s];
  const int ty0 = (blockIdx.x / P.tiles_x) * kTile, tx0 = (blockIdx.x % P.tiles_x) * kTile;
  const int64_t HW = (int64_t)P.H * P.W;
  if (threadIdx.x < kMaxWin) sW[threadIdx.x] = P.w[s][threadIdx.x];
  stage_tile(sA, x + ((int64_t)b * 3 + c) * HW, P.H, P.W, ty0, tx0, R);
  stage_tile(sB, y + ((int64_t)b * 3 + c) * HW, P.H, P.W, ty0, tx0, R);
  __syncthreads();
  float* dst = l1 ? l1f + ((int64_t)b * 3 + c) * HW : mom + ((int64_t)b * P.npairs + job) * 5 * HW;
  const float* sw = sW + kHalo;
  if (R == 4) moments_job<4>(sA, sB, sRow, sw, dst, HW, P.H, P.W, ty0, tx0, l1);
  else if (R == 8) moments_job<8>(sA, sB, sRow, sw, dst, HW, P.H, P.W, ty0, tx0, l1);
  else moments_job<16>(sA, sB, sRow, sw, dst, HW, P.H, P.W, ty0, tx0, l1);
}

__device__ __forceinline__ float powi(float v, int n) {
  float r = 1.0f;
  for (int i = 0; i < n; ++i) r *= v;
  return r;
}

// Per pixel.  BWD = false: partial[block] = the block's sum of pixel losses.  BWD = true: coef [B][npairs][3][H][W] = (a, b, c).
// The products over the pairs never divide by a factor: the product of the OTHER pairs is formed from prefix and suffix products,
// so a cs that is zero or a product that underflows (the trainer's own y_0_pred does that) gives zeros, not NaN.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void msssim_pixel_kernel(const Params P, const float* __restrict__ mom,
                                                                 const float* __restrict__ l1f, const float* __restrict__ d_loss,
                                                                 double* __restrict__ partial, float* __restrict__ coef) {
#pragma clang fp contract(off)
  const int64_t HW = (int64_t)P.H * P.W, N = (int64_t)P.B * HW;
  const float up = BWD ? d_loss[0] * (float)P.red_scale : 0.f;
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < N; q += (int64_t)gridDim.x * kThreads) {
    const int64_t b = q / HW, pix = q - b * HW;
    float vcs[kMaxPairs], vl[kMaxPairs];                 // cs^m, l^m
    float dl_dmx[kMaxPairs], dcs_dmx[kMaxPairs], dcs_dxx[kMaxPairs], dcs_dxy[kMaxPairs];   // times d(v)/d(cs or l) below
#pragma unroll
    for (int p = 0; p < kMaxPairs; ++p) {
      vcs[p] = 1.f; vl[p] = 1.f;
      dl_dmx[p] = dcs_dmx[p] = dcs_dxx[p] = dcs_dxy[p] = 0.f;
      if (p < P.npairs) {
        const float* m = mom + ((b * P.npairs + p) * 5) * HW + pix;
        const float mx = m[0], my = m[HW], gxx = m[2 * HW], gyy = m[3 * HW], gxy = m[4 * HW];
        const float pxy = mx * my, pxx = mx * mx, pyy = my * my;
        const float sx = gxx - pxx, sy = gyy - pyy, sxy = gxy - pxy;
        const float lden = (pxx + pyy) + P.C1, cden = (sx + sy) + P.C2;
        const float l = (2.0f * pxy + P.C1) / lden, cs = (2.0f * sxy + P.C2) / cden;
        const int mc = P.cs_pow[p], ml = P.l_pow[p];
        vcs[p] = powi(cs, mc);
        vl[p] = powi(l, ml);
        if (BWD) {
          const float dvc = mc > 0 ? (float)mc * powi(cs, mc - 1) : 0.f;       // d cs^m / d cs
          const float dvl = ml > 0 ? (float)ml * powi(l, ml - 1) : 0.f;
          dl_dmx[p] = dvl * (2.0f * (my - l * mx) / lden);
          dcs_dmx[p] = dvc * (2.0f * (cs * mx - my) / cden);
          dcs_dxx[p] = dvc * (-cs / cden);
          dcs_dxy[p] = dvc * (2.0f / cden);
        }
      }
    }
    if (!BWD) {
      float pics = 1.f, lm = 1.f;
#pragma unroll
      for (int p = 0; p < kMaxPairs; ++p) { pics *= vcs[p]; lm *= vl[p]; }
      const float* lp = l1f + (b * 3) * HW + pix;
      const float l1 = ((lp[0] + lp[HW]) + lp[2 * HW]) / 3.0f;
      const float ms = 1.0f - lm * pics;
      acc += (double)(P.comp * (P.alpha * ms + (1.0f - P.alpha) * (l1 * P.inv_range)));
    } else {
      float pre_c[kMaxPairs], pre_l[kMaxPairs];
      float rc = 1.f, rl = 1.f;
#pragma unroll
      for (int p = 0; p < kMaxPairs; ++p) { pre_c[p] = rc; pre_l[p] = rl; rc *= vcs[p]; rl *= vl[p]; }
      const float pics = rc, lm = rl;
      const float k = -(up * P.comp * P.alpha);          // d loss / d (lM PIcs), times the upstream gradient
      float sc = 1.f, sl = 1.f;
#pragma unroll
      for (int p = kMaxPairs - 1; p >= 0; --p) {
        if (p < P.npairs) {
          const float gc = k * lm * (pre_c[p] * sc);     // d / d (cs_p^m)
          const float gl = k * pics * (pre_l[p] * sl);   // d / d (l_p^m)
          float* o = coef + ((b * P.npairs + p) * 3) * HW + pix;
          o[0] = gl * dl_dmx[p] + gc * dcs_dmx[p];
          o[HW] = gc * dcs_dxx[p];
          o[2 * HW] = gc * dcs_dxy[p];
        }
        sc *= vcs[p]; sl *= vl[p];
      }
    }
  }
  if (!BWD) {
    const double s = block_sum_to0<kThreads>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kThreads) void msssim_finalize_kernel(const double* __restrict__ partial, int nparts, double scale,
                                                                    float* __restrict__ loss) {
  const double s = sum_partials_to0<kThreads>(partial, nparts, 1);
  if (threadIdx.x == 0) loss[0] = (float)(s * scale);
}

template <int R>
__device__ void adjoint_pair(float* sA, float* sB, float* sRow, const float* sw, const float* __restrict__ cf, int64_t HW, int H,
                             int W, int ty0, int tx0, const float xv[4], const float yv[4], float dx[4]) {
  float ga[4], gb[4], gc[4];
  stage_tile(sA, cf, H, W, ty0, tx0, R);
  stage_tile(sB, cf + HW, H, W, ty0, tx0, R);
  __syncthreads();
  filter_product<R, kA>(sA, sB, sRow, sw, ga);
  filter_product<R, kB>(sA, sB, sRow, sw, gb);
  stage_tile(sA, cf + 2 * HW, H, W, ty0, tx0, R);       // the last reads of sA were before filter_product's barriers
  __syncthreads();
  filter_product<R, kA>(sA, sB, sRow, sw, gc);
#pragma unroll
  for (int j = 0; j < 4; ++j) dx[j] += ga[j] + 2.0f * xv[j] * gb[j] + yv[j] * gc[j];
}

__global__ __launch_bounds__(kThreads) void msssim_adjoint_kernel(const Params P, const float* __restrict__ x,
                                                                   const float* __restrict__ y, const float* __restrict__ coef,
                                                                   const float* __restrict__ d_loss, float* __restrict__ dxo) {
  __shared__ float sA[kIn * kPitchIn];
  __shared__ float sB[kIn * kPitchIn];
  __shared__ float sRow[kIn * kPitchRow];
  __shared__ float sW[kMaxWin];
  __shared__ float sMass[2][kTile];
  const int c = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / P.tiles_x) * kTile, tx0 = (blockIdx.x % P.tiles_x) * kTile;
  const int H = P.H, W = P.W;
  const int64_t HW = (int64_t)H * W;
  const float* xp = x + ((int64_t)b * 3 + c) * HW;
  const float* yp = y + ((int64_t)b * 3 + c) * HW;
  const int gx = tx0 + (threadIdx.x & 31), gy0 = ty0 + (threadIdx.x >> 5) * 4;
  float xv[4], yv[4], dx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = gx < W && gy0 + j < H;
    xv[j] = in ? xp[(int64_t)(gy0 + j) * W + gx] : 0.f;
    yv[j] = in ? yp[(int64_t)(gy0 + j) * W + gx] : 0.f;
  }
  for (int p = 0; p < P.npairs; ++p) {
    if (P.chan[p] != c) continue;                        // block-uniform
    const int s = P.scale[p], R = P.radius[s];
    __syncthreads();                                      // the previous pair's readers of sW are done
    if (threadIdx.x < kMaxWin) sW[threadIdx.x] = P.w[s][threadIdx.x];
    const float* cf = coef + ((int64_t)b * P.npairs + p) * 3 * HW;
    const float* sw = sW + kHalo;
    if (R == 4) adjoint_pair<4>(sA, sB, sRow, sw, cf, HW, H, W, ty0, tx0, xv, yv, dx);
    else if (R == 8) adjoint_pair<8>(sA, sB, sRow, sw, cf, HW, H, W, ty0, tx0, xv, yv, dx);
    else adjoint_pair<16>(sA, sB, sRow, sw, cf, HW, H, W, ty0, tx0, xv, yv, dx);
  }
  // L1 part: the filtered upstream map is uniform * (window mass inside the image along rows) * (the same along columns)
  if (threadIdx.x < 2 * kTile) {
    const int dim = threadIdx.x >> 5, i = threadIdx.x & 31;
    const int pos = (dim == 0 ? ty0 : tx0) + i, n = dim == 0 ? H : W;
    const int R = P.radius[P.l1_scale];
    float m = 0.f;
    for (int k = -R; k <= R; ++k)
      if (pos + k >= 0 && pos + k < n) m += P.w[P.l1_scale][kHalo + k];
    sMass[dim][i] = m;
  }
  __syncthreads();
  const float k1 = d_loss[0] * (float)P.red_scale * ((1.0f - P.alpha) * P.comp * P.inv_range / 3.0f);
  if (gx >= W) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (gy0 + j >= H) continue;
    const float d = xv[j] - yv[j];
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);    // sign(0) = 0, as torch's abs backward
    const float m = sMass[0][(threadIdx.x >> 5) * 4 + j] * sMass[1][threadIdx.x & 31];
    dxo[((int64_t)b * 3 + c) * HW + (int64_t)(gy0 + j) * W + gx] = dx[j] + k1 * sgn * m;
  }
}

// workgroups of the pixel kernel, forward and backward
int pix_blocks(int64_t N) { return parts_for(N, kThreads, kPixMaxBlocks); }

// the forward's scratch: the per-pixel L1 planes, then one partial sum per workgroup of the pixel kernel; returns its size
struct FwdScratch { float* l1f; double* part; };
int64_t fwd_layout(void* base, int64_t N, FwdScratch* f) {
  Carver c(base);
  f->l1f = c.take<float>(N * 3);
  f->part = c.take<double>(pix_blocks(N));
  return c.end;      // NOT c.total(): this size has never been padded, and callers' records hold it
}

// Host-side validation and the kernels' parameter block; no HIP call.
int make_params(const hdiff_msssim_desc* d, Params* P, const char* who) {
  HDIFF_CHECK_ARG(d, "%s: null descriptor", who);
  HDIFF_CHECK_ARG(d->C == 3, "%s: %d channels; the loss takes 3-channel images", who, d->C);
  HDIFF_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->H > 0 && d->W > 0, "%s: bad sizes B=%d H=%d W=%d", who, d->B, d->H, d->W);
  HDIFF_CHECK_ARG(d->nscales >= 1 && d->nscales <= kMaxScales, "%s: %d scales; at most %d", who, d->nscales, kMaxScales);
  HDIFF_CHECK_ARG(d->window >= 1 && d->window <= kMaxWin && (d->window & 1), "%s: window of %d taps; odd and at most %d (sigma_max 8)",
                  who, d->window, kMaxWin);
  HDIFF_CHECK_ARG(d->weights, "%s: null weight table", who);
  HDIFF_CHECK_ARG(d->npairs >= 1 && d->npairs <= kMaxPairs, "%s: %d pairs; at most %d", who, d->npairs, kMaxPairs);
  HDIFF_CHECK_ARG(d->l1_scale >= 0 && d->l1_scale < d->nscales, "%s: l1_scale %d out of range", who, d->l1_scale);
  HDIFF_CHECK_ARG(d->data_range > 0.f, "%s: data_range must be positive", who);
  const int64_t tiles = (int64_t)cdiv(d->W, kTile) * cdiv(d->H, kTile);
  HDIFF_CHECK_ARG(tiles < (1ll << 31) && (int64_t)d->B * d->H * d->W * kMaxPairs * 5 < (1ll << 40), "%s: image too large", who);
  memset(P, 0, sizeof(*P));
  P->B = d->B; P->H = d->H; P->W = d->W; P->tiles_x = cdiv(d->W, kTile);
  P->nscales = d->nscales; P->npairs = d->npairs; P->l1_scale = d->l1_scale;
  const int half = d->window / 2;
  for (int s = 0; s < d->nscales; ++s) {
    int eff = 0;
    for (int k = -half; k <= half; ++k) {
      const float w = d->weights[s * d->window + half + k];
      HDIFF_CHECK_ARG(w == w && w >= 0.f, "%s: bad weight", who);
      P->w[s][kHalo + k] = w;
      if (w > 1e-12f && abs(k) > eff) eff = abs(k);
    }
    P->radius[s] = eff <= 4 ? 4 : (eff <= 8 ? 8 : 16);
    for (int k = -kHalo; k <= kHalo; ++k)
      if (abs(k) > P->radius[s]) P->w[s][kHalo + k] = 0.f;     // the skipped taps, also for the L1 border mass
  }
  for (int p = 0; p < d->npairs; ++p) {
    HDIFF_CHECK_ARG(d->pair_chan[p] >= 0 && d->pair_chan[p] < 3 && d->pair_scale[p] >= 0 && d->pair_scale[p] < d->nscales &&
                        d->pair_cs_pow[p] >= 0 && d->pair_cs_pow[p] <= kMaxPairs && d->pair_l_pow[p] >= 0 && d->pair_l_pow[p] <= 3,
                    "%s: bad pair %d", who, p);
    P->chan[p] = d->pair_chan[p]; P->scale[p] = d->pair_scale[p];
    P->cs_pow[p] = d->pair_cs_pow[p]; P->l_pow[p] = d->pair_l_pow[p];
  }
  P->C1 = d->C1; P->C2 = d->C2; P->alpha = d->alpha; P->comp = d->compensation; P->inv_range = 1.0f / d->data_range;
  P->red_scale = d->mean ? 1.0 / ((double)d->B * d->H * d->W) : 1.0;
  return HDIFF_OK;
}

}  // namespace

extern "C" {

int hdiff_msssim_l1_workspace(const hdiff_msssim_desc* d, int64_t* saved_bytes, int64_t* scratch_bytes) {
  Params P;
  const int rc = make_params(d, &P, "msssim_l1_workspace");
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(saved_bytes && scratch_bytes, "msssim_l1_workspace: null pointer");
  const int64_t N = (int64_t)d->B * d->H * d->W;
  *saved_bytes = N * d->npairs * 5 * (int64_t)sizeof(float);
  FwdScratch f;
  const int64_t fwd = fwd_layout(nullptr, N, &f);
  const int64_t bwd = N * d->npairs * 3 * (int64_t)sizeof(float);
  *scratch_bytes = fwd > bwd ? fwd : bwd;
  return HDIFF_OK;
}

int hdiff_msssim_l1_fwd(const hdiff_msssim_desc* d, const float* x, const float* y, float* loss, void* saved, void* scratch,
                        hdiff_stream_t stream) {
  Params P;
  const int rc = make_params(d, &P, "msssim_l1_fwd");
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && y && loss && saved && scratch, "msssim_l1_fwd: null pointer");
  (void)hipGetLastError();
  const int64_t N = (int64_t)P.B * P.H * P.W;
  float* mom = (float*)saved;
  FwdScratch f;
  fwd_layout(scratch, N, &f);
  const int tiles = P.tiles_x * cdiv(P.H, kTile), nb = pix_blocks(N);
  hipLaunchKernelGGL(msssim_moments_kernel, dim3(tiles, P.npairs + 3, P.B), dim3(kThreads), 0, (hipStream_t)stream, P, x, y, mom,
                     f.l1f);
  hipLaunchKernelGGL(msssim_pixel_kernel<false>, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, P, (const float*)mom,
                     (const float*)f.l1f, (const float*)nullptr, f.part, (float*)nullptr);
  hipLaunchKernelGGL(msssim_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)f.part, nb, P.red_scale,
                     loss);
  HDIFF_CHECK_LAUNCH("msssim_l1_fwd kernels");
  return HDIFF_OK;
}

int hdiff_msssim_l1_bwd(const hdiff_msssim_desc* d, const float* x, const float* y, const float* d_loss, const void* saved,
                        void* scratch, float* dx, hdiff_stream_t stream) {
  Params P;
  const int rc = make_params(d, &P, "msssim_l1_bwd");
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(x && y && d_loss && saved && scratch && dx, "msssim_l1_bwd: null pointer");
  (void)hipGetLastError();
  const int64_t N = (int64_t)P.B * P.H * P.W;
  float* coef = (float*)scratch;
  const int tiles = P.tiles_x * cdiv(P.H, kTile);
  hipLaunchKernelGGL(msssim_pixel_kernel<true>, dim3(pix_blocks(N)), dim3(kThreads), 0, (hipStream_t)stream, P, (const float*)saved,
                     (const float*)nullptr, d_loss, (double*)nullptr, coef);
  hipLaunchKernelGGL(msssim_adjoint_kernel, dim3(tiles, 3, P.B), dim3(kThreads), 0, (hipStream_t)stream, P, x, y, (const float*)coef,
                     d_loss, dx);
  HDIFF_CHECK_LAUNCH("msssim_l1_bwd kernels");
  return HDIFF_OK;
}

}  // extern "C"
