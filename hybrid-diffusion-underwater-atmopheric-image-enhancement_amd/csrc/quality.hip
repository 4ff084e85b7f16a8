// Image-quality scores on the device: PSNR / SSIM of a pair and UIQM = UICM + UISM + UIConM of one image, as the evaluation of the
// reference's utils/rotinas.py:916-928 takes them per image (hdiff_amd/metrics.py and uw_metrics.py are the host restatements).
// Inputs are fp32 [N][3][H][W] with nominal range [0, 1]; every kernel forms v = min(max(x, 0), 1) * 255 in fp32 first (np.clip(img, 0,
// 1) * 255: a float image, not rounded).  Outputs are float64, one row per image.  Images are on blockIdx.z; nothing here depends on N
// or on an image's position in the batch: grids and partial counts are functions of H and W alone.
//
// hdiff_psnr_ssim, two launches:
//   1. ssim_tile_kernel      grid (32x32 tiles, 3, N).  The 38x38 patch of both planes is staged in LDS ([38][39]); every thread owns
//                            four vertically adjacent pixels: the 7x7 window whose top-left corner is that pixel (valid while it stays
//                            inside the image: the (H-6)(W-6) interior positions of the definition), five window moments in double from
//                            sliding row sums, the per-position SSIM; and the squared difference of the owned pixel itself.  float64
//                            block sums in a fixed order into one record per workgroup {sum SSIM, sum d^2, non-finite seen}.
//   2. ssim_finalize_kernel  grid (N): adds the records in index order; psnr, ssim.
// hdiff_uiqm, twelve launches:
//   1. uiqm_init_kernel      zeroes histograms / plane maxima / flags, sets the four selects of every image (2 planes x 2 ranks)
//   2-7. uicm_hist_kernel + uicm_scan_kernel, three times (11 / 11 / 10 bits): radix select of the two cut values of rg = R - G and of
//                            yb = (R + G) / 2 - B on the order-preserving integer key of the fp32 value.  Histograms: integer LDS atomics
//                            per workgroup, merged with integer global atomics (counts do not depend on arrival order).
//   8. uicm_kept_kernel      double sum of the samples strictly between the two cut values (the copies of the cut values are counted)
//   9. uicm_var_kernel       every workgroup rebuilds the trimmed means from the partials (same order everywhere), then sum (v - mu)^2
//  10. sobel_max_kernel      grid (tiles, 1, N): per channel the 34x34 patch in LDS ([34][35], border pixel repeated), Sobel magnitude,
//                            plane maximum by integer max on the bit pattern; on the way the min / max of every full 8x8 block over the
//                            three channels: UIConM's terms
//  11. uism_kernel           the same patch again: t = mag * (255 / M) * v, block extrema (16 lanes per 8x8 block), sum log(hi / lo)
//  12. uiqm_finalize_kernel  grid (N): adds the partials in index order; uicm, uism, uiconm, uiqm
// No float atomics: results are bitwise repeatable.  A non-finite input value sets a per-image flag, and the finalize kernels write NaN
// for that image alone.  The file is compiled with -ffp-contract=off: the fp32 formulas round where numpy's separate operations round.
#include <math.h>

#include "common.h"
#include "radix_select.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kWin = 7;
constexpr int kSsimIn = kTile + kWin - 1;      // 38
constexpr int kSsimPitch = kSsimIn + 1;        // 39, odd
constexpr int kSobIn = kTile + 2;              // 34
constexpr int kSobPitch = kSobIn + 1;          // 35, odd
constexpr int kBins = 2048;
constexpr int kSelects = 4;                    // select = plane * 2 + (0: left cut, 1: right cut)
constexpr int kMaxPixBlocks = 128;
constexpr int kPixPerBlock = kThreads * 16;

using Cut = Select<unsigned>;                  // on the 32-bit key of the fp32 sample

__device__ __forceinline__ float scaled(float x) { return fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f; }

// ---------------------------------------------------------------------------------------------------------------- PSNR / SSIM
// rec: [N][3][tiles][3] = {sum of SSIM over the tile's valid positions, sum of squared differences over its pixels, flag}
__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                              int tiles_x, double* __restrict__ rec) {
  __shared__ float sA[kSsimIn * kSsimPitch];
  __shared__ float sB[kSsimIn * kSsimPitch];
  const int c = blockIdx.y, n = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
  const int64_t HW = (int64_t)H * W;
  const float* pa = a + ((int64_t)n * 3 + c) * HW;
  const float* pb = b + ((int64_t)n * 3 + c) * HW;
  int bad = 0;
  for (int i = threadIdx.x; i < kSsimIn * kSsimIn; i += kThreads) {
    const int r = i / kSsimIn, q = i - r * kSsimIn;
    const int gy = ty0 + r, gx = tx0 + q;
    float va = 0.0f, vb = 0.0f;
    if (gy < H && gx < W) {
      const float xa = pa[(int64_t)gy * W + gx], xb = pb[(int64_t)gy * W + gx];
      bad |= non_finite(xa) || non_finite(xb);
      va = scaled(xa);
      vb = scaled(xb);
    }
    sA[r * kSsimPitch + q] = va;
    sB[r * kSsimPitch + q] = vb;
  }
  bad = __syncthreads_or(bad);
  const int col = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
  double m[4][5];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 5; ++k) m[j][k] = 0.0;
#pragma unroll
  for (int k = 0; k < kWin + 3; ++k) {
    double rs[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int base = (r0 + k) * kSsimPitch + col;
#pragma unroll
    for (int dx = 0; dx < kWin; ++dx) {
      const double x = (double)sA[base + dx], y = (double)sB[base + dx];
      rs[0] += x; rs[1] += y; rs[2] += x * x; rs[3] += y * y; rs[4] += x * y;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k - j >= 0 && k - j < kWin) {
#pragma unroll
        for (int q = 0; q < 5; ++q) m[j][q] += rs[q];
      }
  }
  constexpr double npix = kWin * kWin, cov = npix / (npix - 1.0);
  constexpr double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  double ssum = 0.0, dsum = 0.0;
  const int gx = tx0 + col;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = ty0 + r0 + j;
    if (gy < H && gx < W) {
      const double d = (double)sA[(r0 + j) * kSsimPitch + col] - (double)sB[(r0 + j) * kSsimPitch + col];
      dsum += d * d;
    }
    if (gy <= H - kWin && gx <= W - kWin) {
      const double ux = m[j][0] / npix, uy = m[j][1] / npix, uxx = m[j][2] / npix, uyy = m[j][3] / npix, uxy = m[j][4] / npix;
      const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
      const double num = (2.0 * ux * uy + c1) * (2.0 * vxy + c2);
      const double den = (ux * ux + uy * uy + c1) * (vx + vy + c2);
      ssum += num / den;
    }
  }
  const double s = block_sum_all<kThreads>(ssum), d2 = block_sum_all<kThreads>(dsum);
  if (threadIdx.x == 0) {
    double* o = rec + (((int64_t)n * 3 + c) * gridDim.x + blockIdx.x) * 3;
    o[0] = s; o[1] = d2; o[2] = bad ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void ssim_finalize_kernel(const double* __restrict__ rec, int tiles, int H, int W,
                                                                  double* __restrict__ out) {
  const int n = blockIdx.x;
  const double* r = rec + (int64_t)n * 3 * tiles * 3;
  const double positions = (double)(H - kWin + 1) * (double)(W - kWin + 1);
  double ssim = 0.0, sq = 0.0, bad = 0.0;
  for (int c = 0; c < 3; ++c) {
    ssim += sum_partials<kThreads>(r + (int64_t)c * tiles * 3, tiles, 3) / positions;
    sq += sum_partials<kThreads>(r + (int64_t)c * tiles * 3 + 1, tiles, 3);
    bad += sum_partials<kThreads>(r + (int64_t)c * tiles * 3 + 2, tiles, 3);
  }
  if (threadIdx.x != 0) return;
  const double mse = sq / (3.0 * (double)H * (double)W);
  double psnr = mse == 0.0 ? (double)INFINITY : 10.0 * log10((255.0 * 255.0) / mse);
  ssim = ssim / 3.0;
  if (bad != 0.0) psnr = ssim = (double)NAN;
  out[2 * n] = psnr;
  out[2 * n + 1] = ssim;
}

// ---------------------------------------------------------------------------------------------------------------- UIQM
struct UiqmWs {
  unsigned* hist;      // [3 passes][N][kSelects][kBins]
  Cut* sel;            // [N][kSelects]
  unsigned* mbits;     // [N][3]  bit pattern of the largest Sobel magnitude
  unsigned* flag;      // [N]
  double* kept;        // [N][pix_blocks][2]
  double* var;         // [N][pix_blocks][2]
  double* eme;         // [N][3][tiles]
  double* con;         // [N][tiles]
};

struct UiqmParams {
  int N, H, W, tiles_x, tiles, pix_blocks;
  unsigned K, lo_rank, hi_rank;      // kept = sorted[lo_rank .. hi_rank]
  float inv_count;                   // fp32(1 / (K - t_l - t_r))
  double eme_blocks, con_blocks;     // ceil(H/8) ceil(W/8) and floor(H/8) floor(W/8)
};

__device__ __forceinline__ void colour_pair(const float* __restrict__ img, int64_t HW, int64_t i, float& rg, float& yb, int& bad) {
  const float xr = img[i], xg = img[HW + i], xb = img[2 * HW + i];
  bad |= non_finite(xr) || non_finite(xg) || non_finite(xb);
  const float R = scaled(xr), G = scaled(xg), B = scaled(xb);
  rg = R - G;
  yb = ((R + G) / 2.0f) - B;
}

__global__ __launch_bounds__(kThreads) void uiqm_init_kernel(const UiqmParams P, const UiqmWs ws) {
  const int64_t nh = (int64_t)3 * P.N * kSelects * kBins;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nh; i += (int64_t)gridDim.x * kThreads) ws.hist[i] = 0u;
  if (blockIdx.x != 0) return;
  for (int i = threadIdx.x; i < P.N * 3; i += kThreads) ws.mbits[i] = 0u;
  for (int i = threadIdx.x; i < P.N; i += kThreads) ws.flag[i] = 0u;
  for (int i = threadIdx.x; i < P.N * kSelects; i += kThreads) ws.sel[i] = select_start<unsigned>((i & 1) ? P.hi_rank : P.lo_rank);
}

// One digit of the select: counts, per select, the samples whose key agrees with the select's prefix above `match_shift`
// (match_shift == 32: every sample, one histogram per plane), binned by the `bits` bits below it.
__global__ __launch_bounds__(kThreads) void uicm_hist_kernel(const UiqmParams P, const UiqmWs ws, const float* __restrict__ x, int pass,
                                                              int match_shift, int bits) {
  __shared__ unsigned sh[kSelects * kBins];
  const int n = blockIdx.z;
  for (int i = threadIdx.x; i < kSelects * kBins; i += kThreads) sh[i] = 0u;
  unsigned prefix[kSelects];
#pragma unroll
  for (int s = 0; s < kSelects; ++s) prefix[s] = ws.sel[n * kSelects + s].prefix;
  __syncthreads();
  const int64_t HW = (int64_t)P.H * P.W;
  const float* img = x + (int64_t)n * 3 * HW;
  const int bin_shift = match_shift - bits;
  const unsigned mask = (1u << bits) - 1u;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    float rg, yb;
    colour_pair(img, HW, i, rg, yb, bad);
    const unsigned key[2] = {key_of(rg), key_of(yb)};
#pragma unroll
    for (int s = 0; s < kSelects; ++s) {
      const unsigned k = key[s >> 1];
      if (match_shift == 32) {
        if ((s & 1) == 0) atomicAdd(&sh[s * kBins + (k >> bin_shift)], 1u);      // first digit: select_hist's rule, one histogram per plane
      } else if ((k >> match_shift) == prefix[s]) {
        atomicAdd(&sh[s * kBins + ((k >> bin_shift) & mask)], 1u);
      }
    }
  }
  if (pass == 0 && bad) ws.flag[n] = 1u;
  select_flush<kThreads>(sh, ws.hist + ((int64_t)pass * P.N + n) * kSelects * kBins, kSelects * kBins);
}

// grid (kSelects, 1, N): the bin that holds the select's rank; prefix, rank within the bin, samples below and inside it
__global__ __launch_bounds__(kThreads) void uicm_scan_kernel(const UiqmParams P, const UiqmWs ws, int pass, int bits) {
  const int s = blockIdx.x, n = blockIdx.z;
  const unsigned* h = ws.hist + (((int64_t)pass * P.N + n) * kSelects + select_hist(pass, s)) * kBins;
  select_scan<kThreads, kBins>(h, &ws.sel[n * kSelects + s], bits);
}

// kept: [N][pix_blocks][2]: per plane the double sum of the samples whose key lies strictly between the two cut keys
__global__ __launch_bounds__(kThreads) void uicm_kept_kernel(const UiqmParams P, const UiqmWs ws, const float* __restrict__ x) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)P.H * P.W;
  const float* img = x + (int64_t)n * 3 * HW;
  const unsigned lo0 = ws.sel[n * kSelects + 0].prefix, hi0 = ws.sel[n * kSelects + 1].prefix;
  const unsigned lo1 = ws.sel[n * kSelects + 2].prefix, hi1 = ws.sel[n * kSelects + 3].prefix;
  double a0 = 0.0, a1 = 0.0;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    float rg, yb;
    colour_pair(img, HW, i, rg, yb, bad);
    const unsigned k0 = key_of(rg), k1 = key_of(yb);
    if (k0 > lo0 && k0 < hi0) a0 += (double)rg;
    if (k1 > lo1 && k1 < hi1) a1 += (double)yb;
  }
  const double s0 = block_sum_all<kThreads>(a0), s1 = block_sum_all<kThreads>(a1);
  if (threadIdx.x == 0) {
    double* o = ws.kept + ((int64_t)n * P.pix_blocks + blockIdx.x) * 2;
    o[0] = s0; o[1] = s1;
  }
}

// The trimmed mean of one plane from the partial sums and the select's counts (every thread; ends with a barrier).
__device__ float trimmed_mean(const UiqmParams& P, const UiqmWs& ws, int n, int plane) {
  const double between = sum_partials<kThreads>(ws.kept + (int64_t)n * P.pix_blocks * 2 + plane, P.pix_blocks, 2);
  const Cut lo = ws.sel[n * kSelects + plane * 2], hi = ws.sel[n * kSelects + plane * 2 + 1];
  const double vlo = (double)value_of(lo.prefix), vhi = (double)value_of(hi.prefix);
  double total;
  if (lo.prefix == hi.prefix) {
    total = (double)(P.hi_rank - P.lo_rank + 1u) * vlo;
  } else {
    total = between + (double)(lo.less + lo.eq - P.lo_rank) * vlo + (double)(P.hi_rank - hi.less + 1u) * vhi;
  }
  return (float)((double)P.inv_count * total);
}

// var: [N][pix_blocks][2]: sum over ALL samples of double(fp32(v - mu))^2
__global__ __launch_bounds__(kThreads) void uicm_var_kernel(const UiqmParams P, const UiqmWs ws, const float* __restrict__ x) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)P.H * P.W;
  const float* img = x + (int64_t)n * 3 * HW;
  const float mu0 = trimmed_mean(P, ws, n, 0), mu1 = trimmed_mean(P, ws, n, 1);
  double a0 = 0.0, a1 = 0.0;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    float rg, yb;
    colour_pair(img, HW, i, rg, yb, bad);
    const double d0 = (double)(rg - mu0), d1 = (double)(yb - mu1);
    a0 += d0 * d0;
    a1 += d1 * d1;
  }
  const double s0 = block_sum_all<kThreads>(a0), s1 = block_sum_all<kThreads>(a1);
  if (threadIdx.x == 0) {
    double* o = ws.var + ((int64_t)n * P.pix_blocks + blockIdx.x) * 2;
    o[0] = s0; o[1] = s1;
  }
}

// The 34x34 patch around a 32x32 tile, border pixel repeated (scipy's `reflect` at radius 1); pixels past the image end repeat too
// and are never used by a pixel inside it.
__device__ void stage_sobel(float* s, const float* __restrict__ plane, int H, int W, int ty0, int tx0) {
  for (int i = threadIdx.x; i < kSobIn * kSobIn; i += kThreads) {
    const int r = i / kSobIn, q = i - r * kSobIn;
    int gy = ty0 - 1 + r, gx = tx0 - 1 + q;
    gy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy);
    gx = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
    s[r * kSobPitch + q] = scaled(plane[(int64_t)gy * W + gx]);
  }
}

// scipy.ndimage.sobel on an fp32 plane, both axes, at patch position (r, q) = image pixel + 1: the difference is one fp32
// subtraction, the [1, 2, 1] smoothing of three fp32 values is exact in double and rounded once.  The magnitude is the square
// root of the double sum of squares, rounded to double and then to fp32: hypotf to within that double rounding.
__device__ __forceinline__ float sobel_mag(const float* s, int r, int q) {
  const float* p = s + r * kSobPitch + q;
  float dv[3], dh[3];
#pragma unroll
  for (int k = -1; k <= 1; ++k) {
    dv[k + 1] = p[kSobPitch + k] - p[-kSobPitch + k];
    dh[k + 1] = p[k * kSobPitch + 1] - p[k * kSobPitch - 1];
  }
  const float sx = (float)(2.0 * (double)dv[1] + ((double)dv[0] + (double)dv[2]));
  const float sy = (float)(2.0 * (double)dh[1] + ((double)dh[0] + (double)dh[2]));
  return (float)sqrt((double)sx * (double)sx + (double)sy * (double)sy);
}

// thread -> (8x8 block of the tile, four adjacent pixels of one of its rows); the 16 lanes of a block are adjacent in a wave
struct BlockLane { int blk, row, col0; };
__device__ __forceinline__ BlockLane block_lane() {
  const int blk = threadIdx.x >> 4, sub = threadIdx.x & 15;
  return {blk, (blk >> 2) * 8 + (sub >> 1), (blk & 3) * 8 + (sub & 1) * 4};
}
__device__ __forceinline__ float lanes16_min(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float lanes16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (tiles, 1, N): plane maxima of the Sobel magnitude (mbits) and the tile's sum of UIConM terms (con)
__global__ __launch_bounds__(kThreads) void sobel_max_kernel(const UiqmParams P, const UiqmWs ws, const float* __restrict__ x) {
  __shared__ float sV[kSobIn * kSobPitch];
  __shared__ unsigned sMax[kThreads / 64];
  __shared__ double sTerm[16];
  const int n = blockIdx.z, H = P.H, W = P.W;
  const int ty0 = (blockIdx.x / P.tiles_x) * kTile, tx0 = (blockIdx.x % P.tiles_x) * kTile;
  const int64_t HW = (int64_t)H * W;
  const BlockLane L = block_lane();
  const int gy = ty0 + L.row;
  float lo = 3.402823466e+38f, hi = 0.0f;      // v is in [0, 255]
  for (int c = 0; c < 3; ++c) {
    __syncthreads();
    stage_sobel(sV, x + ((int64_t)n * 3 + c) * HW, H, W, ty0, tx0);
    __syncthreads();
    float mx = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gx = tx0 + L.col0 + j;
      if (gy < H && gx < W) {
        mx = fmaxf(mx, sobel_mag(sV, L.row + 1, L.col0 + j + 1));
        const float v = sV[(L.row + 1) * kSobPitch + L.col0 + j + 1];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) sMax[threadIdx.x >> 6] = __builtin_bit_cast(unsigned, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned m = sMax[0];
      for (int i = 1; i < kThreads / 64; ++i) m = sMax[i] > m ? sMax[i] : m;
      if (m) atomicMax(&ws.mbits[n * 3 + c], m);      // non-negative floats order like their bit patterns
    }
  }
  lo = lanes16_min(lo);
  hi = lanes16_max(hi);
  if ((threadIdx.x & 15) == 0) {
    const int by = ty0 + (L.blk >> 2) * 8, bx = tx0 + (L.blk & 3) * 8;
    double term = 0.0;
    if (by + 8 <= H && bx + 8 <= W) {               // full blocks only
      const float top = hi - lo, bot = hi + lo;
      if (top != 0.0f && bot != 0.0f) {
        const double r = (double)(top / bot);
        term = r * log(r);
      }
    }
    sTerm[L.blk] = term;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < 16; ++i) s += sTerm[i];
    ws.con[(int64_t)n * P.tiles + blockIdx.x] = s;
  }
}

// grid (tiles, 3, N): eme[n][c][tile] = sum over the tile's blocks (edge blocks smaller) of log(hi / lo) of t = mag * (255 / M) * v
__global__ __launch_bounds__(kThreads) void uism_kernel(const UiqmParams P, const UiqmWs ws, const float* __restrict__ x) {
  __shared__ float sV[kSobIn * kSobPitch];
  __shared__ double sTerm[16];
  const int c = blockIdx.y, n = blockIdx.z, H = P.H, W = P.W;
  const int ty0 = (blockIdx.x / P.tiles_x) * kTile, tx0 = (blockIdx.x % P.tiles_x) * kTile;
  const int64_t HW = (int64_t)H * W;
  const float M = __builtin_bit_cast(float, ws.mbits[n * 3 + c]);
  const float scale = 255.0f / M;                   // M == 0 (a constant plane): the finalize kernel writes NaN for the image
  stage_sobel(sV, x + ((int64_t)n * 3 + c) * HW, H, W, ty0, tx0);
  __syncthreads();
  const BlockLane L = block_lane();
  const int gy = ty0 + L.row;
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gx = tx0 + L.col0 + j;
    if (gy < H && gx < W) {
      const float mag = sobel_mag(sV, L.row + 1, L.col0 + j + 1);
      const float t = (mag * scale) * sV[(L.row + 1) * kSobPitch + L.col0 + j + 1];
      lo = fminf(lo, t);
      hi = fmaxf(hi, t);
    }
  }
  lo = lanes16_min(lo);
  hi = lanes16_max(hi);
  if ((threadIdx.x & 15) == 0) {
    const int by = ty0 + (L.blk >> 2) * 8, bx = tx0 + (L.blk & 3) * 8;
    double term = 0.0;
    if (by < H && bx < W) {
      const double dlo = lo == 0.0f ? 1.0 : (double)lo, dhi = hi == 0.0f ? 1.0 : (double)hi;
      term = log(dhi / dlo);
    }
    sTerm[L.blk] = term;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < 16; ++i) s += sTerm[i];
    ws.eme[((int64_t)n * 3 + c) * P.tiles + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kThreads) void uiqm_finalize_kernel(const UiqmParams P, const UiqmWs ws, double* __restrict__ out) {
  const int n = blockIdx.x;
  const double mu0 = (double)trimmed_mean(P, ws, n, 0), mu1 = (double)trimmed_mean(P, ws, n, 1);
  const double var0 = sum_partials<kThreads>(ws.var + (int64_t)n * P.pix_blocks * 2, P.pix_blocks, 2) / (double)P.K;
  const double var1 = sum_partials<kThreads>(ws.var + (int64_t)n * P.pix_blocks * 2 + 1, P.pix_blocks, 2) / (double)P.K;
  double e[3];
  for (int c = 0; c < 3; ++c) e[c] = (2.0 / P.eme_blocks) * sum_partials<kThreads>(ws.eme + ((int64_t)n * 3 + c) * P.tiles, P.tiles, 1);
  const double con = sum_partials<kThreads>(ws.con + (int64_t)n * P.tiles, P.tiles, 1);
  if (threadIdx.x != 0) return;
  double uicm = (-0.0268 * sqrt(mu0 * mu0 + mu1 * mu1)) + (0.1586 * sqrt(var0 + var1));
  double uism = (0.299 * e[0]) + (0.587 * e[1]) + (0.144 * e[2]);
  double uiconm = (-1.0 / P.con_blocks) * con;
  if (ws.mbits[n * 3] == 0u || ws.mbits[n * 3 + 1] == 0u || ws.mbits[n * 3 + 2] == 0u) uism = (double)NAN;
  double uiqm = (0.0282 * uicm) + (0.2953 * uism) + (3.5753 * uiconm);
  if (ws.flag[n]) uicm = uism = uiconm = uiqm = (double)NAN;
  out[4 * n] = uicm;
  out[4 * n + 1] = uism;
  out[4 * n + 2] = uiconm;
  out[4 * n + 3] = uiqm;
}

// ---------------------------------------------------------------------------------------------------------------- host side
int64_t ssim_bytes(int N, int tiles) { return align256((int64_t)N * 3 * tiles * 3 * (int64_t)sizeof(double)); }

// the regions of the UIQM workspace, in order; returns its size
int64_t uiqm_layout(void* base, int N, int tiles, int pb, UiqmWs* ws) {
  Carver c(base);
  ws->hist = c.take<unsigned>((int64_t)3 * N * kSelects * kBins);
  ws->sel = c.take<Cut>((int64_t)N * kSelects);
  ws->mbits = c.take<unsigned>((int64_t)N * 3);
  ws->flag = c.take<unsigned>(N);
  ws->kept = c.take<double>((int64_t)N * pb * 2);
  ws->var = c.take<double>((int64_t)N * pb * 2);
  ws->eme = c.take<double>((int64_t)N * 3 * tiles);
  ws->con = c.take<double>((int64_t)N * tiles);
  return c.total();
}

}  // namespace

extern "C" {

int hdiff_quality_workspace(int N, int H, int W, int64_t* bytes) {
  const int rc = check_sizes("quality_workspace", N, H, W, kWin);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "quality_workspace: null pointer");
  const int tiles = cdiv(W, kTile) * cdiv(H, kTile);
  UiqmWs ws;
  const int64_t u = uiqm_layout(nullptr, N, tiles, parts_for((int64_t)H * W, kPixPerBlock, kMaxPixBlocks), &ws), s = ssim_bytes(N, tiles);
  *bytes = u > s ? u : s;
  return HDIFF_OK;
}

int hdiff_psnr_ssim(const float* a, const float* b, int N, int H, int W, double* out, void* scratch, hdiff_stream_t stream) {
  const int rc = check_sizes("psnr_ssim", N, H, W, kWin);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && b && out && scratch, "psnr_ssim: null pointer");
  (void)hipGetLastError();
  const int tiles_x = cdiv(W, kTile), tiles = tiles_x * cdiv(H, kTile);
  double* rec = (double*)scratch;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3(tiles, 3, N), dim3(kThreads), 0, (hipStream_t)stream, a, b, H, W, tiles_x, rec);
  hipLaunchKernelGGL(ssim_finalize_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, (const double*)rec, tiles, H, W, out);
  HDIFF_CHECK_LAUNCH("psnr_ssim kernels");
  return HDIFF_OK;
}

int hdiff_uiqm(const float* a, int N, int H, int W, double* out, void* scratch, hdiff_stream_t stream) {
  const int rc = check_sizes("uiqm", N, H, W, 8);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && out && scratch, "uiqm: null pointer");
  (void)hipGetLastError();
  UiqmParams P;
  P.N = N; P.H = H; P.W = W;
  P.tiles_x = cdiv(W, kTile);
  P.tiles = P.tiles_x * cdiv(H, kTile);
  const int64_t K = (int64_t)H * W;
  P.pix_blocks = parts_for(K, kPixPerBlock, kMaxPixBlocks);
  P.K = (unsigned)K;
  const int64_t t_l = (int64_t)ceil(0.1 * (double)K), t_r = (int64_t)floor(0.1 * (double)K);
  P.lo_rank = (unsigned)(t_l + 1);
  P.hi_rank = (unsigned)(K - t_r - 1);           // K >= 64: lo_rank <= hi_rank
  P.inv_count = (float)(1.0 / (double)(K - t_l - t_r));
  P.eme_blocks = (double)cdiv(H, 8) * (double)cdiv(W, 8);
  P.con_blocks = (double)(H / 8) * (double)(W / 8);
  UiqmWs ws;
  uiqm_layout(scratch, N, P.tiles, P.pix_blocks, &ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads), pix(P.pix_blocks, 1, N);
  const int64_t nh = (int64_t)3 * N * kSelects * kBins;
  const int init_blocks = (int)((nh / kThreads) > 1024 ? 1024 : (nh / kThreads));
  hipLaunchKernelGGL(uiqm_init_kernel, dim3(init_blocks), blk, 0, s, P, ws);
  const int bits[3] = {11, 11, 10};
  int shift = 32;
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(uicm_hist_kernel, pix, blk, 0, s, P, ws, a, pass, shift, bits[pass]);
    hipLaunchKernelGGL(uicm_scan_kernel, dim3(kSelects, 1, N), blk, 0, s, P, ws, pass, bits[pass]);
    shift -= bits[pass];
  }
  hipLaunchKernelGGL(uicm_kept_kernel, pix, blk, 0, s, P, ws, a);
  hipLaunchKernelGGL(uicm_var_kernel, pix, blk, 0, s, P, ws, a);
  hipLaunchKernelGGL(sobel_max_kernel, dim3(P.tiles, 1, N), blk, 0, s, P, ws, a);
  hipLaunchKernelGGL(uism_kernel, dim3(P.tiles, 3, N), blk, 0, s, P, ws, a);
  hipLaunchKernelGGL(uiqm_finalize_kernel, dim3(N), blk, 0, s, P, ws, out);
  HDIFF_CHECK_LAUNCH("uiqm kernels");
  return HDIFF_OK;
}

}  // extern "C"
