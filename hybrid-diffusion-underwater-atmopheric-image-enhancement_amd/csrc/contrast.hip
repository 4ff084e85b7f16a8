// Contrast enhancement from the histogram, on the device: contrast-limited adaptive histogram equalisation (CLAHE, Zuiderveld 1994, on
// 8-bit planes with bilinearly blended tile tables) and global equalisation by Pillow's rule -- the baselines that lift the
// no-reference scores (UIConM, UCIQE's contrast term) without a model.  tests/_contrast_def.py is the definition the kernels are held
// to; hdiff_amd/classical.py is the caller and composes the passes.  Conventions are those of classical.hip: images fp32 [N][3][H][W],
// read as X_c = min(max(I_c, 0), 1) in fp32 (a NaN clips to 0), images on blockIdx.z, planes on blockIdx.y, grids functions of H and W.
//
//   hdiff_contrast_quantise  one launch: X -> q, uint8 [N][P][H][W].  "rgb" (P = 3): q_c = floor(double(X_c) 255 + 0.5).  "lab" (P = 1):
//                            q = clamp(floor(L 2.55 + 0.5), 0, 255), L of srgb_to_lab(double(X)) (lab.h).  a and b are NOT kept: the
//                            apply kernel recomputes them from X with the same function (the same bits) -- three pow and three cbrt per
//                            pixel there against 16 bytes per pixel written here and read back there.
//   hdiff_clahe_luts         one launch, one workgroup per (tile, plane, image): the tile's 256-bin histogram in LDS by integer LDS
//                            atomics, read through the reflect-101 index map (no padded copy); clip, redistribution and the prefix sum
//                            by two 256-wide integer scans; the table written as 256 bytes.
//   hdiff_equalize_luts      two launches: per-workgroup LDS histograms stored to slots of their own; one workgroup per plane adds the
//                            slots in index order and applies Pillow's rule.  Integers throughout: no arrival order enters.
//   hdiff_contrast_apply     one launch: q' from four table entries blended in fp32 (CLAHE) or from one (equalisation), then fp32(q' /
//                            255), or in "lab" the inverse conversion in double with L' = q' / 2.55.
// A single LDS histogram per workgroup, no per-wave copies: none was measured to pay.  No float atomics, no allocation, no
// synchronisation.  Compiled with -ffp-contract=off: every fp32 operation of the blend rounds on its own, as the definition's does.
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "lab.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;                     // == kThreads: thread t owns bin t
constexpr int kMaxTiles = 16;
constexpr int kMaxParts = 64;                  // equalisation: histogram slots per plane
constexpr int kPerBlock = kThreads * 16;

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// inclusive scan of one value per thread over the workgroup, and the total; `sh` holds kThreads words
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* sh, unsigned& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const unsigned below = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += below;
    __syncthreads();
  }
  const unsigned mine = sh[t];
  total = sh[kThreads - 1];
  __syncthreads();
  return mine;
}

// ---------------------------------------------------------------------------------------------------------------- quantisation
// grid (parts, P, N)
__global__ __launch_bounds__(kThreads) void quantise_kernel(const float* __restrict__ img, int64_t HW, int lab, uint8_t* __restrict__ q) {
  const int n = blockIdx.z, p = blockIdx.y;
  const float* src = img + (int64_t)n * 3 * HW;
  uint8_t* dst = q + ((int64_t)n * gridDim.y + p) * HW;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    if (lab) {
      double L, ca, cb;
      srgb_to_lab((double)clip01(src[i]), (double)clip01(src[HW + i]), (double)clip01(src[2 * HW + i]), L, ca, cb);
      dst[i] = (uint8_t)fmin(fmax(floor(L * 2.55 + 0.5), 0.0), 255.0);
    } else {
      dst[i] = (uint8_t)floor((double)clip01(src[p * HW + i]) * 255.0 + 0.5);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- CLAHE tables
// grid (tiles_y tiles_x, P, N).  A padded row y >= H is row 2 H - 2 - y: with at most tiles_y - 1 <= H - 1 padded rows that is a row
// in [0, H); the same for columns.  Every read is inside the plane, every write inside the tile's 256 bytes.
__global__ __launch_bounds__(kThreads) void clahe_luts_kernel(const uint8_t* __restrict__ q, int H, int W, int tiles_x, int th, int tw,
                                                               unsigned clip, float scale, uint8_t* __restrict__ lut) {
  __shared__ unsigned hist[kBins];
  __shared__ unsigned scan[kThreads];
  const int t = threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
  const uint8_t* src = q + plane * ((int64_t)H * W);
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  hist[t] = 0u;
  __syncthreads();
  const int64_t area = (int64_t)th * tw;
  for (int64_t i = t; i < area; i += kThreads) {
    const int ly = (int)(i / tw), lx = (int)(i - (int64_t)ly * tw);
    int y = tile_y * th + ly, x = tile_x * tw + lx;
    if (y >= H) y = 2 * H - 2 - y;
    if (x >= W) x = 2 * W - 2 - x;
    atomicAdd(&hist[src[(int64_t)y * W + x]], 1u);
  }
  __syncthreads();
  unsigned h = hist[t];
  unsigned excess;
  block_scan(h > clip ? h - clip : 0u, scan, excess);
  h = (h < clip ? h : clip) + excess / kBins;
  const unsigned r = excess % kBins;
  if (r > 0u) {
    const unsigned step = kBins / r;               // r <= 255: at least 1, and r * step <= 256
    if (t % step == 0u && t / step < r) h += 1u;
  }
  unsigned total;
  const unsigned cum = block_scan(h, scan, total);
  lut[(plane * gridDim.x + blockIdx.x) * kBins + t] = (uint8_t)fminf(rintf((float)cum * scale), 255.0f);
}

// ---------------------------------------------------------------------------------------------------------------- equalisation tables
// grid (parts, P, N) -> part[plane][block][256]
__global__ __launch_bounds__(kThreads) void equalize_hist_kernel(const uint8_t* __restrict__ q, int64_t HW, unsigned* __restrict__ part) {
  __shared__ unsigned hist[kBins];
  const int t = threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
  const uint8_t* src = q + plane * HW;
  hist[t] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kThreads + t; i < HW; i += (int64_t)gridDim.x * kThreads) atomicAdd(&hist[src[i]], 1u);
  __syncthreads();
  part[(plane * gridDim.x + blockIdx.x) * kBins + t] = hist[t];
}

// grid (1, P, N).  Pillow's ImageOps.equalize: the identity with fewer than two filled bins or at step == 0; an entry above 255 is
// stored as 255 (what Image.point does with it).
__global__ __launch_bounds__(kThreads) void equalize_luts_kernel(const unsigned* __restrict__ part, int parts, int64_t HW,
                                                                  uint8_t* __restrict__ lut) {
  __shared__ unsigned scan[kThreads];
  __shared__ unsigned hist[kBins];
  __shared__ int last;
  const int t = threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
  const unsigned* src = part + plane * parts * kBins;
  unsigned h = 0u;
  for (int k = 0; k < parts; ++k) h += src[(int64_t)k * kBins + t];
  hist[t] = h;
  if (t == 0) last = 0;
  __syncthreads();
  if (h > 0u) atomicMax(&last, t);
  unsigned filled, total;
  block_scan(h > 0u ? 1u : 0u, scan, filled);      // (its barriers also order the atomicMax before the read of `last`)
  const unsigned before = block_scan(h, scan, total) - h;
  const unsigned step = (unsigned)((HW - (int64_t)hist[last]) / 255);
  const bool identity = filled < 2u || step == 0u;
  unsigned v = (unsigned)t;
  if (!identity) {
    v = (step / 2u + before) / step;
    if (v > 255u) v = 255u;
  }
  lut[plane * kBins + t] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------------------------- application
struct Blend {
  int tiles_y, tiles_x;      // 0, 0: one table per plane and no blend (equalisation)
  float inv_th, inv_tw;
};

// the two tile indices and weights of one axis
__device__ __forceinline__ void axis_weights(int at, float inv, int tiles, int& i1, int& i2, float& w1, float& w2) {
  const float f = (float)at * inv - 0.5f;
  const float fl = floorf(f);
  const int lo = (int)fl;
  w2 = f - fl;
  w1 = 1.0f - w2;
  i1 = lo > 0 ? lo : 0;
  i2 = lo + 1 < tiles - 1 ? lo + 1 : tiles - 1;
  if (i1 > tiles - 1) i1 = tiles - 1;      // never binds (f < tiles - 0.5 by construction); keeps the read in the tables whatever `inv` is
  if (i2 < 0) i2 = 0;                      // likewise (f >= -0.5)
}

// grid (parts, P, N)
__global__ __launch_bounds__(kThreads) void apply_kernel(const float* __restrict__ img, const uint8_t* __restrict__ q,
                                                          const uint8_t* __restrict__ lut, int64_t HW, int W, int lab, const Blend B,
                                                          float* __restrict__ out) {
  const int n = blockIdx.z, p = blockIdx.y;
  const int64_t plane = (int64_t)n * gridDim.y + p;
  const uint8_t* src = q + plane * HW;
  const float* in = img + (int64_t)n * 3 * HW;
  float* dst = out + (int64_t)n * 3 * HW;
  const bool blend = B.tiles_y > 0;
  const uint8_t* tables = lut + plane * (blend ? B.tiles_y * B.tiles_x : 1) * kBins;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const int v = src[i];
    int to;
    if (blend) {
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      int y1, y2, x1, x2;
      float ya1, ya, xa1, xa;
      axis_weights(y, B.inv_th, B.tiles_y, y1, y2, ya1, ya);
      axis_weights(x, B.inv_tw, B.tiles_x, x1, x2, xa1, xa);
      const float l11 = (float)tables[(y1 * B.tiles_x + x1) * kBins + v], l12 = (float)tables[(y1 * B.tiles_x + x2) * kBins + v];
      const float l21 = (float)tables[(y2 * B.tiles_x + x1) * kBins + v], l22 = (float)tables[(y2 * B.tiles_x + x2) * kBins + v];
      const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
      to = (int)fminf(fmaxf(rintf(res), 0.0f), 255.0f);
    } else {
      to = tables[v];
    }
    if (lab) {
      double L, ca, cb, r, g, b;
      srgb_to_lab((double)clip01(in[i]), (double)clip01(in[HW + i]), (double)clip01(in[2 * HW + i]), L, ca, cb);
      lab_to_srgb((double)to / 2.55, ca, cb, r, g, b);
      dst[i] = (float)fmin(fmax(r, 0.0), 1.0);
      dst[HW + i] = (float)fmin(fmax(g, 0.0), 1.0);
      dst[2 * HW + i] = (float)fmin(fmax(b, 0.0), 1.0);
    } else {
      dst[p * HW + i] = (float)((double)to / 255.0);
    }
  }
}

int check_tiles(const char* who, int H, int W, int tiles_y, int tiles_x) {
  HDIFF_CHECK_ARG(tiles_y >= 1 && tiles_y <= kMaxTiles && tiles_x >= 1 && tiles_x <= kMaxTiles,
                  "%s: grid = (%d, %d); each between 1 and %d", who, tiles_y, tiles_x, kMaxTiles);
  HDIFF_CHECK_ARG(H >= tiles_y && W >= tiles_x, "%s: H = %d, W = %d; at least one pixel per tile of the (%d, %d) grid", who, H, W,
                  tiles_y, tiles_x);
  return HDIFF_OK;
}

}  // namespace

extern "C" {

int hdiff_contrast_quantise(const float* img, int N, int H, int W, int lab, uint8_t* q, hdiff_stream_t stream) {
  const int rc = check_sizes("contrast_quantise", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(img && q, "contrast_quantise: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(quantise_kernel, dim3(parts_for(HW, kThreads * 4, 1024), lab ? 1 : 3, N), dim3(kThreads), 0, (hipStream_t)stream,
                     img, HW, lab != 0, q);
  HDIFF_CHECK_LAUNCH("contrast_quantise kernel");
  return HDIFF_OK;
}

int hdiff_clahe_luts(const uint8_t* q, int N, int planes, int H, int W, int tiles_y, int tiles_x, int64_t clip, float scale,
                     uint8_t* lut, hdiff_stream_t stream) {
  int rc = check_sizes("clahe_luts", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  rc = check_tiles("clahe_luts", H, W, tiles_y, tiles_x);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(planes == 1 || planes == 3, "clahe_luts: planes = %d; 3 (R, G, B) or 1 (L)", planes);
  const int th = cdiv(H, tiles_y), tw = cdiv(W, tiles_x);
  const int64_t area = (int64_t)th * tw;
  HDIFF_CHECK_ARG(clip >= 1 && clip <= area, "clahe_luts: clip = %lld; between 1 and the tile's %lld pixels (which clips nothing)",
                  (long long)clip, (long long)area);
  HDIFF_CHECK_ARG(scale > 0.0f && scale <= 255.0f, "clahe_luts: scale = %g; it is fp32(255) / fp32(tile area)", (double)scale);
  HDIFF_CHECK_ARG(q && lut, "clahe_luts: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(clahe_luts_kernel, dim3(tiles_y * tiles_x, planes, N), dim3(kThreads), 0, (hipStream_t)stream, q, H, W, tiles_x,
                     th, tw, (unsigned)clip, scale, lut);
  HDIFF_CHECK_LAUNCH("clahe_luts kernel");
  return HDIFF_OK;
}

int hdiff_equalize_luts_workspace(int N, int planes, int H, int W, int64_t* bytes) {
  const int rc = check_sizes("equalize_luts_workspace", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(planes == 1 || planes == 3, "equalize_luts_workspace: planes = %d; 3 (R, G, B) or 1 (L)", planes);
  HDIFF_CHECK_ARG(bytes, "equalize_luts_workspace: null pointer");
  Carver c(nullptr);
  c.take<unsigned>((int64_t)N * planes * parts_for((int64_t)H * W, kPerBlock, kMaxParts) * kBins);
  *bytes = c.total();
  return HDIFF_OK;
}

int hdiff_equalize_luts(const uint8_t* q, int N, int planes, int H, int W, uint8_t* lut, void* scratch, hdiff_stream_t stream) {
  const int rc = check_sizes("equalize_luts", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(planes == 1 || planes == 3, "equalize_luts: planes = %d; 3 (R, G, B) or 1 (L)", planes);
  HDIFF_CHECK_ARG(q && lut && scratch, "equalize_luts: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  const int parts = parts_for(HW, kPerBlock, kMaxParts);
  Carver c(scratch);
  unsigned* part = c.take<unsigned>((int64_t)N * planes * parts * kBins);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(equalize_hist_kernel, dim3(parts, planes, N), dim3(kThreads), 0, s, q, HW, part);
  hipLaunchKernelGGL(equalize_luts_kernel, dim3(1, planes, N), dim3(kThreads), 0, s, (const unsigned*)part, parts, HW, lut);
  HDIFF_CHECK_LAUNCH("equalize_luts kernels");
  return HDIFF_OK;
}

int hdiff_contrast_apply(const float* img, const uint8_t* q, const uint8_t* lut, int N, int H, int W, int lab, int tiles_y, int tiles_x,
                         float inv_th, float inv_tw, float* out, hdiff_stream_t stream) {
  int rc = check_sizes("contrast_apply", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  Blend B;
  B.tiles_y = tiles_y; B.tiles_x = tiles_x; B.inv_th = inv_th; B.inv_tw = inv_tw;
  if (tiles_y != 0 || tiles_x != 0) {
    rc = check_tiles("contrast_apply", H, W, tiles_y, tiles_x);
    if (rc != HDIFF_OK) return rc;
    HDIFF_CHECK_ARG(inv_th > 0.0f && inv_th <= 1.0f && inv_tw > 0.0f && inv_tw <= 1.0f,
                    "contrast_apply: inv_th = %g, inv_tw = %g; each is fp32(1) / fp32(tile side)", (double)inv_th, (double)inv_tw);
  }
  HDIFF_CHECK_ARG(img && q && lut && out && (const float*)out != img, "contrast_apply: null or aliased pointers");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(apply_kernel, dim3(parts_for(HW, kThreads * 4, 1024), lab ? 1 : 3, N), dim3(kThreads), 0, (hipStream_t)stream, img, q,
                     lut, HW, W, lab != 0, B, out);
  HDIFF_CHECK_LAUNCH("contrast_apply kernel");
  return HDIFF_OK;
}

}  // extern "C"
