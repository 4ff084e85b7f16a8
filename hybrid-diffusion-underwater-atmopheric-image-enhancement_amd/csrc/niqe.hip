// NIQE on the device (Mittal, Soundararajan, Bovik 2013, "Making a completely blind image quality analyzer"): the no-reference score of
// the atmospheric half of the project and of the full-size results, and the fit of its "pristine" model.  tests/_niqe_def.py is the
// float64 definition the kernels are held to; agreement with the authors' MATLAB release is unpinned (hdiff.h lists the deviations).
// Conventions are those of quality.hip and uciqe.hip: input fp32 [N][3][H][W] with nominal range [0, 1], images on blockIdx.z, grids
// functions of H, W and patch alone, everything in double, one row of 36 features per block of patch x patch pixels.
//
// hdiff_niqe_features, nine launches (ten while the table of the device is not built yet):
//   0. niqe_table_kernel   R(g) = G(2/g)^2 / (G(1/g) G(3/g)) for g = 0.2 + 0.001 k, k = 0 .. 9800, into a __device__ array: once per
//                          device (again in every call that is being captured: a captured launch does not run until it is replayed)
//   1. niqe_init_kernel    zeroes the per-image NaN flags
//   2. niqe_gray_kernel    the cropped gray plane in double (8-bit rounding of channels and gray with quantize); flags NaN pixels
//   per scale s = 1, 2 (block side p = patch / s):
//   3. niqe_mscn_kernel    mu and E[x^2] by the separable 7-tap window (rows, then columns, taps in ascending order, replicated edges)
//                          from an LDS-staged tile of 16 x 64 outputs; writes m = (x - mu) / (sigma + 1) and sigma
//   4. niqe_block_kernel   one workgroup per (block, image): the six sums of each of the five vectors (the block and its products with
//                          four copies of itself shifted circularly INSIDE the block), read from global memory (a 96 x 96 block in
//                          double does not fit a workgroup's LDS; it is L2-resident); five lanes search the table and write the 18
//                          features; at scale 1 it also sums sigma over the block (sharp) -- one slot per block, no atomics
//   5. niqe_half_kernel    after scale 1: the 8-tap bicubic reduction by two, rows then columns per output value
// This is the suggested launch list with the sharpness sum moved from the filter kernel into the block kernel, whose workgroups are the
// blocks (a filter tile straddles blocks), and with the init kernel.  hdiff_niqe_moments / hdiff_niqe_keep / hdiff_niqe_pool_moments are
// one launch each.  No float atomics, no allocation, no synchronisation.  Compiled with -ffp-contract=off: the per-pixel values (gray,
// mu, sigma, m, the reduced plane) round where the definition's separate double operations round and equal them bit for bit; what
// differs from numpy is the order of the per-block sums and the last bits of lgamma / exp.
#include <math.h>

#include "common.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kFeat = 18;                      // per scale
constexpr int kRow = 36;                       // a block's row: scale 1, then scale 2
constexpr int kOut = kRow + kRow * kRow + 1;   // mean, covariance, count
constexpr int kTable = 9801;
constexpr int kTileH = 16, kTileW = 64, kHalo = 3;
constexpr int kChunk = 64;                     // rows of the moments kernel staged at a time
constexpr int kMaxPixBlocks = 1024;

__device__ double g_table[kTable];

// exp(-x^2 / (2 (7/6)^2)), x = -3 .. 3, normalised to sum 1 (tests/test_niqe_cpu.py holds the definition's window to these literals)
__constant__ double kWin[7] = {0.012560200468474614, 0.07882796468173002, 0.2372960771171706, 0.34263151546524945,
                               0.2372960771171706, 0.07882796468173002, 0.012560200468474614};
// Keys' cubic (a = -0.5) at 3.5, 2.5, 1.5, 0.5 halves of a pixel on either side, normalised: exact binary fractions
__constant__ double kCubic[8] = {-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875};

struct NiqeWs {
  unsigned* flag;      // [N]
  double* gray;        // [N][Hc * Wc]
  double* half;        // [N][Hc / 2 * Wc / 2]
  double* mscn;        // [N][Hc * Wc]          (the scale-2 planes use the front of each image's region)
  double* sigma;       // [N][Hc * Wc]
};

__device__ __forceinline__ double table_gamma(int k) { return 0.2 + 0.001 * (double)k; }
__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(kThreads) void niqe_table_kernel() {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= kTable) return;
  const double g = table_gamma(k);
  g_table[k] = exp((2.0 * lgamma(2.0 / g) - lgamma(1.0 / g)) - lgamma(3.0 / g));
}

__global__ __launch_bounds__(kThreads) void niqe_init_kernel(unsigned* __restrict__ flag, int N) {
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < N; i += gridDim.x * kThreads) flag[i] = 0u;
}

__device__ __forceinline__ double clip01(float v) { return v != v ? (double)NAN : (double)fminf(fmaxf(v, 0.0f), 1.0f); }

__global__ __launch_bounds__(kThreads) void niqe_gray_kernel(const float* __restrict__ x, int H, int W, int Hc, int Wc, int quantize,
                                                              double* __restrict__ gray, unsigned* __restrict__ flag) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)H * W, K = (int64_t)Hc * Wc;
  const float* img = x + (int64_t)n * 3 * HW;
  double* out = gray + (int64_t)n * K;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < K; i += (int64_t)gridDim.x * kThreads) {
    const int64_t at = (i / Wc) * W + (i % Wc);
    double r = 255.0 * clip01(img[at]), g = 255.0 * clip01(img[HW + at]), b = 255.0 * clip01(img[2 * HW + at]);
    if (quantize) { r = floor(r + 0.5); g = floor(g + 0.5); b = floor(b + 0.5); }
    double v = (0.298936021293775 * r + 0.587043074451121 * g) + 0.114020904255103 * b;
    if (quantize) v = floor(v + 0.5);
    bad |= v != v;
    out[i] = v;
  }
  if (bad) flag[n] = 1u;
}

__global__ __launch_bounds__(kThreads) void niqe_mscn_kernel(const double* __restrict__ in, int Hs, int Ws, int64_t image_stride,
                                                              double* __restrict__ mscn, double* __restrict__ sigma) {
  constexpr int RH = kTileH + 2 * kHalo, RW = kTileW + 2 * kHalo;
  __shared__ double tile[RH][RW];
  __shared__ double hm[RH][kTileW];
  __shared__ double hs[RH][kTileW];
  const int n = blockIdx.z, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const double* src = in + (int64_t)n * image_stride;
  for (int i = threadIdx.x; i < RH * RW; i += kThreads) {
    const int r = i / RW, c = i % RW;
    const int y = min(max(y0 + r - kHalo, 0), Hs - 1), xx = min(max(x0 + c - kHalo, 0), Ws - 1);
    tile[r][c] = src[(int64_t)y * Ws + xx];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RH * kTileW; i += kThreads) {
    const int r = i / kTileW, c = i % kTileW;
    double a = 0.0, s = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double v = tile[r][c + k];
      a += kWin[k] * v;
      s += kWin[k] * (v * v);
    }
    hm[r][c] = a;
    hs[r][c] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kThreads) {
    const int r = i / kTileW, c = i % kTileW;
    const int y = y0 + r, xx = x0 + c;
    if (y >= Hs || xx >= Ws) continue;
    double mu = 0.0, ss = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      mu += kWin[k] * hm[r + k][c];
      ss += kWin[k] * hs[r + k][c];
    }
    const double sg = sqrt(fabs(ss - mu * mu));
    const int64_t at = (int64_t)n * image_stride + (int64_t)y * Ws + xx;
    mscn[at] = (tile[r + kHalo][c + kHalo] - mu) / (sg + 1.0);
    sigma[at] = sg;
  }
}

__global__ __launch_bounds__(kThreads) void niqe_half_kernel(const double* __restrict__ in, int Hs, int Ws, int64_t in_stride,
                                                              double* __restrict__ out, int64_t out_stride) {
  const int n = blockIdx.z, Ho = Hs / 2, Wo = Ws / 2;
  const double* src = in + (int64_t)n * in_stride;
  double* dst = out + (int64_t)n * out_stride;
  const int64_t K = (int64_t)Ho * Wo;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < K; i += (int64_t)gridDim.x * kThreads) {
    const int oy = (int)(i / Wo), ox = (int)(i % Wo);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const double* row = src + (int64_t)min(max(2 * oy - 3 + a, 0), Hs - 1) * Ws;
      double h = 0.0;
#pragma unroll
      for (int b = 0; b < 8; ++b) h += kCubic[b] * row[min(max(2 * ox - 3 + b, 0), Ws - 1)];
      acc += kCubic[a] * h;
    }
    dst[i] = acc;
  }
}

// GAM[argmin (R - rn)^2], the first minimum: R rises with k, so the minimum is one of the two entries around rn; NaN for a NaN rn
__device__ double table_alpha(double rn) {
  if (rn != rn) return (double)NAN;
  int lo = 0, hi = kTable - 1;                   // the largest k with R[k] <= rn, or 0
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g_table[mid] <= rn) lo = mid; else hi = mid - 1;
  }
  int k = lo;
  if (k + 1 < kTable) {
    const double d0 = g_table[k] - rn, d1 = g_table[k + 1] - rn;
    if (d1 * d1 < d0 * d0) k = k + 1;
  }
  return table_gamma(k);
}

__global__ __launch_bounds__(kThreads) void niqe_block_kernel(const double* __restrict__ mscn, const double* __restrict__ sigma,
                                                               int Ws, int64_t image_stride, int p, int bw, int P,
                                                               const unsigned* __restrict__ flag, double* __restrict__ feats,
                                                               double* __restrict__ sharp) {
  __shared__ double S[30];
  const int n = blockIdx.z, blk = blockIdx.x;
  const int by = blk / bw, bx = blk % bw;
  const double* b = mscn + (int64_t)n * image_stride + (int64_t)by * p * Ws + (int64_t)bx * p;
  double acc[30];
#pragma unroll
  for (int q = 0; q < 30; ++q) acc[q] = 0.0;
  double sg = 0.0;
  const int count = p * p;
  for (int idx = threadIdx.x; idx < count; idx += kThreads) {
    const int i = idx / p, j = idx % p;
    const int iu = i == 0 ? p - 1 : i - 1, jl = j == 0 ? p - 1 : j - 1, jr = j == p - 1 ? 0 : j + 1;
    const double c = b[(int64_t)i * Ws + j];
    const double* up = b + (int64_t)iu * Ws;
    const double v[5] = {c, c * b[(int64_t)i * Ws + jl], c * up[j], c * up[jl], c * up[jr]};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const double sq = v[q] * v[q];
      acc[6 * q] += fabs(v[q]);
      acc[6 * q + 1] += sq;
      if (v[q] < 0.0) { acc[6 * q + 2] += sq; acc[6 * q + 3] += 1.0; }
      if (v[q] > 0.0) { acc[6 * q + 4] += sq; acc[6 * q + 5] += 1.0; }
    }
    if (sharp) sg += sigma[(int64_t)n * image_stride + ((int64_t)by * p + i) * Ws + (int64_t)bx * p + j];
  }
#pragma unroll
  for (int q = 0; q < 30; ++q) {
    const double s = block_sum_all<kThreads>(acc[q]);
    if (threadIdx.x == 0) S[q] = s;
  }
  if (sharp) {
    const double s = block_sum_all<kThreads>(sg);
    if (threadIdx.x == 0) sharp[(int64_t)n * P + blk] = s / (double)count;
  }
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= 5) return;
  const double* s = S + 6 * q;
  const double ls = sqrt(s[2] / s[3]), rs = sqrt(s[4] / s[5]);
  const double mabs = s[0] / (double)count, msq = s[1] / (double)count;
  const double gh = ls / rs, rh = (mabs * mabs) / msq;
  const double rn = ((rh * (gh * gh * gh + 1.0)) * (gh + 1.0)) / ((gh * gh + 1.0) * (gh * gh + 1.0));
  double alpha = table_alpha(rn);
  const double g1 = lgamma(1.0 / alpha), g2 = lgamma(2.0 / alpha), g3 = lgamma(3.0 / alpha);
  const double c = sqrt(exp(g1 - g3));
  double bl = ls * c, br = rs * c;
  double mean = q == 0 ? (bl + br) / 2.0 : (br - bl) * exp(g2 - g1);
  if (flag[n]) alpha = mean = bl = br = (double)NAN;      // a NaN pixel anywhere: the image has no rows
  double* f = feats + ((int64_t)n * P + blk) * kRow;
  if (q == 0) {
    f[0] = alpha; f[1] = mean;
  } else {
    f += 2 + 4 * (q - 1);
    f[0] = alpha; f[1] = mean; f[2] = bl; f[3] = br;
  }
}

// ---------------------------------------------------------------------------------------------------------------- moments
__device__ double block_max(double v) {      // the largest non-NaN value, to every thread (-inf if there is none)
  __shared__ double part[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = part[0];
  for (int i = 1; i < kThreads / 64; ++i) r = fmax(r, part[i]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ bool row_finite(const double* __restrict__ f) {
  bool ok = true;
  for (int c = 0; c < kRow; ++c) ok = ok && finite64(f[c]);
  return ok;
}

// the cut a row's sharpness must exceed: threshold * max(sharp of the image); -inf (every finite row) without a threshold
__device__ double sharp_cut(const double* __restrict__ sharp, int P, double threshold) {
  if (!(threshold > 0.0)) return -INFINITY;
  double m = -INFINITY;
  for (int r = threadIdx.x; r < P; r += kThreads) m = fmax(m, sharp[r]);
  return threshold * block_max(m);
}

// grid (N): keep[n][r] = row r of image n is finite and sharper than the cut
__global__ __launch_bounds__(kThreads) void niqe_keep_kernel(const double* __restrict__ feats, const double* __restrict__ sharp, int P,
                                                              double threshold, int* __restrict__ keep) {
  const int n = blockIdx.x;
  const double* sh = sharp ? sharp + (int64_t)n * P : nullptr;
  const double cut = sharp_cut(sh, P, sh ? threshold : 0.0);
  for (int r = threadIdx.x; r < P; r += kThreads)
    keep[(int64_t)n * P + r] = row_finite(feats + ((int64_t)n * P + r) * kRow) && (!sh || !(threshold > 0.0) || sh[r] > cut);
}

// grid (N): out[n] = {mean[36], cov[36][36], count} of the valid rows of image n, rows added in index order: the rows are staged
// kChunk at a time; thread c < 36 adds column c of the chunk's valid rows, then (second pass) every thread adds its entries of the
// covariance.  keep != null: validity is keep[n][r] (the pool: N = 1, P = the rows of the bank); otherwise it is computed here.
__global__ __launch_bounds__(kThreads) void niqe_moments_kernel(const double* __restrict__ feats, const double* __restrict__ sharp,
                                                                 const int* __restrict__ keep, int P, double threshold,
                                                                 double* __restrict__ out) {
  __shared__ double rows[kChunk][kRow];
  __shared__ int ok[kChunk];
  __shared__ double mean[kRow];
  __shared__ double total;
  const int n = blockIdx.x, tid = threadIdx.x;
  const double* f = feats + (int64_t)n * P * kRow;
  const double* sh = (!keep && sharp) ? sharp + (int64_t)n * P : nullptr;
  const bool cutting = sh && threshold > 0.0;
  const double cut = sharp_cut(sh, P, cutting ? threshold : 0.0);
  constexpr int kPer = (kRow * kRow + kThreads - 1) / kThreads;
  double acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) acc[e] = 0.0;
  double colsum = 0.0, cnt = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int base = 0; base < P; base += kChunk) {
      const int rows_here = min(kChunk, P - base);
      if (tid < rows_here) {
        const int r = base + tid;
        ok[tid] = keep ? keep[(int64_t)n * P + r] != 0 : (row_finite(f + (int64_t)r * kRow) && (!cutting || sh[r] > cut));
      }
      __syncthreads();
      for (int i = tid; i < rows_here * kRow; i += kThreads) {
        const int r = i / kRow, c = i % kRow;
        const double v = ok[r] ? f[(int64_t)(base + r) * kRow + c] : 0.0;
        rows[r][c] = pass == 0 ? v : v - mean[c];
      }
      __syncthreads();
      if (pass == 0) {
        if (tid < kRow) {
          for (int r = 0; r < rows_here; ++r)
            if (ok[r]) { colsum += rows[r][tid]; if (tid == 0) cnt += 1.0; }
        }
      } else {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
          const int at = tid + e * kThreads;
          if (at < kRow * kRow) {
            const int i = at / kRow, j = at % kRow;
            for (int r = 0; r < rows_here; ++r)
              if (ok[r]) acc[e] += rows[r][i] * rows[r][j];
          }
        }
      }
      __syncthreads();
    }
    if (pass == 0) {
      if (tid == 0) total = cnt;
      __syncthreads();
      if (tid < kRow) mean[tid] = colsum / total;      // no valid row: 0 / 0
      __syncthreads();
    }
  }
  double* o = out + (int64_t)n * kOut;
  const double count = total;
  if (tid < kRow) o[tid] = mean[tid];
  if (tid == 0) o[kOut - 1] = count;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int at = tid + e * kThreads;
    if (at < kRow * kRow) o[kRow + at] = count >= 2.0 ? acc[e] / (count - 1.0) : (double)NAN;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct Geometry { int bh, bw, Hc, Wc, P; int64_t K; };

Geometry geometry(int H, int W, int patch) {
  Geometry g;
  g.bh = H / patch; g.bw = W / patch;
  g.Hc = g.bh * patch; g.Wc = g.bw * patch;
  g.P = g.bh * g.bw;
  g.K = (int64_t)g.Hc * g.Wc;
  return g;
}

int64_t niqe_layout(void* base, int N, const Geometry& g, NiqeWs* ws) {
  Carver c(base);
  ws->flag = c.take<unsigned>(N);
  ws->gray = c.take<double>((int64_t)N * g.K);
  ws->half = c.take<double>((int64_t)N * (g.K / 4));
  ws->mscn = c.take<double>((int64_t)N * g.K);
  ws->sigma = c.take<double>((int64_t)N * g.K);
  return c.total();
}

int check_niqe(const char* who, int N, int H, int W, int patch) {
  HDIFF_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d; between 1 and 65535 images", who, N);
  HDIFF_CHECK_ARG(patch >= 8 && patch <= 512 && patch % 2 == 0, "%s: patch = %d; an even block side between 8 and 512", who, patch);
  HDIFF_CHECK_ARG(H >= patch && W >= patch, "%s: H = %d, W = %d; both sides must be at least patch = %d", who, H, W, patch);
  HDIFF_CHECK_ARG(H <= 16384 && W <= 16384, "%s: H = %d, W = %d is too large; sides of at most 16384", who, H, W);
  return HDIFF_OK;
}

int check_rows(const char* who, int N, int P) {
  HDIFF_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d; between 1 and 65535 images", who, N);
  HDIFF_CHECK_ARG(P >= 1 && P <= (1 << 22), "%s: P = %d; between 1 and 2^22 rows per image", who, P);
  return HDIFF_OK;
}

bool threshold_ok(double t) { return t >= 0.0 && t < 1.0; }

}  // namespace

extern "C" {

int hdiff_niqe_workspace(int N, int H, int W, int patch, int64_t* bytes) {
  const int rc = check_niqe("niqe_workspace", N, H, W, patch);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "niqe_workspace: null pointer");
  NiqeWs ws;
  *bytes = niqe_layout(nullptr, N, geometry(H, W, patch), &ws);
  return HDIFF_OK;
}

int hdiff_niqe_features(const float* img, int N, int H, int W, int patch, int quantize, double* feats, double* sharp, void* scratch,
                        hdiff_stream_t stream) {
  const int rc = check_niqe("niqe_features", N, H, W, patch);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(img && feats && sharp && scratch, "niqe_features: null pointer");
  (void)hipGetLastError();
  const Geometry g = geometry(H, W, patch);
  NiqeWs ws;
  niqe_layout(scratch, N, g, &ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads);
  static uint64_t table_built = 0;
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capturing) != hipSuccess) capturing = hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  // a captured launch runs at replay only: it must not count as having built the table
  if (capturing != hipStreamCaptureStatusNone || first_use_on_device(table_built))
    hipLaunchKernelGGL(niqe_table_kernel, dim3(cdiv(kTable, kThreads)), blk, 0, s);
  hipLaunchKernelGGL(niqe_init_kernel, dim3(cdiv(N, kThreads)), blk, 0, s, ws.flag, N);
  hipLaunchKernelGGL(niqe_gray_kernel, dim3(parts_for(g.K, kThreads * 4, kMaxPixBlocks), 1, N), blk, 0, s, img, H, W, g.Hc, g.Wc,
                     quantize ? 1 : 0, ws.gray, ws.flag);
  const double* plane = ws.gray;
  int Hs = g.Hc, Ws = g.Wc, p = patch;
  int64_t stride = g.K;
  for (int scale = 0; scale < 2; ++scale) {
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3(cdiv(Ws, kTileW), cdiv(Hs, kTileH), N), blk, 0, s, plane, Hs, Ws, stride, ws.mscn,
                       ws.sigma);
    hipLaunchKernelGGL(niqe_block_kernel, dim3(g.P, 1, N), blk, 0, s, (const double*)ws.mscn, (const double*)ws.sigma, Ws, stride, p,
                       g.bw, g.P, (const unsigned*)ws.flag, feats + scale * kFeat, scale == 0 ? sharp : (double*)nullptr);
    if (scale == 0) {
      hipLaunchKernelGGL(niqe_half_kernel, dim3(parts_for(g.K / 4, kThreads * 4, kMaxPixBlocks), 1, N), blk, 0, s, plane, Hs, Ws,
                         stride, ws.half, g.K / 4);
      plane = ws.half;
      Hs /= 2; Ws /= 2; p /= 2; stride = g.K / 4;
    }
  }
  HDIFF_CHECK_LAUNCH("niqe_features kernels");
  return HDIFF_OK;
}

int hdiff_niqe_moments(const double* feats, const double* sharp, int N, int P, double sharp_threshold, double* out,
                       hdiff_stream_t stream) {
  const int rc = check_rows("niqe_moments", N, P);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(threshold_ok(sharp_threshold), "niqe_moments: sharp_threshold = %g; in [0, 1), 0 keeps every finite row",
                  sharp_threshold);
  HDIFF_CHECK_ARG(feats && out && (sharp || sharp_threshold == 0.0), "niqe_moments: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(niqe_moments_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, feats, sharp, (const int*)nullptr, P,
                     sharp_threshold, out);
  HDIFF_CHECK_LAUNCH("niqe_moments kernel");
  return HDIFF_OK;
}

int hdiff_niqe_keep(const double* feats, const double* sharp, int N, int P, double sharp_threshold, int* keep, hdiff_stream_t stream) {
  const int rc = check_rows("niqe_keep", N, P);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(threshold_ok(sharp_threshold), "niqe_keep: sharp_threshold = %g; in [0, 1), 0 keeps every finite row",
                  sharp_threshold);
  HDIFF_CHECK_ARG(feats && keep && (sharp || sharp_threshold == 0.0), "niqe_keep: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(niqe_keep_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, feats, sharp, P, sharp_threshold, keep);
  HDIFF_CHECK_LAUNCH("niqe_keep kernel");
  return HDIFF_OK;
}

int hdiff_niqe_pool_moments(const double* feats, const int* keep, int rows, double* out, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(rows >= 1 && rows <= (1 << 26), "niqe_pool_moments: rows = %d; between 1 and 2^26", rows);
  HDIFF_CHECK_ARG(feats && keep && out, "niqe_pool_moments: null pointer");
  (void)hipGetLastError();
  hipLaunchKernelGGL(niqe_moments_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, feats, (const double*)nullptr, keep, rows,
                     0.0, out);
  HDIFF_CHECK_LAUNCH("niqe_pool_moments kernel");
  return HDIFF_OK;
}

}  // extern "C"
