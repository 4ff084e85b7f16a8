// Classical baselines on the device: He, Sun and Tang's dark-channel prior (DCP), the underwater variant of Drews et al. (UDCP, the
// prior over G and B alone), Dong et al.'s inverted-image form for low light, and gray-world / shades-of-gray white balance -- the
// methods dehazing, underwater and low-light work reports beside its scores, and the classical inverses of the degradation
// synth_degrade.hip draws (tests/_classical_def.py is the definition the kernels are held to; hdiff_amd/classical.py is the caller and
// composes the passes).  Conventions are those of the score kernels (color_diff.hip): images fp32 [N][3][H][W] with nominal range
// [0, 1], images on blockIdx.z, grids and partial counts functions of H and W alone.
//
// Every kernel reads X_c = min(max(I_c, 0), 1) in fp32 (a NaN clips to 0), or fp32(1 - that) with `invert`.
//   hdiff_classical_point_min   one launch: min over the channel set of X_c, or of fp32(double(X_c) / double(A_c))
//   hdiff_classical_window_min  one launch: the (2 r + 1)^2 minimum of a plane, clipped at the border.  A workgroup owns a kTile x kTile
//                               block of outputs: it stages the block with its halo of r in LDS (+inf outside the image), takes the row
//                               minima into a second LDS array, then the column minima of those.  A minimum is exact: the result does
//                               not depend on the order.  With `affine` the store is fp32(1 - omega double(min)).
//   hdiff_classical_airlight    nine launches: init; three digits (11 / 11 / 10 bits) of the radix select of the cut on the fp32 key of
//                               the dark channel (radix_select.h; integer LDS atomics merged with integer global atomics); the best
//                               candidate of every workgroup; the best of those.  "Best" is a total order -- larger sum, then lower
//                               index -- so neither reduction depends on arrival order.
//   hdiff_classical_recover     one launch: the scene radiance, one rounding
//   hdiff_white_balance         three launches: per-workgroup double sums of X^p (or maxima), the gains, the scaled image
// No float atomics, no allocation, no synchronisation.  Compiled with -ffp-contract=off: every value rounds where the definition's
// separately written operation rounds.
#include <math.h>

#include "common.h"
#include "radix_select.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 2048;
constexpr int kPasses = 3;
constexpr int kTile = 32;                      // the window minimum: outputs per workgroup and side
constexpr int kMaxR = 31;                      // patch <= 63
constexpr int kSpan = kTile + 2 * kMaxR;       // the staged block's side at the largest patch
constexpr int kMaxParts = 256;                 // the reductions: one partial per workgroup, eight pixels per thread
constexpr int kPerBlock = kThreads * 8;

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float read01(const float* __restrict__ p, int64_t i, int invert) {
  const float v = clip01(p[i]);
  return invert ? 1.0f - v : v;
}

// ---------------------------------------------------------------------------------------------------------------- pointwise minimum
__global__ __launch_bounds__(kThreads) void point_min_kernel(const float* __restrict__ img, int64_t HW, int first, int invert,
                                                              const float* __restrict__ airlight, float* __restrict__ out) {
  const int n = blockIdx.z;
  const float* p = img + (int64_t)n * 3 * HW;
  float* o = out + (int64_t)n * HW;
  double a[3] = {1.0, 1.0, 1.0};
  if (airlight)
    for (int c = 0; c < 3; ++c) a[c] = (double)airlight[n * 3 + c];
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    float m = INFINITY;
    for (int c = first; c < 3; ++c) {
      const float x = read01(p, c * HW + i, invert);
      m = fminf(m, airlight ? (float)((double)x / a[c]) : x);
    }
    o[i] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------------- windowed minimum
// grid (ceil(W / kTile), ceil(H / kTile), N).  Every global read and write is guarded by 0 <= y < H, 0 <= x < W; the LDS indices stay
// below (kTile + 2 r)^2 <= kSpan^2 and (kTile + 2 r) kTile <= kSpan kTile.
__global__ __launch_bounds__(kThreads) void window_min_kernel(const float* __restrict__ in, int H, int W, int r, int affine,
                                                               double omega, float* __restrict__ out) {
  __shared__ float a[kSpan * kSpan];
  __shared__ float b[kSpan * kTile];
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)H * W;
  const float* src = in + (int64_t)n * HW;
  float* dst = out + (int64_t)n * HW;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const int span = kTile + 2 * r;
  for (int i = threadIdx.x; i < span * span; i += kThreads) {
    const int ly = i / span, lx = i - ly * span;
    const int y = y0 - r + ly, x = x0 - r + lx;
    a[i] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(int64_t)y * W + x] : INFINITY;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < span * kTile; i += kThreads) {
    const int ly = i / kTile, lx = i - ly * kTile;
    const float* row = a + ly * span + lx;
    float m = row[0];
    for (int k = 1; k <= 2 * r; ++k) m = fminf(m, row[k]);
    b[i] = m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTile * kTile; i += kThreads) {
    const int ly = i / kTile, lx = i - ly * kTile;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const float* col = b + ly * kTile + lx;
    float m = col[0];
    for (int k = 1; k <= 2 * r; ++k) m = fminf(m, col[k * kTile]);
    dst[(int64_t)y * W + x] = affine ? (float)(1.0 - omega * (double)m) : m;
  }
}

// ---------------------------------------------------------------------------------------------------------------- airlight
using Cut = Select<unsigned>;

struct Best { double sum; unsigned idx; unsigned pad; };      // sum < 0: no candidate

struct AirWs {
  unsigned* hist;      // [kPasses][N][kBins]
  Cut* sel;            // [N]
  Best* best;          // [N][parts]
};

struct AirParams {
  int N, H, W, parts, invert;
  unsigned rank;
};

__device__ __forceinline__ bool better(double s, unsigned i, double s2, unsigned i2) { return s > s2 || (s == s2 && i < i2); }

// the best (sum, index) of the workgroup, to thread 0
__device__ __forceinline__ void block_best(double& s, unsigned& idx) {
  __shared__ double ss[kThreads];
  __shared__ unsigned si[kThreads];
  ss[threadIdx.x] = s;
  si[threadIdx.x] = idx;
  __syncthreads();
  for (int step = kThreads / 2; step >= 1; step >>= 1) {
    if ((int)threadIdx.x < step && better(ss[threadIdx.x + step], si[threadIdx.x + step], ss[threadIdx.x], si[threadIdx.x])) {
      ss[threadIdx.x] = ss[threadIdx.x + step];
      si[threadIdx.x] = si[threadIdx.x + step];
    }
    __syncthreads();
  }
  s = ss[0];
  idx = si[0];
}

__global__ __launch_bounds__(kThreads) void air_init_kernel(const AirParams P, const AirWs ws) {
  const int64_t nh = (int64_t)kPasses * P.N * kBins;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nh; i += (int64_t)gridDim.x * kThreads) ws.hist[i] = 0u;
  if (blockIdx.x != 0) return;
  for (int i = threadIdx.x; i < P.N; i += kThreads) ws.sel[i] = select_start<unsigned>(P.rank);
}

// One digit of the select: counts the pixels whose key agrees with the select's prefix above `match_shift` (match_shift == 32: every
// pixel), binned by the `bits` bits below it.
__global__ __launch_bounds__(kThreads) void air_hist_kernel(const AirParams P, const AirWs ws, const float* __restrict__ dark, int pass,
                                                             int match_shift, int bits) {
  __shared__ unsigned sh[kBins];
  const int n = blockIdx.z;
  for (int i = threadIdx.x; i < kBins; i += kThreads) sh[i] = 0u;
  const unsigned prefix = ws.sel[n].prefix;
  __syncthreads();
  const int64_t HW = (int64_t)P.H * P.W;
  const float* plane = dark + (int64_t)n * HW;
  const int bin_shift = match_shift - bits;
  const unsigned mask = (1u << bits) - 1u;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const unsigned k = key_of(plane[i]);
    const unsigned bin = (k >> bin_shift) & mask;
    if (match_shift == 32 || (k >> match_shift) == prefix) atomicAdd(&sh[bin], 1u);
  }
  select_flush<kThreads>(sh, ws.hist + ((int64_t)pass * P.N + n) * kBins, kBins);
}

__global__ __launch_bounds__(kThreads) void air_scan_kernel(const AirParams P, const AirWs ws, int pass, int bits) {
  const int n = blockIdx.z;
  select_scan<kThreads, kBins>(ws.hist + ((int64_t)pass * P.N + n) * kBins, &ws.sel[n], bits);
}

__global__ __launch_bounds__(kThreads) void air_candidate_kernel(const AirParams P, const AirWs ws, const float* __restrict__ img,
                                                                  const float* __restrict__ dark) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)P.H * P.W;
  const float* p = img + (int64_t)n * 3 * HW;
  const float* plane = dark + (int64_t)n * HW;
  const unsigned cut = ws.sel[n].prefix;
  double s = -1.0;
  unsigned idx = 0xffffffffu;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    if (key_of(plane[i]) < cut) continue;
    const double v = ((double)read01(p, i, P.invert) + (double)read01(p, HW + i, P.invert)) + (double)read01(p, 2 * HW + i, P.invert);
    if (better(v, (unsigned)i, s, idx)) {
      s = v;
      idx = (unsigned)i;
    }
  }
  block_best(s, idx);
  if (threadIdx.x == 0) {
    Best o;
    o.sum = s; o.idx = idx; o.pad = 0u;
    ws.best[(int64_t)n * P.parts + blockIdx.x] = o;
  }
}

// grid (N): the best of the workgroups' candidates (P.parts <= kMaxParts = kThreads).  The pixel at the cut's own rank is a candidate, so
// there is always one.
__global__ __launch_bounds__(kThreads) void air_pick_kernel(const AirParams P, const AirWs ws, const float* __restrict__ img,
                                                             float* __restrict__ airlight, float* __restrict__ cut) {
  const int n = blockIdx.x;
  double s = -1.0;
  unsigned idx = 0xffffffffu;
  if ((int)threadIdx.x < P.parts) {
    const Best b = ws.best[(int64_t)n * P.parts + threadIdx.x];
    s = b.sum;
    idx = b.idx;
  }
  block_best(s, idx);
  if (threadIdx.x != 0) return;
  const int64_t HW = (int64_t)P.H * P.W;
  cut[n] = value_of(ws.sel[n].prefix);
  if (idx >= (unsigned)HW) idx = 0u;      // unreachable for finite `dark`; keeps the read inside the image whatever the plane holds
  const float* p = img + (int64_t)n * 3 * HW;
  for (int c = 0; c < 3; ++c) airlight[n * 3 + c] = fmaxf(read01(p, c * HW + idx, P.invert), (float)(1.0 / 255.0));
}

int64_t air_layout(void* base, int N, int parts, AirWs* ws) {
  Carver c(base);
  ws->hist = c.take<unsigned>((int64_t)kPasses * N * kBins);
  ws->sel = c.take<Cut>(N);
  ws->best = c.take<Best>((int64_t)N * parts);
  return c.total();
}

// ---------------------------------------------------------------------------------------------------------------- recovery
__global__ __launch_bounds__(kThreads) void recover_kernel(const float* __restrict__ img, const float* __restrict__ t,
                                                            const float* __restrict__ airlight, int64_t HW, int invert, double t0,
                                                            float* __restrict__ out) {
  const int n = blockIdx.z, c = blockIdx.y;
  const float* p = img + ((int64_t)n * 3 + c) * HW;
  const float* tp = t + (int64_t)n * HW;
  float* o = out + ((int64_t)n * 3 + c) * HW;
  const double a = (double)airlight[n * 3 + c];
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const double x = (double)read01(p, i, invert);
    const double j = ((x - a) / fmax((double)tp[i], t0)) + a;
    const float v = (float)fmin(fmax(j, 0.0), 1.0);
    o[i] = invert ? 1.0f - v : v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- white balance
// the maximum of the workgroup's values, to every thread (values >= 0)
__device__ __forceinline__ double block_max_all(double v) {
  __shared__ double mm[kThreads];
  mm[threadIdx.x] = v;
  __syncthreads();
  for (int step = kThreads / 2; step >= 1; step >>= 1) {
    if ((int)threadIdx.x < step) mm[threadIdx.x] = fmax(mm[threadIdx.x], mm[threadIdx.x + step]);
    __syncthreads();
  }
  const double r = mm[0];
  __syncthreads();
  return r;
}

// grid (parts, 3, N) -> part[n][c][block]: the sum of double(X)^p over the workgroup's pixels, or their maximum at p = inf
__global__ __launch_bounds__(kThreads) void wb_partial_kernel(const float* __restrict__ img, int64_t HW, int parts, double p,
                                                               double* __restrict__ part) {
  const int n = blockIdx.z, c = blockIdx.y;
  const float* src = img + ((int64_t)n * 3 + c) * HW;
  const bool is_max = isinf(p), plain = p == 1.0;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const double v = (double)clip01(src[i]);
    if (is_max) acc = fmax(acc, v);
    else acc += plain ? v : pow(v, p);
  }
  const double total = is_max ? block_max_all(acc) : block_sum_all<kThreads>(acc);
  if (threadIdx.x == 0) part[((int64_t)n * 3 + c) * parts + blockIdx.x] = total;
}

// grid (N) -> gains[n][3]
__global__ __launch_bounds__(kThreads) void wb_gain_kernel(const double* __restrict__ part, int64_t HW, int parts, double p,
                                                            double* __restrict__ gains) {
  const int n = blockIdx.x;
  const bool is_max = isinf(p);
  double m[3];
  for (int c = 0; c < 3; ++c) {
    const double* q = part + ((int64_t)n * 3 + c) * parts;
    if (is_max) {
      m[c] = block_max_all((int)threadIdx.x < parts ? q[threadIdx.x] : 0.0);
    } else {
      const double mean = sum_partials<kThreads>(q, parts, 1) / (double)HW;
      m[c] = p == 1.0 ? mean : pow(mean, 1.0 / p);
    }
  }
  if (threadIdx.x != 0) return;
  const double gray = ((m[0] + m[1]) + m[2]) / 3.0;
  for (int c = 0; c < 3; ++c) gains[n * 3 + c] = gray / fmax(m[c], 1e-6);
}

__global__ __launch_bounds__(kThreads) void wb_apply_kernel(const float* __restrict__ img, int64_t HW, const double* __restrict__ gains,
                                                             float* __restrict__ out) {
  const int n = blockIdx.z, c = blockIdx.y;
  const float* src = img + ((int64_t)n * 3 + c) * HW;
  float* o = out + ((int64_t)n * 3 + c) * HW;
  const double g = gains[n * 3 + c];
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads)
    o[i] = (float)fmin(fmax((double)clip01(src[i]) * g, 0.0), 1.0);
}

}  // namespace

extern "C" {

int hdiff_classical_point_min(const float* img, int N, int H, int W, int channels, int invert, const float* airlight, float* out,
                              hdiff_stream_t stream) {
  const int rc = check_sizes("classical_point_min", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(channels == 3 || channels == 2, "classical_point_min: channels = %d; 3 (R, G, B) or 2 (G, B)", channels);
  HDIFF_CHECK_ARG(img && out, "classical_point_min: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(point_min_kernel, dim3(parts_for(HW, kThreads * 2, 1024), 1, N), dim3(kThreads), 0, (hipStream_t)stream, img, HW,
                     3 - channels, invert != 0, airlight, out);
  HDIFF_CHECK_LAUNCH("classical_point_min kernel");
  return HDIFF_OK;
}

int hdiff_classical_window_min(const float* in, int N, int H, int W, int patch, int affine, double omega, float* out,
                               hdiff_stream_t stream) {
  const int rc = check_sizes("classical_window_min", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(patch >= 1 && patch <= 2 * kMaxR + 1 && (patch & 1), "classical_window_min: patch = %d; odd, between 1 and %d", patch,
                  2 * kMaxR + 1);
  HDIFF_CHECK_ARG(cdiv(H, kTile) <= 65535, "classical_window_min: H = %d; at most %d rows", H, 65535 * kTile);
  HDIFF_CHECK_ARG(in && out && in != out, "classical_window_min: null or aliased pointers");
  HDIFF_CHECK_ARG(!affine || (omega == omega && fabs(omega) <= 1e300), "classical_window_min: omega must be finite");
  (void)hipGetLastError();
  hipLaunchKernelGGL(window_min_kernel, dim3(cdiv(W, kTile), cdiv(H, kTile), N), dim3(kThreads), 0, (hipStream_t)stream, in, H, W,
                     patch / 2, affine != 0, omega, out);
  HDIFF_CHECK_LAUNCH("classical_window_min kernel");
  return HDIFF_OK;
}

int hdiff_classical_airlight_workspace(int N, int H, int W, int64_t* bytes) {
  const int rc = check_sizes("classical_airlight_workspace", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "classical_airlight_workspace: null pointer");
  AirWs ws;
  *bytes = air_layout(nullptr, N, parts_for((int64_t)H * W, kPerBlock, kMaxParts), &ws);
  return HDIFF_OK;
}

int hdiff_classical_airlight(const float* img, const float* dark, int N, int H, int W, int invert, int64_t n_top, float* airlight,
                             float* cut, void* scratch, hdiff_stream_t stream) {
  const int rc = check_sizes("classical_airlight", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  const int64_t HW = (int64_t)H * W;
  HDIFF_CHECK_ARG(n_top >= 1 && n_top <= HW, "classical_airlight: n_top = %lld; between 1 and H W = %lld", (long long)n_top,
                  (long long)HW);
  HDIFF_CHECK_ARG(img && dark && airlight && cut && scratch, "classical_airlight: null pointer");
  (void)hipGetLastError();
  AirParams P;
  P.N = N; P.H = H; P.W = W; P.invert = invert != 0;
  P.parts = parts_for(HW, kPerBlock, kMaxParts);
  P.rank = (unsigned)(HW - n_top);
  AirWs ws;
  air_layout(scratch, N, P.parts, &ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads), grid(P.parts, 1, N);
  const int64_t nh = (int64_t)kPasses * N * kBins;
  hipLaunchKernelGGL(air_init_kernel, dim3((int)(nh / kThreads > 1024 ? 1024 : nh / kThreads)), blk, 0, s, P, ws);
  const int bits[kPasses] = {11, 11, 10};
  int shift = 32;
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(air_hist_kernel, grid, blk, 0, s, P, ws, dark, pass, shift, bits[pass]);
    hipLaunchKernelGGL(air_scan_kernel, dim3(1, 1, N), blk, 0, s, P, ws, pass, bits[pass]);
    shift -= bits[pass];
  }
  hipLaunchKernelGGL(air_candidate_kernel, grid, blk, 0, s, P, ws, img, dark);
  hipLaunchKernelGGL(air_pick_kernel, dim3(N), blk, 0, s, P, ws, img, airlight, cut);
  HDIFF_CHECK_LAUNCH("classical_airlight kernels");
  return HDIFF_OK;
}

int hdiff_classical_recover(const float* img, const float* t, const float* airlight, int N, int H, int W, int invert, double t0,
                            float* out, hdiff_stream_t stream) {
  const int rc = check_sizes("classical_recover", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(t0 > 0.0 && t0 <= 1e300, "classical_recover: t0 = %g; it must be finite and positive", t0);
  HDIFF_CHECK_ARG(img && t && airlight && out, "classical_recover: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(recover_kernel, dim3(parts_for(HW, kThreads * 2, 1024), 3, N), dim3(kThreads), 0, (hipStream_t)stream, img, t,
                     airlight, HW, invert != 0, t0, out);
  HDIFF_CHECK_LAUNCH("classical_recover kernel");
  return HDIFF_OK;
}

int hdiff_white_balance_workspace(int N, int H, int W, int64_t* bytes) {
  const int rc = check_sizes("white_balance_workspace", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "white_balance_workspace: null pointer");
  Carver c(nullptr);
  c.take<double>((int64_t)N * 3 * parts_for((int64_t)H * W, kPerBlock, kMaxParts));
  *bytes = c.total();
  return HDIFF_OK;
}

int hdiff_white_balance(const float* img, int N, int H, int W, double p, double* gains, float* out, void* scratch,
                        hdiff_stream_t stream) {
  const int rc = check_sizes("white_balance", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(p >= 1.0, "white_balance: p = %g; at least 1 (inf: the maximum)", p);
  HDIFF_CHECK_ARG(img && gains && out && scratch, "white_balance: null pointer");
  (void)hipGetLastError();
  const int64_t HW = (int64_t)H * W;
  const int parts = parts_for(HW, kPerBlock, kMaxParts);
  Carver c(scratch);
  double* part = c.take<double>((int64_t)N * 3 * parts);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads);
  hipLaunchKernelGGL(wb_partial_kernel, dim3(parts, 3, N), blk, 0, s, img, HW, parts, p, part);
  hipLaunchKernelGGL(wb_gain_kernel, dim3(N), blk, 0, s, (const double*)part, HW, parts, p, gains);
  hipLaunchKernelGGL(wb_apply_kernel, dim3(parts_for(HW, kThreads * 2, 1024), 3, N), blk, 0, s, img, HW, (const double*)gains, out);
  HDIFF_CHECK_LAUNCH("white_balance kernels");
  return HDIFF_OK;
}

}  // extern "C"
