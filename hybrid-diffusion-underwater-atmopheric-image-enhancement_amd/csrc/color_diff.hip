// Colour difference between a prediction and its target on the device: CIEDE2000, CIE76 and the angular error, the scores dehazing,
// low-light and underwater colour-restoration work reports beside PSNR and SSIM (tests/_color_def.py is the definition the kernels are
// held to; tests/golden/ciede2000_sharma.json pins the formula to the published table of Sharma, Wu and Dalal 2005).  Conventions are
// those of quality.hip and uciqe.hip: inputs fp32 [N][3][H][W] with nominal range [0, 1], images on blockIdx.z, grids and partial
// counts functions of H and W alone, outputs float64, one row per image.
//
// Per pixel, in double: rgb = double(min(max(x, 0), 1)) (the clip in fp32), sRGB -> CIE L*a*b* (lab.h) for both images, then
//   de76  = sqrt(dL^2 + da^2 + db^2)
//   de00  = CIEDE2000 with kL = kC = kH = 1 (ciede2000 below, every operation in the definition's order)
//   angle = atan2(|u x v|, u . v) * (180 / pi) on the clipped RGB vectors; the pixel counts when neither vector is black
// Per image: de00 = mean(de00), de00_p95 = the nearest-rank 95th percentile of de00 (rank (95 n + 99) / 100 - 1 of the ascending
// sort), de76 = mean(de76), angular = mean of angle over the counted pixels (NaN when there are none).
//
// hdiff_color_diff, fifteen launches:
//   1. color_init_kernel      zeroes the histograms and flags, sets the select of every image
//   2. color_pixel_kernel     both conversions, the three per-pixel values; keeps the de00 plane as doubles in the scratch (and, when
//                             asked, rounded once to fp32 in `map`); per-workgroup double sums and the integer count; the non-finite flag
//   3-14. color_hist_kernel + color_scan_kernel, six times (11 / 11 / 11 / 11 / 10 / 10 bits): radix select of the percentile on the
//                             order-preserving 64-bit key of the double (radix_select.h; de00 is never negative, -0 and +0 share a key
//                             all the same).  Integer LDS atomics per workgroup, merged with integer global atomics.
//  15. color_finalize_kernel  grid (N): adds the partials in index order; the four scores
// No float atomics, no allocation, no synchronisation.  Compiled with -ffp-contract=off: identical images give exactly 0.
#include <math.h>

#include "common.h"
#include "lab.h"
#include "radix_select.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 2048;
constexpr int kPasses = 6;
constexpr int kMaxPixBlocks = 1024;            // the pixel kernel: arithmetic-bound, two pixels per thread
constexpr int kPixPerBlock = kThreads * 2;
constexpr int kMaxHistBlocks = 256;            // the histogram kernels: one LDS histogram per workgroup to flush, as in uciqe.hip
constexpr int kHistPerBlock = kThreads * 8;

constexpr double kPi = 3.141592653589793;
constexpr double kR2D = 180.0 / kPi;
constexpr double kD2R = kPi / 180.0;
constexpr double kPow25_7 = 6103515625.0;

// ---------------------------------------------------------------------------------------------------------------- the hue angle
// atan2 rounded correctly (in all but astronomically rare cases), evaluated in double-double arithmetic.  The hue rules of CIEDE2000
// branch at |h1' - h2'| = 180 degrees exactly, and colours with exactly opposite chroma vectors sit ON that branch -- the published
// table holds two such pairs (rows 10 and 14) on purpose.  There the last bit of the two angles decides which value comes out, so a
// library atan2 that is one unit off (the device's is, at row 14) returns the other side of the discontinuity, 0.06 away.  The
// correctly rounded angle makes that decision a property of the formula, not of a math library.
struct dd { double hi, lo; };

__device__ __forceinline__ dd quick_two_sum(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }      // |a| >= |b|
__device__ __forceinline__ dd two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd two_prod(double a, double b) { const double p = a * b; return {p, fma(a, b, -p)}; }
__device__ __forceinline__ dd dd_add(dd a, dd b) {
  dd s = two_sum(a.hi, b.hi);
  const dd t = two_sum(a.lo, b.lo);
  s = quick_two_sum(s.hi, s.lo + t.hi);
  return quick_two_sum(s.hi, s.lo + t.lo);
}
__device__ __forceinline__ dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
  const dd p = two_prod(a.hi, b.hi);
  return quick_two_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
__device__ __forceinline__ dd dd_div(dd a, dd b) {
  const double q1 = a.hi / b.hi;
  dd r = dd_add(a, dd_neg(dd_mul(b, {q1, 0.0})));
  const double q2 = r.hi / b.hi;
  r = dd_add(r, dd_neg(dd_mul(b, {q2, 0.0})));
  const double q3 = r.hi / b.hi;
  return dd_add(quick_two_sum(q1, q2), {q3, 0.0});
}
__device__ __forceinline__ dd dd_sqrt(dd a) {      // a > 0: one Newton step on the double root
  const double x = 1.0 / sqrt(a.hi), ax = a.hi * x;
  const dd err = dd_add(a, dd_neg(two_prod(ax, ax)));
  return two_sum(ax, err.hi * (x * 0.5));
}

// atan2(y, x) of finite doubles.  r = min(|x|, |y|) / max(|x|, |y|) in [0, 1]; three half-angle steps r <- r / (1 + sqrt(1 + r^2))
// bring it below tan(pi / 32); the alternating series of atan to the 35th power leaves less than 2^-110; the octant is undone with
// pi and pi / 2 as double-doubles.
__device__ __forceinline__ double atan2_cr(double y, double x) {
  if (x == 0.0 || y == 0.0 || !(fabs(x) <= 1.7976931348623157e308) || !(fabs(y) <= 1.7976931348623157e308)) return atan2(y, x);
  const double ax = fabs(x), ay = fabs(y);
  const bool swap = ay > ax;
  dd r = dd_div({swap ? ax : ay, 0.0}, {swap ? ay : ax, 0.0});
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const dd root = dd_sqrt(dd_add({1.0, 0.0}, dd_mul(r, r)));
    r = dd_div(r, dd_add({1.0, 0.0}, root));
  }
  const dd z = dd_neg(dd_mul(r, r));
  dd s = {1.0 / 37.0, fma(-(1.0 / 37.0), 37.0, 1.0) / 37.0};
#pragma unroll
  for (int n = 35; n >= 1; n -= 2) {
    const double c = 1.0 / (double)n;
    s = dd_add(dd_mul(s, z), {c, fma(-c, (double)n, 1.0) / (double)n});
  }
  dd t = dd_mul(r, s);
  t.hi *= 8.0; t.lo *= 8.0;
  if (swap) t = dd_add({1.5707963267948966, 6.123233995736766e-17}, dd_neg(t));
  if (x < 0.0) t = dd_add({3.141592653589793, 1.2246467991473532e-16}, dd_neg(t));
  return y < 0.0 ? -t.hi : t.hi;
}

using Cut = Select<unsigned long long>;

struct ColorWs {
  unsigned* hist;      // [kPasses][N][kBins]
  Cut* sel;            // [N]
  unsigned* flag;      // [N]
  unsigned* count;     // [N][pix_blocks]     pixels whose angle counts
  double* part;        // [N][pix_blocks][3]  sum of de00, of de76, of the counted angles
  double* de00;        // [N][H * W]
};

struct ColorParams {
  int N, H, W, pix_blocks, hist_blocks;
  unsigned K, rank;              // pixels per image; the rank of the percentile (from 0)
};

__device__ __forceinline__ double pow7(double x) {
  const double x2 = x * x, x4 = x2 * x2;
  return (x4 * x2) * x;
}

// h' in degrees, in [0, 360); 0 where both components are 0
__device__ __forceinline__ double hue_deg(double b, double ap) {
  double h = atan2_cr(b, ap) * kR2D;
  if (h < 0.0) h = h + 360.0;
  return (ap == 0.0 && b == 0.0) ? 0.0 : h;
}

// Sharma, Wu, Dalal 2005, kL = kC = kH = 1; the operations and their order are those of tests/_color_def.ciede2000_terms
__device__ __forceinline__ double ciede2000(double L1, double a1, double b1, double L2, double a2, double b2) {
  const double c1 = sqrt((a1 * a1) + (b1 * b1)), c2 = sqrt((a2 * a2) + (b2 * b2));
  const double cb7 = pow7((c1 + c2) / 2.0);
  const double g = 0.5 * (1.0 - sqrt(cb7 / (cb7 + kPow25_7)));
  const double ap1 = (1.0 + g) * a1, ap2 = (1.0 + g) * a2;
  const double cp1 = sqrt((ap1 * ap1) + (b1 * b1)), cp2 = sqrt((ap2 * ap2) + (b2 * b2));
  const double h1 = hue_deg(b1, ap1), h2 = hue_deg(b2, ap2);
  const double dl = L2 - L1, dc = cp2 - cp1, cc = cp1 * cp2;
  const double d = h2 - h1;
  const double dh = cc == 0.0 ? 0.0 : (fabs(d) <= 180.0 ? d : (d > 180.0 ? d - 360.0 : d + 360.0));
  const double dH = (2.0 * sqrt(cc)) * sin((dh / 2.0) * kD2R);
  const double lb = (L1 + L2) / 2.0, cb = (cp1 + cp2) / 2.0;
  const double hs = h1 + h2;
  const double hb = cc == 0.0 ? hs : (fabs(h1 - h2) <= 180.0 ? hs / 2.0 : (hs < 360.0 ? (hs + 360.0) / 2.0 : (hs - 360.0) / 2.0));
  const double t = (((1.0 - (0.17 * cos((hb - 30.0) * kD2R))) + (0.24 * cos((2.0 * hb) * kD2R)))
                    + (0.32 * cos(((3.0 * hb) + 6.0) * kD2R))) - (0.20 * cos(((4.0 * hb) - 63.0) * kD2R));
  const double q = (hb - 275.0) / 25.0;
  const double dtheta = 30.0 * exp(-(q * q));
  const double cbp7 = pow7(cb);
  const double rc = 2.0 * sqrt(cbp7 / (cbp7 + kPow25_7));
  const double l50 = (lb - 50.0) * (lb - 50.0);
  const double sl = 1.0 + ((0.015 * l50) / sqrt(20.0 + l50));
  const double sc = 1.0 + (0.045 * cb);
  const double sh = 1.0 + ((0.015 * cb) * t);
  const double rt = -sin((2.0 * dtheta) * kD2R) * rc;
  const double tl = dl / sl, tc = dc / sc, th = dH / sh;
  return sqrt((((tl * tl) + (tc * tc)) + (th * th)) + ((rt * tc) * th));
}

__global__ __launch_bounds__(kThreads) void color_init_kernel(const ColorParams P, const ColorWs ws) {
  const int64_t nh = (int64_t)kPasses * P.N * kBins;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nh; i += (int64_t)gridDim.x * kThreads) ws.hist[i] = 0u;
  if (blockIdx.x != 0) return;
  for (int i = threadIdx.x; i < P.N; i += kThreads) {
    ws.flag[i] = 0u;
    ws.sel[i] = select_start<unsigned long long>(P.rank);
  }
}

__global__ __launch_bounds__(kThreads) void color_pixel_kernel(const ColorParams P, const ColorWs ws, const float* __restrict__ pred,
                                                                const float* __restrict__ target, float* __restrict__ map) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)P.H * P.W;
  const float* p = pred + (int64_t)n * 3 * HW;
  const float* t = target + (int64_t)n * 3 * HW;
  double* plane = ws.de00 + (int64_t)n * HW;
  double sum_00 = 0.0, sum_76 = 0.0, sum_ang = 0.0;
  unsigned counted = 0u;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const float pr = p[i], pg = p[HW + i], pb = p[2 * HW + i];
    const float tr = t[i], tg = t[HW + i], tb = t[2 * HW + i];
    bad |= non_finite(pr) || non_finite(pg) || non_finite(pb) || non_finite(tr) || non_finite(tg) || non_finite(tb);
    const double u0 = (double)fminf(fmaxf(pr, 0.0f), 1.0f), u1 = (double)fminf(fmaxf(pg, 0.0f), 1.0f),
                 u2 = (double)fminf(fmaxf(pb, 0.0f), 1.0f);
    const double v0 = (double)fminf(fmaxf(tr, 0.0f), 1.0f), v1 = (double)fminf(fmaxf(tg, 0.0f), 1.0f),
                 v2 = (double)fminf(fmaxf(tb, 0.0f), 1.0f);
    double L1, a1, b1, L2, a2, b2;
    srgb_to_lab(u0, u1, u2, L1, a1, b1);
    srgb_to_lab(v0, v1, v2, L2, a2, b2);
    const double dl = L2 - L1, da = a2 - a1, db = b2 - b1;
    const double e76 = sqrt(((dl * dl) + (da * da)) + (db * db));
    const double e00 = ciede2000(L1, a1, b1, L2, a2, b2);
    const double cx = (u1 * v2) - (u2 * v1), cy = (u2 * v0) - (u0 * v2), cz = (u0 * v1) - (u1 * v0);
    const double cross = sqrt(((cx * cx) + (cy * cy)) + (cz * cz));
    const double dot = ((u0 * v0) + (u1 * v1)) + (u2 * v2);
    const bool valid = (u0 != 0.0 || u1 != 0.0 || u2 != 0.0) && (v0 != 0.0 || v1 != 0.0 || v2 != 0.0);
    plane[i] = e00;
    if (map) map[(int64_t)n * HW + i] = (float)e00;
    sum_00 += e00;
    sum_76 += e76;
    if (valid) {
      sum_ang += atan2(cross, dot) * kR2D;
      ++counted;
    }
  }
  if (bad) ws.flag[n] = 1u;
  const double s0 = block_sum_all<kThreads>(sum_00), s1 = block_sum_all<kThreads>(sum_76), s2 = block_sum_all<kThreads>(sum_ang);
  const double s3 = block_sum_all<kThreads>((double)counted);      // whole numbers below 2^53: exact in any order
  if (threadIdx.x == 0) {
    double* o = ws.part + ((int64_t)n * P.pix_blocks + blockIdx.x) * 3;
    o[0] = s0; o[1] = s1; o[2] = s2;
    ws.count[(int64_t)n * P.pix_blocks + blockIdx.x] = (unsigned)s3;
  }
}

// One digit of the select: counts the pixels whose key agrees with the select's prefix above `match_shift` (match_shift == 64: every
// pixel), binned by the `bits` bits below it.
__global__ __launch_bounds__(kThreads) void color_hist_kernel(const ColorParams P, const ColorWs ws, int pass, int match_shift,
                                                               int bits) {
  __shared__ unsigned sh[kBins];
  const int n = blockIdx.z;
  for (int i = threadIdx.x; i < kBins; i += kThreads) sh[i] = 0u;
  const unsigned long long prefix = ws.sel[n].prefix;
  __syncthreads();
  const int64_t HW = (int64_t)P.H * P.W;
  const double* plane = ws.de00 + (int64_t)n * HW;
  const int bin_shift = match_shift - bits;
  const unsigned mask = (1u << bits) - 1u;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const unsigned long long k = key_of(plane[i]);
    const unsigned bin = (unsigned)(k >> bin_shift) & mask;
    if (match_shift == 64 || (k >> match_shift) == prefix) atomicAdd(&sh[bin], 1u);
  }
  select_flush<kThreads>(sh, ws.hist + ((int64_t)pass * P.N + n) * kBins, kBins);
}

// grid (1, 1, N): the bin that holds the select's rank; prefix, rank within the bin, pixels below and inside it
__global__ __launch_bounds__(kThreads) void color_scan_kernel(const ColorParams P, const ColorWs ws, int pass, int bits) {
  const int n = blockIdx.z;
  select_scan<kThreads, kBins>(ws.hist + ((int64_t)pass * P.N + n) * kBins, &ws.sel[n], bits);
}

__global__ __launch_bounds__(kThreads) void color_finalize_kernel(const ColorParams P, const ColorWs ws, double* __restrict__ out) {
  const int n = blockIdx.x;
  const double* part = ws.part + (int64_t)n * P.pix_blocks * 3;
  const double s00 = sum_partials<kThreads>(part, P.pix_blocks, 3), s76 = sum_partials<kThreads>(part + 1, P.pix_blocks, 3);
  const double sang = sum_partials<kThreads>(part + 2, P.pix_blocks, 3);
  if (threadIdx.x != 0) return;
  unsigned counted = 0u;
  for (int i = 0; i < P.pix_blocks; ++i) counted += ws.count[(int64_t)n * P.pix_blocks + i];
  double e00 = s00 / (double)P.K, p95 = value_of(ws.sel[n].prefix), e76 = s76 / (double)P.K;
  double ang = counted ? sang / (double)counted : (double)NAN;
  if (ws.flag[n]) e00 = p95 = e76 = ang = (double)NAN;
  out[4 * n] = e00;
  out[4 * n + 1] = p95;
  out[4 * n + 2] = e76;
  out[4 * n + 3] = ang;
}

__global__ __launch_bounds__(kThreads) void ciede2000_lab_kernel(const double* __restrict__ lab1, const double* __restrict__ lab2,
                                                                  int64_t n, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    out[i] = ciede2000(lab1[3 * i], lab1[3 * i + 1], lab1[3 * i + 2], lab2[3 * i], lab2[3 * i + 1], lab2[3 * i + 2]);
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the regions of the workspace, in order; returns its size
int64_t color_layout(void* base, int N, int64_t K, int pb, ColorWs* ws) {
  Carver c(base);
  ws->hist = c.take<unsigned>((int64_t)kPasses * N * kBins);
  ws->sel = c.take<Cut>(N);
  ws->flag = c.take<unsigned>(N);
  ws->count = c.take<unsigned>((int64_t)N * pb);
  ws->part = c.take<double>((int64_t)N * pb * 3);
  ws->de00 = c.take<double>((int64_t)N * K);
  return c.total();
}

}  // namespace

extern "C" {

int hdiff_color_diff_workspace(int N, int H, int W, int64_t* bytes) {
  const int rc = check_sizes("color_diff_workspace", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "color_diff_workspace: null pointer");
  const int64_t K = (int64_t)H * W;
  ColorWs ws;
  *bytes = color_layout(nullptr, N, K, parts_for(K, kPixPerBlock, kMaxPixBlocks), &ws);
  return HDIFF_OK;
}

int hdiff_color_diff(const float* pred, const float* target, int N, int H, int W, double* out, float* map, void* scratch,
                     hdiff_stream_t stream) {
  const int rc = check_sizes("color_diff", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(pred && target && out && scratch, "color_diff: null pointer");
  (void)hipGetLastError();
  ColorParams P;
  P.N = N; P.H = H; P.W = W;
  const int64_t K = (int64_t)H * W;
  P.pix_blocks = parts_for(K, kPixPerBlock, kMaxPixBlocks);
  P.hist_blocks = parts_for(K, kHistPerBlock, kMaxHistBlocks);
  P.K = (unsigned)K;
  P.rank = (unsigned)((95 * K + 99) / 100 - 1);
  ColorWs ws;
  color_layout(scratch, N, K, P.pix_blocks, &ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads), pix(P.pix_blocks, 1, N), hist(P.hist_blocks, 1, N);
  const int64_t nh = (int64_t)kPasses * N * kBins;
  const int init_blocks = (int)((nh / kThreads) > 1024 ? 1024 : (nh / kThreads));
  hipLaunchKernelGGL(color_init_kernel, dim3(init_blocks), blk, 0, s, P, ws);
  hipLaunchKernelGGL(color_pixel_kernel, pix, blk, 0, s, P, ws, pred, target, map);
  const int bits[kPasses] = {11, 11, 11, 11, 10, 10};
  int shift = 64;
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(color_hist_kernel, hist, blk, 0, s, P, ws, pass, shift, bits[pass]);
    hipLaunchKernelGGL(color_scan_kernel, dim3(1, 1, N), blk, 0, s, P, ws, pass, bits[pass]);
    shift -= bits[pass];
  }
  hipLaunchKernelGGL(color_finalize_kernel, dim3(N), blk, 0, s, P, ws, out);
  HDIFF_CHECK_LAUNCH("color_diff kernels");
  return HDIFF_OK;
}

int hdiff_ciede2000_lab(const double* lab1, const double* lab2, int64_t n, double* out, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(n >= 1 && n <= (1ll << 30), "ciede2000_lab: n = %lld; between 1 and 2^30 rows", (long long)n);
  HDIFF_CHECK_ARG(lab1 && lab2 && out, "ciede2000_lab: null pointer");
  (void)hipGetLastError();
  const int blocks = parts_for(n, kThreads, 4096);
  hipLaunchKernelGGL(ciede2000_lab_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, lab1, lab2, n, out);
  HDIFF_CHECK_LAUNCH("ciede2000_lab kernel");
  return HDIFF_OK;
}

}  // extern "C"
