// UCIQE on the device: the colour-quality score the reference's evaluation takes per sampled image beside UIQM (the UCIQE part of
// `nmetrics`, metrics/metrics.py:301-337, called at utils/rotinas.py:923 and :1171; tests/_uciqe_def.py is the definition the kernels
// are held to, hdiff_amd/uw_metrics.nmetrics the host restatement).  Conventions are those of quality.hip: input fp32 [N][3][H][W] with
// nominal range [0, 1], images on blockIdx.z, grids and partial counts functions of H and W alone, outputs float64, one row per image.
//
// Per pixel, in double: rgb = double(min(max(x, 0), 1)) * scale (the clip in fp32), sRGB -> linear -> XYZ (D65) -> CIE L*a*b* (lab.h),
// chroma = sqrt(a^2 + b^2), saturation = chroma / L (0 where chroma or L is 0).  Per image:
//   sc   = sqrt(mean((chroma - mean(chroma))^2))                     two passes
//   conl = mean(the `top` largest L) - mean(the `top` smallest L)    top = round_half_even(0.01 H W); NaN when top == 0
//   us   = mean(saturation)
//   uciqe = 0.4680 sc + 0.2745 conl + 0.2576 us
//
// hdiff_uciqe, sixteen launches:
//   1. uciqe_init_kernel      zeroes the histograms and flags, sets the two selects of every image (ranks top - 1 from either end)
//   2. uciqe_lab_kernel       the conversion; writes the L and chroma planes as doubles into the scratch; per-workgroup double sums of
//                             chroma and of the saturation term; the non-finite flag
//   3-14. uciqe_hist_kernel + uciqe_scan_kernel, six times (11 / 11 / 11 / 11 / 10 / 10 bits): radix select of the two cut values of L
//                             on the order-preserving 64-bit integer key of the double (an fp32 key would not do: doubles that share
//                             one fp32 value straddle the cut).  Histograms: integer LDS atomics per workgroup, merged with integer
//                             global atomics, so counts do not depend on arrival order.
//  15. uciqe_tail_kernel      sum of L strictly below the low cut and strictly above the high cut (the finalize kernel adds the copies
//                             of the cut values that belong to each tail, which makes ties at a cut exact); every workgroup rebuilds
//                             mean(chroma) from the partials, in the same order everywhere, and sums (chroma - mean)^2
//  16. uciqe_finalize_kernel  grid (N): adds the partials in index order; sc, conl, us, uciqe
// This is the suggested launch list with one addition, the init kernel (the histograms and selects must be reset by the call itself:
// no memset node, nothing left to the caller), and with the chroma plane kept, so that the conversion runs once per pixel.
// No float atomics, no allocation, no synchronisation.  Compiled with -ffp-contract=off: the per-pixel formulas round where the
// definition's separate double operations round (black comes out as exactly L = 0, chroma = 0).
#include <math.h>

#include "common.h"
#include "lab.h"
#include "radix_select.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 2048;
constexpr int kSelects = 2;                    // 0: the low cut, 1: the high cut
constexpr int kPasses = 6;
constexpr int kMaxPixBlocks = 256;
constexpr int kPixPerBlock = kThreads * 8;

// on the 64-bit key of L (L comes out a few ulp below zero for near-black pixels: -0 and +0 must share a key)
using Cut = Select<unsigned long long>;

struct UciqeWs {
  unsigned* hist;      // [kPasses][N][kSelects][kBins]
  Cut* sel;            // [N][kSelects]
  unsigned* flag;      // [N]
  double* part;        // [N][pix_blocks][2]  sum of chroma, sum of the saturation term
  double* tail;        // [N][pix_blocks][3]  sum of L below the low cut, above the high cut, sum of (chroma - mean)^2
  double* lum;         // [N][H * W]
  double* chroma;      // [N][H * W]
};

struct UciqeParams {
  int N, H, W, pix_blocks;
  unsigned K, top;               // pixels per image; size of each tail (0: conl is undefined)
  double scale;
};

__global__ __launch_bounds__(kThreads) void uciqe_init_kernel(const UciqeParams P, const UciqeWs ws) {
  const int64_t nh = (int64_t)kPasses * P.N * kSelects * kBins;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nh; i += (int64_t)gridDim.x * kThreads) ws.hist[i] = 0u;
  if (blockIdx.x != 0) return;
  for (int i = threadIdx.x; i < P.N; i += kThreads) ws.flag[i] = 0u;
  const unsigned t = P.top ? P.top : 1u;      // top == 0: any rank inside the image; the result is not used
  for (int i = threadIdx.x; i < P.N * kSelects; i += kThreads) ws.sel[i] = select_start<unsigned long long>((i & 1) ? P.K - t : t - 1u);
}

__global__ __launch_bounds__(kThreads) void uciqe_lab_kernel(const UciqeParams P, const UciqeWs ws, const float* __restrict__ x) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)P.H * P.W;
  const float* img = x + (int64_t)n * 3 * HW;
  double* lum = ws.lum + (int64_t)n * HW;
  double* chr = ws.chroma + (int64_t)n * HW;
  double sum_c = 0.0, sum_s = 0.0;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const float xr = img[i], xg = img[HW + i], xb = img[2 * HW + i];
    bad |= non_finite(xr) || non_finite(xg) || non_finite(xb);
    double L, ca, cb;
    srgb_to_lab((double)fminf(fmaxf(xr, 0.0f), 1.0f) * P.scale, (double)fminf(fmaxf(xg, 0.0f), 1.0f) * P.scale,
                (double)fminf(fmaxf(xb, 0.0f), 1.0f) * P.scale, L, ca, cb);
    const double c = sqrt(ca * ca + cb * cb);
    lum[i] = L;
    chr[i] = c;
    sum_c += c;
    sum_s += (c == 0.0 || L == 0.0) ? 0.0 : c / L;
  }
  if (bad) ws.flag[n] = 1u;
  const double s0 = block_sum_all<kThreads>(sum_c), s1 = block_sum_all<kThreads>(sum_s);
  if (threadIdx.x == 0) {
    double* o = ws.part + ((int64_t)n * P.pix_blocks + blockIdx.x) * 2;
    o[0] = s0; o[1] = s1;
  }
}

// One digit of the select: counts, per select, the pixels whose key agrees with the select's prefix above `match_shift`
// (match_shift == 64: every pixel, one histogram for both selects), binned by the `bits` bits below it.
__global__ __launch_bounds__(kThreads) void uciqe_hist_kernel(const UciqeParams P, const UciqeWs ws, int pass, int match_shift,
                                                               int bits) {
  __shared__ unsigned sh[kSelects * kBins];
  const int n = blockIdx.z;
  for (int i = threadIdx.x; i < kSelects * kBins; i += kThreads) sh[i] = 0u;
  const unsigned long long p0 = ws.sel[n * kSelects].prefix, p1 = ws.sel[n * kSelects + 1].prefix;
  __syncthreads();
  const int64_t HW = (int64_t)P.H * P.W;
  const double* lum = ws.lum + (int64_t)n * HW;
  const int bin_shift = match_shift - bits;
  const unsigned mask = (1u << bits) - 1u;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const unsigned long long k = key_of(lum[i]);
    const unsigned bin = (unsigned)(k >> bin_shift) & mask;
    if (match_shift == 64) {
      atomicAdd(&sh[bin], 1u);      // first digit: select_hist's rule, one histogram for both selects
    } else {
      if ((k >> match_shift) == p0) atomicAdd(&sh[bin], 1u);
      if ((k >> match_shift) == p1) atomicAdd(&sh[kBins + bin], 1u);
    }
  }
  select_flush<kThreads>(sh, ws.hist + ((int64_t)pass * P.N + n) * kSelects * kBins, kSelects * kBins);
}

// grid (kSelects, 1, N): the bin that holds the select's rank; prefix, rank within the bin, pixels below and inside it
__global__ __launch_bounds__(kThreads) void uciqe_scan_kernel(const UciqeParams P, const UciqeWs ws, int pass, int bits) {
  const int s = blockIdx.x, n = blockIdx.z;
  const unsigned* h = ws.hist + (((int64_t)pass * P.N + n) * kSelects + select_hist(pass, s)) * kBins;
  select_scan<kThreads, kBins>(h, &ws.sel[n * kSelects + s], bits);
}

__global__ __launch_bounds__(kThreads) void uciqe_tail_kernel(const UciqeParams P, const UciqeWs ws) {
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)P.H * P.W;
  const double* lum = ws.lum + (int64_t)n * HW;
  const double* chr = ws.chroma + (int64_t)n * HW;
  const unsigned long long lo = ws.sel[n * kSelects].prefix, hi = ws.sel[n * kSelects + 1].prefix;
  const double mean = sum_partials<kThreads>(ws.part + (int64_t)n * P.pix_blocks * 2, P.pix_blocks, 2) / (double)P.K;
  double below = 0.0, above = 0.0, spread = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kThreads) {
    const double L = lum[i], d = chr[i] - mean;
    const unsigned long long k = key_of(L);
    if (k < lo) below += L;
    if (k > hi) above += L;
    spread += d * d;
  }
  const double s0 = block_sum_all<kThreads>(below), s1 = block_sum_all<kThreads>(above), s2 = block_sum_all<kThreads>(spread);
  if (threadIdx.x == 0) {
    double* o = ws.tail + ((int64_t)n * P.pix_blocks + blockIdx.x) * 3;
    o[0] = s0; o[1] = s1; o[2] = s2;
  }
}

__global__ __launch_bounds__(kThreads) void uciqe_finalize_kernel(const UciqeParams P, const UciqeWs ws, double* __restrict__ out) {
  const int n = blockIdx.x;
  const double* part = ws.part + (int64_t)n * P.pix_blocks * 2;
  const double* tail = ws.tail + (int64_t)n * P.pix_blocks * 3;
  const double sum_s = sum_partials<kThreads>(part + 1, P.pix_blocks, 2);
  const double below = sum_partials<kThreads>(tail, P.pix_blocks, 3), above = sum_partials<kThreads>(tail + 1, P.pix_blocks, 3);
  const double spread = sum_partials<kThreads>(tail + 2, P.pix_blocks, 3);
  if (threadIdx.x != 0) return;
  const Cut lo = ws.sel[n * kSelects], hi = ws.sel[n * kSelects + 1];
  double sc = sqrt(spread / (double)P.K);
  double us = sum_s / (double)P.K;
  double conl = (double)NAN;
  if (P.top) {
    // the sorted prefix of length top: everything strictly below the cut, then copies of the cut value; the mirror image on top
    const double low = below + (double)(P.top - lo.less) * value_of(lo.prefix);
    const double high = above + (double)(P.top - (P.K - hi.less - hi.eq)) * value_of(hi.prefix);
    conl = high / (double)P.top - low / (double)P.top;
  }
  double uciqe = ((0.4680 * sc) + (0.2745 * conl)) + (0.2576 * us);
  if (ws.flag[n]) sc = conl = us = uciqe = (double)NAN;
  out[4 * n] = sc;
  out[4 * n + 1] = conl;
  out[4 * n + 2] = us;
  out[4 * n + 3] = uciqe;
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the regions of the workspace, in order; returns its size
int64_t uciqe_layout(void* base, int N, int64_t K, int pb, UciqeWs* ws) {
  Carver c(base);
  ws->hist = c.take<unsigned>((int64_t)kPasses * N * kSelects * kBins);
  ws->sel = c.take<Cut>((int64_t)N * kSelects);
  ws->flag = c.take<unsigned>(N);
  ws->part = c.take<double>((int64_t)N * pb * 2);
  ws->tail = c.take<double>((int64_t)N * pb * 3);
  ws->lum = c.take<double>((int64_t)N * K);
  ws->chroma = c.take<double>((int64_t)N * K);
  return c.total();
}

}  // namespace

extern "C" {

int hdiff_uciqe_workspace(int N, int H, int W, int64_t* bytes) {
  const int rc = check_sizes("uciqe_workspace", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(bytes, "uciqe_workspace: null pointer");
  const int64_t K = (int64_t)H * W;
  UciqeWs ws;
  *bytes = uciqe_layout(nullptr, N, K, parts_for(K, kPixPerBlock, kMaxPixBlocks), &ws);
  return HDIFF_OK;
}

int hdiff_uciqe(const float* a, int N, int H, int W, double scale, double* out, void* scratch, hdiff_stream_t stream) {
  const int rc = check_sizes("uciqe", N, H, W, 1);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(scale > 0.0 && scale <= 1.7976931348623157e308, "uciqe: scale = %g; it must be finite and positive", scale);
  HDIFF_CHECK_ARG(a && out && scratch, "uciqe: null pointer");
  (void)hipGetLastError();
  UciqeParams P;
  P.N = N; P.H = H; P.W = W;
  const int64_t K = (int64_t)H * W;
  P.pix_blocks = parts_for(K, kPixPerBlock, kMaxPixBlocks);
  P.K = (unsigned)K;
  P.top = (unsigned)nearbyint((0.01 * (double)H) * (double)W);      // numpy's round: half to even
  P.scale = scale;
  UciqeWs ws;
  uciqe_layout(scratch, N, K, P.pix_blocks, &ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads), pix(P.pix_blocks, 1, N);
  const int64_t nh = (int64_t)kPasses * N * kSelects * kBins;
  const int init_blocks = (int)((nh / kThreads) > 1024 ? 1024 : (nh / kThreads));
  hipLaunchKernelGGL(uciqe_init_kernel, dim3(init_blocks), blk, 0, s, P, ws);
  hipLaunchKernelGGL(uciqe_lab_kernel, pix, blk, 0, s, P, ws, a);
  const int bits[kPasses] = {11, 11, 11, 11, 10, 10};
  int shift = 64;
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(uciqe_hist_kernel, pix, blk, 0, s, P, ws, pass, shift, bits[pass]);
    hipLaunchKernelGGL(uciqe_scan_kernel, dim3(kSelects, 1, N), blk, 0, s, P, ws, pass, bits[pass]);
    shift -= bits[pass];
  }
  hipLaunchKernelGGL(uciqe_tail_kernel, pix, blk, 0, s, P, ws);
  hipLaunchKernelGGL(uciqe_finalize_kernel, dim3(N), blk, 0, s, P, ws, out);
  HDIFF_CHECK_LAUNCH("uciqe kernels");
  return HDIFF_OK;
}

}  // extern "C"
