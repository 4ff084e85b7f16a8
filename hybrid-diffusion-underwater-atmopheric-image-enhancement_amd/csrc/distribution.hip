// Set-level statistics of feature rows on the device: what a Frechet distance and a KID over a feature extractor need from the rows
// (hdiff_amd/quality.py: moments, kid, DistributionMeter; tests/_distribution_def.py is the definition the kernels are held to).
// Features are fp32, n rows of d values, value (r, i) at feats[r * row_stride + i * ch_stride] (strides in elements): the class-token
// view nf[:, :, 0] of a channel-major (B, C, L) tensor is read in place with row_stride = C * L, ch_stride = L.
//
// hdiff_feat_moments, two launches, everything in double:
//   1. moments_mean_kernel     one thread per channel: sum of (double)x[r][i] over r = 0 .. n-1 in that order, divided once by n
//   2. moments_scatter_kernel  one workgroup per 32 x 32 tile of (i, j), every tile of the square (the product commutes, so cov[i][j]
//                              and cov[j][i] come out bit for bit equal without a mirror pass); the centred rows x[r][.] - mean[.] are
//                              staged in LDS 32 rows at a time and every thread walks r in order for its 2 x 2 outputs; difference,
//                              product and sum each round on their own; divided once by n - 1 (n = 1: 0 / 0 = NaN)
// hdiff_kid_sums, four launches: the kernel k(x, y) = (x.y / d + 1)^3 in double, x.y accumulated over the channels 0 .. d-1 in order
// (a product of two fp32 values is exact in double), the cube as (t * t) * t.
//   1-3. kid_pairs_kernel      the a-a, b-b and a-b blocks.  One workgroup per pair of 32-row blocks (I, J), I <= J; 32 channels at a
//                              time go through LDS.  A thread holds 2 x 2 row pairs (i, j), i in I, j in J, and for each BOTH
//                              k(x_i, y_j) and k(x_j, y_i), which it adds first: that sum commutes, and everything behind it is indexed
//                              by the unordered pair, so a call with a and b swapped gives the swapped triple bit for bit.  (In the
//                              a-a and b-b blocks the two are the same number; it is computed once and added to itself.)  On I == J
//                              the pairs i < j count as above, i == j once (not at all in a-a and b-b: the sums there run over
//                              i != j), i > j not.  The workgroup's sum goes to its own slot of the scratch.
//   4. kid_total_kernel        three workgroups: the slots of one block each, added in a fixed order
// Plain fp64 vector arithmetic: the fp64 MFMA would fix neither the order of the channel sum nor that of the row sum to the
// definition's, and at a few hundred rows the launches are short either way.
// The LDS tiles are [reduction index][tile index]: the 16 threads that differ in tx read 16 consecutive doubles (32 banks of the 64
// a ds_read_b64 sees), the two ty values of a 32-lane half read one address each (a broadcast): no bank conflicts in the loop.  The
// pair kernel stages rows that are contiguous along the REDUCTION axis, so its tiles are padded to 33 doubles per line: the 32 lanes
// that write one row then fall on distinct bank pairs two by two instead of on one.
// No float atomics, no allocation, no synchronisation; every sum has one order.  Compiled with -ffp-contract=off.
#include <math.h>

#include "common.h"
#include "reduce.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;               // outputs per tile side; a thread holds (ty, ty + 16) x (tx, tx + 16)
constexpr int kChunk = 32;              // rows (moments) or channels (pairs) staged at a time
constexpr int kPad = kTile + 1;
constexpr int kMaxRows = 32768;
constexpr int kMaxDim = 8192;

struct Rows {
  const float* p;
  int n;
  int64_t row_stride, ch_stride;
};

__global__ __launch_bounds__(kThreads) void moments_mean_kernel(const Rows X, int d, double* __restrict__ mean) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= d) return;
  const float* col = X.p + (int64_t)i * X.ch_stride;
  double s = 0.0;
  for (int r = 0; r < X.n; ++r) s += (double)col[(int64_t)r * X.row_stride];
  mean[i] = s / (double)X.n;
}

__global__ __launch_bounds__(kThreads) void moments_scatter_kernel(const Rows X, int d, const double* __restrict__ mean,
                                                                    double* __restrict__ cov) {
  __shared__ double ci[kChunk][kTile], cj[kChunk][kTile];
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int k = threadIdx.x & (kTile - 1), rq = threadIdx.x >> 5;      // staging: channel k of rows rq, rq + 8, ...
  const bool has_i = i0 + k < d, has_j = j0 + k < d;
  const double mi = has_i ? mean[i0 + k] : 0.0, mj = has_j ? mean[j0 + k] : 0.0;
  const float* pi = X.p + (int64_t)(i0 + k) * X.ch_stride;
  const float* pj = X.p + (int64_t)(j0 + k) * X.ch_stride;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 0; r0 < X.n; r0 += kChunk) {
    const int len = X.n - r0 < kChunk ? X.n - r0 : kChunk;
    for (int r = rq; r < len; r += kThreads / kTile) {
      const int64_t off = (int64_t)(r0 + r) * X.row_stride;
      ci[r][k] = has_i ? (double)pi[off] - mi : 0.0;
      cj[r][k] = has_j ? (double)pj[off] - mj : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < len; ++r) {
      const double a0 = ci[r][ty], a1 = ci[r][ty + 16], b0 = cj[r][tx], b1 = cj[r][tx + 16];
      acc[0] += a0 * b0;
      acc[1] += a0 * b1;
      acc[2] += a1 * b0;
      acc[3] += a1 * b1;
    }
    __syncthreads();
  }
  const double denom = (double)X.n - 1.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + ty + 16 * (q >> 1), j = j0 + tx + 16 * (q & 1);
    if (i < d && j < d) cov[(int64_t)i * d + j] = acc[q] / denom;
  }
}

__device__ __forceinline__ double poly3(double dot, double d) {
  const double t = dot / d + 1.0;
  return (t * t) * t;
}

// linear tile id -> (I, J), I <= J, tiles ordered by J then I
__device__ __forceinline__ void tile_of(int t, int* I, int* J) {
  int j = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((int64_t)j * (j + 1) / 2 > t) --j;
  while ((int64_t)(j + 1) * (j + 2) / 2 <= t) ++j;
  *J = j;
  *I = t - (int)((int64_t)j * (j + 1) / 2);
}

// one line of a staged tile: channel c0 + c of row `row` of X, 0 outside the set
__device__ __forceinline__ double row_value(const Rows& X, int row, int c, int d) {
  return (row < X.n && c < d) ? (double)X.p[(int64_t)row * X.row_stride + (int64_t)c * X.ch_stride] : 0.0;
}

// SELF: Y is X and the diagonal is left out
template <bool SELF>
__global__ __launch_bounds__(kThreads) void kid_pairs_kernel(const Rows X, const Rows Y, int d, double* __restrict__ slots) {
  __shared__ double xi[kChunk][kPad], xj[kChunk][kPad];
  __shared__ double yi[SELF ? 1 : kChunk][kPad], yj[SELF ? 1 : kChunk][kPad];
  int I, J;
  tile_of(blockIdx.x, &I, &J);
  const int i0 = I * kTile, j0 = J * kTile;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = threadIdx.x & (kChunk - 1), kq = threadIdx.x >> 5;      // staging: channel c of rows kq, kq + 8, ...
  double u[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};      // u: x_i . y_j    w: x_j . y_i
  for (int c0 = 0; c0 < d; c0 += kChunk) {
    const int len = d - c0 < kChunk ? d - c0 : kChunk;
    for (int k = kq; k < kTile; k += kThreads / kChunk) {
      xi[c][k] = row_value(X, i0 + k, c0 + c, d);
      xj[c][k] = row_value(X, j0 + k, c0 + c, d);
      if constexpr (!SELF) {
        yi[c][k] = row_value(Y, i0 + k, c0 + c, d);
        yj[c][k] = row_value(Y, j0 + k, c0 + c, d);
      }
    }
    __syncthreads();
    for (int cc = 0; cc < len; ++cc) {
      const double a0 = xi[cc][ty], a1 = xi[cc][ty + 16];
      const double b0 = SELF ? xj[cc][tx] : yj[cc][tx], b1 = SELF ? xj[cc][tx + 16] : yj[cc][tx + 16];
      u[0] += a0 * b0;
      u[1] += a0 * b1;
      u[2] += a1 * b0;
      u[3] += a1 * b1;
      if constexpr (!SELF) {
        const double e0 = yi[cc][ty], e1 = yi[cc][ty + 16], f0 = xj[cc][tx], f1 = xj[cc][tx + 16];
        w[0] += f0 * e0;
        w[1] += f1 * e0;
        w[2] += f0 * e1;
        w[3] += f1 * e1;
      }
    }
    __syncthreads();
  }
  const double dd = (double)d;
  double sum = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + ty + 16 * (q >> 1), j = j0 + tx + 16 * (q & 1);
    const bool in_u = i < X.n && j < Y.n, in_w = j < X.n && i < Y.n;      // (i, j) and (j, i) lie inside the n x m rectangle
    double v = 0.0;
    if (i < j) {
      const double ku = poly3(u[q], dd), kw = SELF ? ku : poly3(w[q], dd);
      v = (in_u ? ku : 0.0) + (in_w ? kw : 0.0);
    } else if (i == j && !SELF) {
      v = in_u ? poly3(u[q], dd) : 0.0;
    }
    sum += v;
  }
  const double total = block_sum_all<kThreads>(sum);
  if (threadIdx.x == 0) slots[blockIdx.x] = total;
}

struct KidCounts { int tiles[3]; };

__global__ __launch_bounds__(kThreads) void kid_total_kernel(const double* __restrict__ slots, const KidCounts K,
                                                              double* __restrict__ out) {
  const int b = blockIdx.x;
  int first = 0;
  for (int q = 0; q < b; ++q) first += K.tiles[q];
  const double s = sum_partials<kThreads>(slots + first, K.tiles[b], 1);
  if (threadIdx.x == 0) out[b] = s;
}

int tiles_of(int rows) {
  const int nb = (rows + kTile - 1) / kTile;
  return nb * (nb + 1) / 2;
}

int check_rows(const char* who, const char* name, int n, int d, int64_t row_stride, int64_t ch_stride) {
  HDIFF_CHECK_ARG(n >= 1 && n <= kMaxRows, "%s: %s = %d; between 1 and %d rows", who, name, n, kMaxRows);
  HDIFF_CHECK_ARG(d >= 1 && d <= kMaxDim, "%s: d = %d; between 1 and %d values per row", who, d, kMaxDim);
  HDIFF_CHECK_ARG(row_stride >= 1 && ch_stride >= 1 && row_stride <= (1ll << 40) && ch_stride <= (1ll << 40),
                  "%s: strides of %s = (%lld, %lld); both must be positive element counts", who, name, (long long)row_stride,
                  (long long)ch_stride);
  return HDIFF_OK;
}

}  // namespace

extern "C" {

int hdiff_feat_moments(const float* feats, int n, int d, int64_t row_stride, int64_t ch_stride, double* mean, double* cov,
                       hdiff_stream_t stream) {
  const int rc = check_rows("feat_moments", "n", n, d, row_stride, ch_stride);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(feats && mean && cov, "feat_moments: null pointer");
  (void)hipGetLastError();
  const Rows X{feats, n, row_stride, ch_stride};
  hipStream_t s = (hipStream_t)stream;
  const int nb = cdiv(d, kTile);
  hipLaunchKernelGGL(moments_mean_kernel, dim3(cdiv(d, kThreads)), dim3(kThreads), 0, s, X, d, mean);
  hipLaunchKernelGGL(moments_scatter_kernel, dim3(nb, nb), dim3(kThreads), 0, s, X, d, (const double*)mean, cov);
  HDIFF_CHECK_LAUNCH("feat_moments kernels");
  return HDIFF_OK;
}

int hdiff_kid_workspace(int n, int m, int64_t* bytes) {
  HDIFF_CHECK_ARG(n >= 1 && n <= kMaxRows, "kid_workspace: n = %d; between 1 and %d rows", n, kMaxRows);
  HDIFF_CHECK_ARG(m >= 1 && m <= kMaxRows, "kid_workspace: m = %d; between 1 and %d rows", m, kMaxRows);
  HDIFF_CHECK_ARG(bytes, "kid_workspace: null pointer");
  *bytes = align256(((int64_t)tiles_of(n) + tiles_of(m) + tiles_of(n > m ? n : m)) * (int64_t)sizeof(double));
  return HDIFF_OK;
}

int hdiff_kid_sums(const float* a, int n, const float* b, int m, int d, int64_t a_row_stride, int64_t a_ch_stride,
                   int64_t b_row_stride, int64_t b_ch_stride, double* out, void* scratch, hdiff_stream_t stream) {
  int rc = check_rows("kid_sums", "n", n, d, a_row_stride, a_ch_stride);
  if (rc != HDIFF_OK) return rc;
  rc = check_rows("kid_sums", "m", m, d, b_row_stride, b_ch_stride);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(a && b && out && scratch, "kid_sums: null pointer");
  (void)hipGetLastError();
  const Rows A{a, n, a_row_stride, a_ch_stride}, B{b, m, b_row_stride, b_ch_stride};
  KidCounts K;
  K.tiles[0] = tiles_of(n); K.tiles[1] = tiles_of(m); K.tiles[2] = tiles_of(n > m ? n : m);
  double* slots = (double*)scratch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kid_pairs_kernel<true>, dim3(K.tiles[0]), dim3(kThreads), 0, s, A, A, d, slots);
  hipLaunchKernelGGL(kid_pairs_kernel<true>, dim3(K.tiles[1]), dim3(kThreads), 0, s, B, B, d, slots + K.tiles[0]);
  hipLaunchKernelGGL(kid_pairs_kernel<false>, dim3(K.tiles[2]), dim3(kThreads), 0, s, A, B, d, slots + K.tiles[0] + K.tiles[1]);
  hipLaunchKernelGGL(kid_total_kernel, dim3(3), dim3(kThreads), 0, s, (const double*)slots, K, out);
  HDIFF_CHECK_LAUNCH("kid_sums kernels");
  return HDIFF_OK;
}

}  // extern "C"
