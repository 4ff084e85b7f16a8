// DPM-Solver++(2M) update kernels (Lu et al. 2022, data-prediction form, multistep) of both samplers: the label-conditioned
// one with classifier-free guidance and the captured loop's bookkeeping (the sibling of small_ops.hip's cfg_ddim_step_kernel), the
// image-conditioned one (ddim_ops.hip's ddim_step_kernel) and its overlapping-window form (tile_ops.hip's tile_ddim_step_kernel).
// HBM-bound streaming kernels: the DDIM update's traffic plus one read and one write of the x0 history (8 bytes per element).
//
//   x0 = (x - eps * s1m) / sa ; [x0 = clamp(x0, -1, 1)] ; v = A * x + B * x0 ; [C != 0:  v = v + C * x0_prev] ; x0_prev = x0 ; x = v
//
// tab[k] = {s1m, sa, A, B, C} of position k in the time-step list (DiffusionCondition.py: dpmpp_table).  One rounding per written
// operation -- compiled with -ffp-contract=off, and the pragma repeats it -- so a plain torch program of the same lines gives the
// same bits.  The clamp is written with compares: a NaN stays a NaN.  The branch on C is uniform per launch and is not an
// optimisation: at the first step of a loop (and at the closing one) C is 0 and x0_prev holds whatever the last call left, which
// must not be read into the sum (0 * NaN is NaN).  Every element is read and written by the same thread, so x, x_next and the
// history update in place.
#include "common.h"
#include "device.h"

using namespace hdiff;

#pragma clang fp contract(off)

namespace {

inline int grid_for(int64_t n, int per_thread = 1) {
  int64_t blocks = (n + (int64_t)256 * per_thread - 1) / ((int64_t)256 * per_thread);
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct DpmppRow {
  float s1m, sa, A, B, C;
  bool clip, use_prev;
};

// k = *step_ptr clamped into [0, nsteps): never index outside the table, whatever the counter holds
__device__ __forceinline__ DpmppRow load_row(const float* __restrict__ tab, const int32_t* step_ptr, int nsteps, int clip_x0) {
  int k = *step_ptr;
  k = k < 0 ? 0 : (k >= nsteps ? nsteps - 1 : k);
  const float* row = tab + 5 * (size_t)k;
  DpmppRow r{row[0], row[1], row[2], row[3], row[4], clip_x0 != 0, false};
  r.use_prev = r.C != 0.f;
  return r;
}

// one element: `prev` is read only when r.use_prev; returns the new x, x0 goes to the history
__device__ __forceinline__ float dpmpp_update(float xi, float eps, float prev, const DpmppRow& r, float& x0_out) {
  float x0 = (xi - eps * r.s1m) / r.sa;
  if (r.clip) x0 = x0 < -1.f ? -1.f : (x0 > 1.f ? 1.f : x0);
  float v = r.A * xi + r.B * x0;
  if (r.use_prev) v = v + r.C * prev;
  x0_out = x0;
  return v;
}

// 4 consecutive floats from i0: one 16-byte access for a whole quad of a 16-byte aligned buffer, else element by element
__device__ __forceinline__ void ld4(const float* p, int64_t i0, int64_t n, bool wide, float (&v)[4]) {
  if (wide) {
    const float4 t = *reinterpret_cast<const float4*>(p + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i0 + e < n ? p[i0 + e] : 0.f;
  }
}
__device__ __forceinline__ void st4(float* p, int64_t i0, int64_t n, bool wide, const float (&v)[4]) {
  if (wide) {
    *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < n) p[i0 + e] = v[e];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Label-conditioned sampler: eps = (1+w)*eps_c - w*eps_u, the update, and cfg_ddim_step_kernel's bookkeeping -- x_next also goes
// to the two halves of the next UNet input, the workgroup that finishes last decrements the device-resident position and writes
// the next time vector tau[k - 1] from t_tab.  x and x_next may be the same buffer: neither is __restrict__.
// ---------------------------------------------------------------------------------------------------------------------
struct CfgDpmppStepK {
  const float* x; const float* eps_c; const float* eps_u; float* x_next; float* x0_prev;
  const float* tab; const int64_t* t_tab; int32_t* step_ptr; int nsteps; int clip_x0; float w1, w;
  int32_t* nan_flag; int64_t n; int vec;                     // vec: every float buffer is 16-byte aligned
  float* x_dup0; float* x_dup1; int64_t* t_next; int t_count; unsigned* done_counter;     // loop bookkeeping (all optional)
};
__global__ void cfg_dpmpp_step_kernel(const CfgDpmppStepK p) {
  const DpmppRow r = load_row(p.tab, p.step_ptr, p.nsteps, p.clip_x0);
  bool bad = false;
  const int64_t n = p.n, nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    const bool wide = p.vec != 0 && i0 + 3 < n;
    float xv[4], ec[4], eu[4], pv[4] = {0.f, 0.f, 0.f, 0.f}, v[4], x0[4];
    ld4(p.x, i0, n, wide, xv);
    ld4(p.eps_c, i0, n, wide, ec);
    ld4(p.eps_u, i0, n, wide, eu);
    if (r.use_prev) ld4(p.x0_prev, i0, n, wide, pv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float eps = p.w1 * ec[e] - p.w * eu[e];
      v[e] = dpmpp_update(xv[e], eps, pv[e], r, x0[e]);
      bad |= (i0 + e < n) && (v[e] != v[e]);
    }
    st4(p.x0_prev, i0, n, wide, x0);
    st4(p.x_next, i0, n, wide, v);
    if (p.x_dup0) st4(p.x_dup0, i0, n, wide, v);
    if (p.x_dup1) st4(p.x_dup1, i0, n, wide, v);
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(p.nan_flag, 1);
  }
  if (p.done_counter != nullptr) {
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicInc(p.done_counter, gridDim.x - 1) == gridDim.x - 1;   // wraps back to 0 by itself
    __syncthreads();
    if (is_last) {
      const int next = *p.step_ptr - 1;
      const int kn = next < 0 ? 0 : (next >= p.nsteps ? p.nsteps - 1 : next);
      if (p.t_count > 0) {
        const int64_t t = p.t_tab[kn];
        for (int i = threadIdx.x; i < p.t_count; i += blockDim.x) p.t_next[i] = t;
      }
      if (threadIdx.x == 0) *p.step_ptr = next;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Image-conditioned sampler, untiled: eps as the model gives it.  y and y_next may be the same buffer.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void dpmpp_step_kernel(const float* y, const float* __restrict__ eps, float* y_next, float* x0_prev,
                                  const float* __restrict__ tab, const int32_t* __restrict__ step_ptr, int nsteps, int clip_x0,
                                  int32_t* __restrict__ nan_flag, int64_t n, int vec) {
  const DpmppRow r = load_row(tab, step_ptr, nsteps, clip_x0);
  bool bad = false;
  const int64_t nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    const bool wide = vec != 0 && i0 + 3 < n;
    float yv[4], ev[4], pv[4] = {0.f, 0.f, 0.f, 0.f}, v[4], x0[4];
    ld4(y, i0, n, wide, yv);
    ld4(eps, i0, n, wide, ev);
    if (r.use_prev) ld4(x0_prev, i0, n, wide, pv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = dpmpp_update(yv[e], ev[e], pv[e], r, x0[e]);
      bad |= (i0 + e < n) && (v[e] != v[e]);
    }
    st4(x0_prev, i0, n, wide, x0);
    st4(y_next, i0, n, wide, v);
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Image-conditioned sampler over windows: tile_ddim_step_kernel's gather-form blend -- eps = sum over the covering windows (jy
// outer, jx inner, ascending; the first product initialises the sum) of (ay * ax) * eps_w[window][c][py - oy][px - ox] -- then the
// update on the full image with a full-size history, in place.  The blend reads up to nine scattered values per pixel and takes
// the linear index apart by division, as its sibling does: one float per thread and iteration.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void tile_dpmpp_step_kernel(float* y, const float* __restrict__ eps_w, float* x0_prev,
                                       const int32_t* __restrict__ first_y, const int32_t* __restrict__ count_y,
                                       const float* __restrict__ weight_y, const int32_t* __restrict__ origin_y,
                                       const int32_t* __restrict__ first_x, const int32_t* __restrict__ count_x,
                                       const float* __restrict__ weight_x, const int32_t* __restrict__ origin_x,
                                       const float* __restrict__ tab, const int32_t* __restrict__ step_ptr, int nsteps,
                                       int clip_x0, int32_t* __restrict__ nan_flag, int C, int H, int W, int ny, int nx, int th,
                                       int tw, int64_t n) {
  const DpmppRow r = load_row(tab, step_ptr, nsteps, clip_x0);
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int px = (int)(i % W);
    int64_t rr = i / W;
    const int py = (int)(rr % H);
    rr /= H;
    const int c = (int)(rr % C);
    const int64_t b = rr / C;
    // indices are clamped: a bad table gives a wrong blend, never an access outside eps_w
    const int fy = clampi(first_y[py], 0, ny - 1), cy = clampi(count_y[py], 1, 3);
    const int fx = clampi(first_x[px], 0, nx - 1), cx = clampi(count_x[px], 1, 3);
    float e = 0.f;
    for (int jy = 0; jy < cy; ++jy) {
      const int iy = min(fy + jy, ny - 1);
      const int ly = clampi(py - origin_y[iy], 0, th - 1);
      const float ay = weight_y[3 * py + jy];
      const int64_t row = ((b * ny + iy) * nx * C + c) * th + ly;      // + ix * C * th below
      for (int jx = 0; jx < cx; ++jx) {
        const int ix = min(fx + jx, nx - 1);
        const int lx = clampi(px - origin_x[ix], 0, tw - 1);
        const float t = (ay * weight_x[3 * px + jx]) * eps_w[(row + (int64_t)ix * C * th) * tw + lx];
        e = (jy | jx) == 0 ? t : e + t;
      }
    }
    float x0;
    const float v = dpmpp_update(y[i], e, r.use_prev ? x0_prev[i] : 0.f, r, x0);
    bad |= (v != v);
    x0_prev[i] = x0;
    y[i] = v;
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
  }
}

}  // namespace

extern "C" {

int hdiff_cfg_dpmpp_step(const float* x, const float* eps_c, const float* eps_u, float* x_next, float* x0_prev, const float* tab,
                         const int32_t* step_ptr, int nsteps, double w, int clip_x0, int32_t* nan_flag, int64_t n,
                         hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && eps_c && eps_u && x_next && x0_prev && tab && step_ptr && nan_flag, "cfg_dpmpp_step: null pointer");
  HDIFF_CHECK_ARG(nsteps > 0 && n > 0, "cfg_dpmpp_step: bad sizes nsteps=%d n=%lld", nsteps, (long long)n);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int vec = aligned16(x) && aligned16(eps_c) && aligned16(eps_u) && aligned16(x_next) && aligned16(x0_prev);
  CfgDpmppStepK k{x, eps_c, eps_u, x_next, x0_prev, tab, nullptr, const_cast<int32_t*>(step_ptr), nsteps, clip_x0 != 0,
                  (float)(1.0 + w), (float)w, nan_flag, n, vec, nullptr, nullptr, nullptr, 0, nullptr};
  hipLaunchKernelGGL(cfg_dpmpp_step_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("cfg_dpmpp_step_kernel");
  return HDIFF_OK;
}

int hdiff_cfg_dpmpp_step_loop(const hdiff_cfg_dpmpp_loop_desc* d, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(d && d->x && d->eps_c && d->eps_u && d->x_next && d->x0_prev && d->tab && d->step_ptr && d->nan_flag &&
                      d->done_counter, "cfg_dpmpp_step_loop: null pointer");
  HDIFF_CHECK_ARG(d->nsteps > 0 && d->n > 0 && d->t_count >= 0 && (d->t_count == 0 || (d->t_next && d->t_tab)),
                  "cfg_dpmpp_step_loop: bad sizes nsteps=%d n=%lld t_count=%d", d->nsteps, (long long)d->n, d->t_count);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int vec = aligned16(d->x) && aligned16(d->eps_c) && aligned16(d->eps_u) && aligned16(d->x_next) && aligned16(d->x0_prev) &&
                  aligned16(d->x_dup0) && aligned16(d->x_dup1);
  CfgDpmppStepK k{d->x, d->eps_c, d->eps_u, d->x_next, d->x0_prev, d->tab, d->t_tab, d->step_ptr, d->nsteps, d->clip_x0 != 0,
                  (float)(1.0 + d->w), (float)d->w, d->nan_flag, d->n, vec, d->x_dup0, d->x_dup1, d->t_next, d->t_count,
                  d->done_counter};
  hipLaunchKernelGGL(cfg_dpmpp_step_kernel, dim3(grid_for(d->n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("cfg_dpmpp_step_kernel");
  return HDIFF_OK;
}

int hdiff_dpmpp_step(const float* y, const float* eps, float* y_next, float* x0_prev, const float* tab, const int32_t* step_ptr,
                     int nsteps, int clip_x0, int32_t* nan_flag, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(y && eps && y_next && x0_prev && tab && step_ptr && nan_flag && n > 0 && nsteps > 0, "dpmpp_step: bad arguments");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int vec = aligned16(y) && aligned16(eps) && aligned16(y_next) && aligned16(x0_prev);
  hipLaunchKernelGGL(dpmpp_step_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps, y_next, x0_prev, tab,
                     step_ptr, nsteps, clip_x0, nan_flag, n, vec);
  HDIFF_CHECK_LAUNCH("dpmpp_step_kernel");
  return HDIFF_OK;
}

int hdiff_tile_dpmpp_step(float* y, const float* eps_w, float* x0_prev, const int32_t* first_y, const int32_t* count_y,
                          const float* weight_y, const int32_t* origin_y, const int32_t* first_x, const int32_t* count_x,
                          const float* weight_x, const int32_t* origin_x, const float* tab, const int32_t* step_ptr, int nsteps,
                          int clip_x0, int32_t* nan_flag, int B, int C, int H, int W, int ny, int nx, int th, int tw,
                          hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(y && eps_w && x0_prev && first_y && count_y && weight_y && origin_y && first_x && count_x && weight_x &&
                      origin_x && tab && step_ptr && nan_flag, "tile_dpmpp_step: null pointer");
  HDIFF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && th > 0 && tw > 0 && nsteps > 0 && th <= H && tw <= W &&
                      (int64_t)B * ny * nx <= 0x7fffffff,
                  "tile_dpmpp_step: bad sizes (B %d C %d H %d W %d ny %d nx %d th %d tw %d nsteps %d)", B, C, H, W, ny, nx, th, tw,
                  nsteps);
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(tile_dpmpp_step_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps_w, x0_prev, first_y,
                     count_y, weight_y, origin_y, first_x, count_x, weight_x, origin_x, tab, step_ptr, nsteps, clip_x0, nan_flag,
                     C, H, W, ny, nx, th, tw, n);
  HDIFF_CHECK_LAUNCH("tile_dpmpp_step_kernel");
  return HDIFF_OK;
}

}  // extern "C"
