// Overlapping-window DDIM sampling of the image-conditioned sampler (diffusion/Diffusion.py, `tile=`): the crop of model-sized
// windows out of the full image, and the one full-image kernel of a step -- the weighted blend of the windows' noise estimates
// fused with ddim_ops.hip's DDIM update.  Streaming kernels, one float per thread and iteration, the 64-bit linear index taken
// apart by division (not profiled on their own: a few MB per step beside the UNet's launches); compiled with -ffp-contract=off so
// that the blend and the update round like separate fp32 tensor ops.
//
// Layout (diffusion/Diffusion.py: tile_origins / tile_weights): per axis a list of window origins; window (b, iy, ix) has index
// (b * ny + iy) * nx + ix and covers rows origin_y[iy] .. + th - 1, columns origin_x[ix] .. + tw - 1.  The windows covering a
// position are a consecutive run first[p] .. first[p] + count[p] - 1 (count <= 3) with normalised weights weight[p][0..2].
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

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// out[slot][c][ly][lx] = x[b][c][oy + ly][ox + lx] of window w = min(w0 + slot, B * ny * nx - 1).  One thread per output
// element, consecutive threads along a window row: both sides of the copy are contiguous runs of tw floats.  Origins are
// clamped into [0, H - th] x [0, W - tw]: whatever the tables hold, no read leaves the tensor.
__global__ void tile_gather_kernel(const float* __restrict__ x, float* __restrict__ out, const int32_t* __restrict__ origin_y,
                                   const int32_t* __restrict__ origin_x, int C, int H, int W, int ny, int nx, int th, int tw,
                                   int w0, int n_windows, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int lx = (int)(i % tw);
    int64_t r = i / tw;
    const int ly = (int)(r % th);
    r /= th;
    const int c = (int)(r % C);
    const int slot = (int)(r / C);
    const int w = min(w0 + slot, n_windows - 1);          // a padding slot repeats the last window
    const int ix = w % nx, iy = (w / nx) % ny, b = w / (nx * ny);
    const int oy = clampi(origin_y[iy], 0, H - th), ox = clampi(origin_x[ix], 0, W - tw);
    out[i] = x[(((int64_t)b * C + c) * H + (oy + ly)) * W + (ox + lx)];
  }
}

// One step on the full image, in place: eps = sum over the covering windows (jy outer, jx inner, ascending; the first product
// initialises the sum) of (ay * ax) * eps_w[window][c][py - oy][px - ox], then ddim_step_kernel's two lines with the same
// table row.  Gather form: every pixel is written by one thread, the order of the sum is fixed -- bitwise repeatable.
// Consecutive threads run along an image row, so each window's reads are contiguous runs as well.
__global__ void tile_ddim_step_kernel(float* y, const float* __restrict__ eps_w,
                                      const int32_t* __restrict__ first_y, const int32_t* __restrict__ count_y,
                                      const float* __restrict__ weight_y, const int32_t* __restrict__ origin_y,
                                      const int32_t* __restrict__ first_x, const int32_t* __restrict__ count_x,
                                      const float* __restrict__ weight_x, const int32_t* __restrict__ origin_x,
                                      const float* __restrict__ tab, const int32_t* __restrict__ step_ptr, int nsteps,
                                      int32_t* __restrict__ nan_flag, int C, int H, int W, int ny, int nx, int th, int tw,
                                      int64_t n) {
  int k = *step_ptr;
  k = k < 0 ? 0 : (k >= nsteps ? nsteps - 1 : k);          // never index outside the table, whatever the counter holds
  const float s1m = tab[4 * k + 0], sa = tab[4 * k + 1], san = tab[4 * k + 2], c2 = tab[4 * k + 3];
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int px = (int)(i % W);
    int64_t r = i / W;
    const int py = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int64_t b = r / C;
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
    const float y0 = (y[i] - e * s1m) / sa;
    const float v = san * y0 + c2 * e;
    bad |= (v != v);
    y[i] = v;
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
  }
}

}  // namespace

extern "C" {

int hdiff_tile_gather(const float* x, float* out, const int32_t* origin_y, const int32_t* origin_x, int B, int C, int H, int W,
                      int ny, int nx, int th, int tw, int w0, int n_slots, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && out && origin_y && origin_x, "tile_gather: null pointer");
  HDIFF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && th > 0 && tw > 0 && n_slots > 0 && th <= H && tw <= W &&
                      (int64_t)B * ny * nx <= 0x7fffffff && w0 >= 0 && (int64_t)w0 < (int64_t)B * ny * nx &&
                      (int64_t)w0 + n_slots <= 0x7fffffff,
                  "tile_gather: bad sizes (B %d C %d H %d W %d ny %d nx %d th %d tw %d w0 %d n_slots %d)", B, C, H, W, ny, nx, th,
                  tw, w0, n_slots);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int64_t n = (int64_t)n_slots * C * th * tw;
  hipLaunchKernelGGL(tile_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, x, out, origin_y, origin_x, C,
                     H, W, ny, nx, th, tw, w0, B * ny * nx, n);
  HDIFF_CHECK_LAUNCH("tile_gather_kernel");
  return HDIFF_OK;
}

int hdiff_tile_ddim_step(float* y, const float* eps_w, const int32_t* first_y, const int32_t* count_y, const float* weight_y,
                         const int32_t* origin_y, const int32_t* first_x, const int32_t* count_x, const float* weight_x,
                         const int32_t* origin_x, const float* tab, const int32_t* step_ptr, int nsteps, int32_t* nan_flag,
                         int B, int C, int H, int W, int ny, int nx, int th, int tw, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(y && eps_w && first_y && count_y && weight_y && origin_y && first_x && count_x && weight_x && origin_x && tab &&
                      step_ptr && nan_flag, "tile_ddim_step: null pointer");
  HDIFF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && th > 0 && tw > 0 && nsteps > 0 && th <= H && tw <= W &&
                      (int64_t)B * ny * nx <= 0x7fffffff,
                  "tile_ddim_step: bad sizes (B %d C %d H %d W %d ny %d nx %d th %d tw %d nsteps %d)", B, C, H, W, ny, nx, th, tw,
                  nsteps);
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(tile_ddim_step_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps_w, first_y, count_y,
                     weight_y, origin_y, first_x, count_x, weight_x, origin_x, tab, step_ptr, nsteps, nan_flag, C, H, W, ny, nx,
                     th, tw, n);
  HDIFF_CHECK_LAUNCH("tile_ddim_step_kernel");
  return HDIFF_OK;
}

}  // extern "C"
