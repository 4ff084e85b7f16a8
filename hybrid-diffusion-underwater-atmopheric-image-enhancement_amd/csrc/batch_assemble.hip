// One training batch of image pairs, assembled on the device from a resident uint8 cache (hdiff_amd/device_data.py), with ONE geometric
// transform per pair: random crop resized back to H x W, horizontal flip, vertical flip, quarter turns -- the same for the three
// channels and for both images of the pair.  tests/_augment_def.py is the definition the kernel is held to, bit for bit; there is no
// floating point anywhere in this file.
//
// Sample i (its index in the cache) at epoch e draws A = philox4x32_10(seed, i, 2 e) and B = philox4x32_10(seed, i, 2 e + 1):
//   hflip = A[0] < th_hflip, vflip = A[1] < th_vflip, k = rot90 ? A[2] >> 30 : 0, cropped = A[3] < th_crop        (thresholds of 2^32)
//   cropped:  ch = lo_h + ((B[0] * (H - lo_h + 1)) >> 32),  cw = clamp((2 ch W + H) / (2 H), 1, W),
//             y0 = (B[1] * (H - ch + 1)) >> 32,  x0 = (B[2] * (W - cw + 1)) >> 32;   otherwise the box is the image.
// The result is rot90(vflip(hflip(resize(box))), k).  The kernel is a gather: an output pixel inverts the quarter turn and the flips,
// then evaluates the bilinear magnification with half-pixel centres in integers: along an axis of n outputs over c source positions
// from c0, D = 2 n, num = (2 o + 1) c - n, i = floor(num / D), f = num - i D, taps c0 + clamp(i, 0, c - 1) and c0 + clamp(i + 1, 0,
// c - 1) (clamped to the BOX), weights D - f and f; a pixel is (acc + Dy Dx / 2) / (Dy Dx) in 64 bits.
//
// A thread produces kVec consecutive output x of one row for the three channels of both images: the parameters and the taps are
// computed once per pixel position, and a full, 4-byte aligned group leaves as one 32-bit store per plane; everything else (W not a
// multiple of kVec, rows that start off the alignment) is stored byte by byte.  No atomics, no shared state, no scratch: sample j of
// the output is a function of (a, b, idx[j], seed, epoch, settings) alone.  idx is read on the device and not checked there.
#include "common.h"
#include "philox.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;
constexpr int kMaxSide = 4096;

struct AssembleParams {
  const uint8_t* a;
  const uint8_t* b;
  const int64_t* idx;
  uint8_t* out_a;
  uint8_t* out_b;
  int B, H, W, groups;      // groups = ceil(W / kVec)
  uint64_t seed;
  uint32_t epoch;
  uint64_t th_hflip, th_vflip, th_crop;
  int rot90, lo_h;
};

struct Taps { int t0, t1; uint32_t f; };      // the two source positions and the weight of the second, of D = 2 n

// output position o of n, over the box [c0, c0 + c)
__device__ __forceinline__ Taps axis_taps(int o, int n, int c, int c0) {
  const int D = 2 * n;
  const int num = (2 * o + 1) * c - n;        // >= c - n > -D: the floor of a negative num / D is -1
  const int i = num >= 0 ? num / D : -1;
  Taps t;
  t.f = (uint32_t)(num - i * D);
  t.t0 = c0 + (i < 0 ? 0 : (i > c - 1 ? c - 1 : i));
  t.t1 = c0 + (i + 1 > c - 1 ? c - 1 : i + 1);
  return t;
}

__global__ __launch_bounds__(kThreads) void batch_assemble_kernel(const AssembleParams P) {
  const int H = P.H, W = P.W;
  const int64_t HW = (int64_t)H * W;
  const int64_t total = (int64_t)P.B * H * P.groups;
  const bool alias = P.a == P.b;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
    const int xg = (int)(t % P.groups);
    const int y = (int)((t / P.groups) % H);
    const int64_t j = t / ((int64_t)P.groups * H);
    const int64_t i = P.idx[j];

    uint32_t A[4], R[4];
    philox4x32_10(P.seed, (uint64_t)i, 2ull * P.epoch, A);
    const bool hflip = A[0] < P.th_hflip, vflip = A[1] < P.th_vflip, cropped = A[3] < P.th_crop;
    const int k = P.rot90 ? (int)(A[2] >> 30) : 0;
    int ch = H, cw = W, y0 = 0, x0 = 0;
    if (cropped) {
      philox4x32_10(P.seed, (uint64_t)i, 2ull * P.epoch + 1ull, R);
      ch = P.lo_h + (int)(((uint64_t)R[0] * (uint64_t)(H - P.lo_h + 1)) >> 32);
      const int64_t w = (2ll * ch * W + H) / (2ll * H);
      cw = w < 1 ? 1 : (w > W ? W : (int)w);
      y0 = (int)(((uint64_t)R[1] * (uint64_t)(H - ch + 1)) >> 32);
      x0 = (int)(((uint64_t)R[2] * (uint64_t)(W - cw + 1)) >> 32);
    }
    const uint64_t Dy = 2ull * H, Dx = 2ull * W, DD = Dy * Dx;

    const int xb = xg * kVec;
    const int nx = W - xb < kVec ? W - xb : kVec;
    Taps ty[kVec], tx[kVec];
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
      const int x = xb + (v < nx ? v : 0);      // the positions past the row's end repeat a valid one and are not stored
      int py, px;                                // where the output pixel sits before the quarter turns (H == W when k != 0)
      switch (k) {
        case 1: py = x; px = W - 1 - y; break;
        case 2: py = H - 1 - y; px = W - 1 - x; break;
        case 3: py = H - 1 - x; px = y; break;
        default: py = y; px = x; break;
      }
      const int cy = vflip ? H - 1 - py : py, cx = hflip ? W - 1 - px : px;
      ty[v] = axis_taps(cy, H, ch, y0);
      tx[v] = axis_taps(cx, W, cw, x0);
    }

    const int64_t out_row = ((int64_t)j * 3 * H + y) * W + xb;
    uint32_t packed[2][3];      // kVec pixels of each plane, the first in the low byte
#pragma unroll
    for (int img = 0; img < 2; ++img) {
      const uint8_t* src = (img ? P.b : P.a) + i * 3 * HW;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (img == 1 && alias) {
          packed[1][c] = packed[0][c];
          continue;
        }
        const uint8_t* plane = src + c * HW;
        uint32_t word = 0u;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
          const uint8_t* r0 = plane + (int64_t)ty[v].t0 * W;
          uint32_t p = r0[tx[v].t0];
          if (ty[v].f | tx[v].f) {                 // never taken for a box that is the image: its weights are all (D, 0)
            const uint8_t* r1 = plane + (int64_t)ty[v].t1 * W;
            const uint32_t fx = tx[v].f, gx = (uint32_t)Dx - fx;
            const uint64_t top = gx * p + fx * (uint32_t)r0[tx[v].t1];
            const uint64_t bot = gx * (uint32_t)r1[tx[v].t0] + fx * (uint32_t)r1[tx[v].t1];
            const uint64_t acc = (Dy - ty[v].f) * top + (uint64_t)ty[v].f * bot;
            p = (uint32_t)((acc + DD / 2) / DD);
          }
          word |= p << (8 * v);
        }
        packed[img][c] = word;
      }
    }
#pragma unroll
    for (int img = 0; img < 2; ++img) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint8_t* o = (img ? P.out_b : P.out_a) + out_row + c * HW;
        if (nx == kVec && ((uintptr_t)o & 3u) == 0) {
          *reinterpret_cast<uint32_t*>(o) = packed[img][c];
        } else {
          for (int v = 0; v < nx; ++v) o[v] = (uint8_t)(packed[img][c] >> (8 * v));
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int hdiff_batch_assemble(const uint8_t* a, const uint8_t* b, const int64_t* idx, int B, int64_t N, int H, int W, uint64_t seed,
                         uint32_t epoch, uint64_t th_hflip, uint64_t th_vflip, int rot90, uint64_t th_crop, int crop_lo_h,
                         uint8_t* out_a, uint8_t* out_b, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(a && b && idx && out_a && out_b, "batch_assemble: null pointer");
  HDIFF_CHECK_ARG(B >= 1, "batch_assemble: B = %d; a batch holds at least 1 sample", B);
  HDIFF_CHECK_ARG(N >= 1, "batch_assemble: N = %lld; the cache holds at least 1 sample", (long long)N);
  HDIFF_CHECK_ARG(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "batch_assemble: H = %d, W = %d; both sides between 1 and %d", H,
                  W, kMaxSide);
  const uint64_t one = 1ull << 32;
  HDIFF_CHECK_ARG(th_hflip <= one && th_vflip <= one && th_crop <= one,
                  "batch_assemble: thresholds %llu, %llu, %llu; a probability is at most 2^32", (unsigned long long)th_hflip,
                  (unsigned long long)th_vflip, (unsigned long long)th_crop);
  HDIFF_CHECK_ARG(crop_lo_h >= 1 && crop_lo_h <= H, "batch_assemble: crop_lo_h = %d; between 1 and H = %d", crop_lo_h, H);
  HDIFF_CHECK_ARG(!rot90 || H == W, "batch_assemble: rot90 needs square images, got H = %d, W = %d", H, W);
  HDIFF_CHECK_ARG(epoch < (1u << 31), "batch_assemble: epoch = %u; below 2^31", epoch);
  (void)hipGetLastError();
  AssembleParams P;
  P.a = a; P.b = b; P.idx = idx; P.out_a = out_a; P.out_b = out_b;
  P.B = B; P.H = H; P.W = W; P.groups = cdiv(W, kVec);
  P.seed = seed; P.epoch = epoch;
  P.th_hflip = th_hflip; P.th_vflip = th_vflip; P.th_crop = th_crop;
  P.rot90 = rot90 ? 1 : 0; P.lo_h = crop_lo_h;
  const int64_t total = (int64_t)B * H * P.groups;
  hipLaunchKernelGGL(batch_assemble_kernel, dim3(grid_ceil_8k(total)), dim3(kThreads), 0, (hipStream_t)stream, P);
  HDIFF_CHECK_LAUNCH("batch_assemble kernel");
  return HDIFF_OK;
}

}  // extern "C"
