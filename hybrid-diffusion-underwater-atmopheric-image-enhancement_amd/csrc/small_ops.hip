// Small dense layers, the elementwise ops around the model (q_sample, squared error, clip, axpby, dropout masks) and the in-graph
// normal generator (gfx950).  The samplers' per-step update kernels are in sampler_step.hip.
// All HBM- or latency-bound; none of them shows up next to attention/conv at the target sizes, so they are written
// for clarity: one wave per output of a GEMV, 16-byte grid-stride loops for the elementwise passes.
#include "common.h"
#include "device.h"
#include "philox.h"

// q_sample and axpby must round exactly like the reference's separate mul / sub / add tensor ops:
// fma contraction is forbidden in this file (hipcc defaults to -ffp-contract=fast for device code, and HIP's __fmul_rn
// is a plain, contractible '*'): the Makefile compiles it with -ffp-contract=off and the pragma repeats it.
#pragma clang fp contract(off)

using namespace hdiff;

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// y[b][j] (+)= bias[j] + sum_k W[j][k] * f(x_row(b)[k]); one wave per (b, j).
// Reference: nn.Embedding gather + nn.Linear (+Swish on the input) at ModelCondition.py:38-43, 56-61, 174-181.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void linear_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                   const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ y,
                                   int B, int K, int N, int n_rows, int swish_input, int accumulate) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B * N) return;
  const int b = wave / N, j = wave - b * N;
  int64_t row = idx ? idx[b] : (int64_t)b;
  if (idx && n_rows > 0) row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);   // never fault on a bad index; the host validates
  const float* xr = x + (size_t)row * K;
  const float* wr = W + (size_t)j * K;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) {
    float v = xr[k];
    if (swish_input) v = swishf(v);
    s = fmaf(wr[k], v, s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    if (bias) s += bias[j];
    y[(size_t)b * N + j] = accumulate ? y[(size_t)b * N + j] + s : s;
  }
}

// All per-block projections of the time / label embeddings in ONE launch (ResBlock.forward, ModelCondition.py:199-200:
// h += temb_proj(temb)[:, :, None, None]; h += cond_proj(cemb)[:, :, None, None], each Swish -> Linear): job j computes
//   y_j[b][n] = (sum_k swish(x0[b][k]) w0_j[n][k] + b0_j[n]) + (sum_k swish(x1[b][k]) w1_j[n][k] + b1_j[n])
// with the SAME roundings as the two accumulating linear_rows launches it replaces (each dot product reduced on its own,
// bias added, then the two results added).  One wave per output; the job of a wave is found from the prefix table.
__global__ void linear_rows_multi_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                         const hdiff_linear_job* __restrict__ jobs, int njobs, int total_n, int B, int K) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B * total_n) return;
  const int b = wave / total_n, gn = wave - b * total_n;
  int j = 0;
  while (j + 1 < njobs && jobs[j + 1].first <= gn) ++j;          // wave-uniform, at most a few dozen jobs
  const hdiff_linear_job job = jobs[j];
  const int n = gn - job.first;
  const float* xr0 = x0 + (size_t)b * K;
  const float* wr0 = job.w0 + (size_t)n * K;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s = fmaf(wr0[k], swishf(xr0[k]), s);
  s = wave_sum(s);
  float t = 0.f;
  if (job.w1 != nullptr) {
    const float* xr1 = x1 + (size_t)b * K;
    const float* wr1 = job.w1 + (size_t)n * K;
    for (int k = lane; k < K; k += 64) t = fmaf(wr1[k], swishf(xr1[k]), t);
    t = wave_sum(t);
  }
  if (lane == 0) {
    if (job.b0) s += job.b0[n];
    if (job.w1 != nullptr) {
      if (job.b1) t += job.b1[n];
      s = s + t;
    }
    job.y[(size_t)b * job.n + n] = s;
  }
}

// The in-graph normal generator: Philox4x32-10 + Box-Muller (philox.h), 4 normals per counter.
__global__ void randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
  const int64_t nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const float4 z = normal4(seed, (uint64_t)q, offset);
    const int64_t i = q << 2;
    if (i + 3 < n) {
      *reinterpret_cast<float4*>(out + i) = z;
    } else {
      const float zz[4] = {z.x, z.y, z.z, z.w};
      for (int e = 0; e < 4 && i + e < n; ++e) out[i + e] = zz[e];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Diffusion elementwise ops (DiffusionCondition.py)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                const int64_t* __restrict__ t, const float* __restrict__ sa,
                                const float* __restrict__ sb, float* __restrict__ xt, int per_sample, int T) {
  const int b = blockIdx.y;
  int64_t tb = t[b];
  tb = tb < 0 ? 0 : (tb >= T ? T - 1 : tb);     // never fault on a bad index; the host validates (extract raises)
  const float a = sa[tb], c = sb[tb];
  const size_t base = (size_t)b * per_sample;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per_sample; i += gridDim.x * blockDim.x)
    xt[base + i] = a * x0[base + i] + c * noise[base + i];   // mul, mul, add: the reference's roundings (contraction is off)
}

__global__ void sq_err_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                              int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    out[i] = d * d;
  }
}

__global__ void clip_kernel(const float* __restrict__ x, float* __restrict__ y, float lo, float hi, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = fminf(fmaxf(x[i], lo), hi);
}
__global__ void axpby_kernel(float a, const float* __restrict__ x, float b, const float* __restrict__ y,
                             float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = y ? a * x[i] + b * y[i] : a * x[i];   // separate roundings (mul, mul, add): contraction is off in this file
}


// ---------------------------------------------------------------------------------------------------------------------
// Backward of linear_rows (autograd of nn.Linear / nn.Embedding, TrainCondition.py:60).  Tiny shapes (B <= 128,
// K, N <= 512): one thread per output, samples walked in order so the sums are reproducible.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dswishf(float v) {
  const float sg = 1.0f / (1.0f + __expf(-v));
  return sg * (1.0f + v * (1.0f - sg));
}

__global__ void linear_rows_bwd_w_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, int n_rows,
                                         const float* __restrict__ dy, float* __restrict__ dW, float* __restrict__ db, int B,
                                         int K, int N, int swish_input, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * K) return;
  const int n = i / K, k = i - n * K;
  float s = 0.f, sb = 0.f;
  for (int b = 0; b < B; ++b) {
    int64_t row = idx ? idx[b] : (int64_t)b;
    if (idx && n_rows > 0) row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);
    float v = x[(size_t)row * K + k];
    if (swish_input) v = swishf(v);
    const float g = dy[(size_t)b * N + n];
    s = fmaf(g, v, s);
    sb += g;
  }
  dW[i] = accumulate ? dW[i] + s : s;
  if (k == 0 && db) db[n] = accumulate ? db[n] + sb : sb;
}

// g = sum_n dy[n] * W[n][k]: eight independent partial sums so that eight loads are in flight per lane (a single fma chain
// waits one L2 round trip per term: 86 us for a 4 x 512 x 256 layer, 8 workgroups on the whole chip); fixed combination order.
__device__ __forceinline__ float dot_rows(const float* __restrict__ dyb, const float* __restrict__ Wk, int N, int K) {
  float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int n = 0;
  for (; n + 8 <= N; n += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = fmaf(dyb[n + j], Wk[(size_t)(n + j) * K], g[j]);
  }
  for (; n < N; ++n) g[0] = fmaf(dyb[n], Wk[(size_t)n * K], g[0]);
  return ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]));
}

__global__ void linear_rows_bwd_x_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, int n_rows,
                                         const float* __restrict__ W, const float* __restrict__ dy, float* __restrict__ dx,
                                         int B, int K, int N, int swish_input, int pad_row) {
  if (idx) {
    // gradient of the gathered table rows: one thread per column walks the samples in order (no atomics)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    for (int b = 0; b < B; ++b) {
      int64_t row = idx[b];
      if (n_rows > 0) row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);
      if (row == pad_row) continue;     // nn.Embedding(padding_idx): the padding row never receives a gradient
      float g = dot_rows(dy + (size_t)b * N, W + k, N, K);
      if (swish_input) g *= dswishf(x[(size_t)row * K + k]);
      dx[(size_t)row * K + k] += g;
    }
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i - b * K;
  float g = dot_rows(dy + (size_t)b * N, W + k, N, K);
  if (swish_input) g *= dswishf(x[i]);
  dx[i] = g;
}

// d eps_hat of the unreduced squared error: 2 * (a - b) * dloss  (DiffusionCondition.py:45)
__global__ void sq_err_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ dl,
                                  float* __restrict__ da, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    da[i] = 2.0f * (a[i] - b[i]) * dl[i];
}

// Bernoulli keep-mask scaled by 1/keep (nn.Dropout in train mode, ModelCondition.py:185), same Philox stream as randn
__global__ void dropout_mask_kernel(float* __restrict__ out, int64_t n, float keep, uint64_t seed, uint64_t offset) {
  const float scale = 1.0f / keep;
  const int64_t nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4x32_10(seed, (uint64_t)q, offset, r);
    for (int e = 0; e < 4; ++e) {
      const int64_t i = (q << 2) + e;
      if (i < n) out[i] = ((float)(r[e] >> 8) * (1.0f / 16777216.0f) < keep) ? scale : 0.f;
    }
  }
}
// The same keep decisions as ONE BIT each: bit (i & 31) of word (i >> 5) is set exactly where dropout_mask_kernel writes a non-zero
// value for element i (same Philox counter q = i / 4, same compare); unused bits of the last word are 0.  One thread per word
// (eight Philox calls), so no two threads write the same word.
__global__ void dropout_keep_bits_kernel(uint32_t* __restrict__ bits, int64_t n, float keep, uint64_t seed, uint64_t offset) {
  const int64_t nw = (n + 31) >> 5;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t word = 0;
    for (int j = 0; j < 8; ++j) {
      const int64_t q = (w << 3) + j;
      if ((q << 2) >= n) break;
      uint32_t r[4];
      philox4x32_10(seed, (uint64_t)q, offset, r);
      for (int e = 0; e < 4; ++e) {
        const int64_t i = (q << 2) + e;
        if (i < n && (float)(r[e] >> 8) * (1.0f / 16777216.0f) < keep) word |= 1u << (4 * j + e);
      }
    }
    bits[w] = word;
  }
}
__global__ void mul_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = a[i] * b[i];
}

}  // namespace

extern "C" {

int hdiff_linear_rows(const float* x, const int64_t* idx, int n_rows, const float* W, const float* bias, float* y, int B,
                      int K, int N, int swish_input, int accumulate, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && W && y, "linear_rows: null pointer");
  HDIFF_CHECK_ARG(B > 0 && K > 0 && N > 0, "linear_rows: bad sizes");
  const int waves = B * N;
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(linear_rows_kernel, dim3(cdiv(waves, 4)), dim3(256), 0, (hipStream_t)stream, x, idx, W, bias, y, B,
                     K, N, n_rows, swish_input, accumulate);
  HDIFF_CHECK_LAUNCH("linear_rows_kernel");
  return HDIFF_OK;
}

int hdiff_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                   float* xt, int B, int per_sample, int T, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x0 && noise && t && sqrt_ab && sqrt_1mab && xt, "q_sample: null pointer");
  HDIFF_CHECK_ARG(B > 0 && B <= 65535 && per_sample > 0 && T > 0, "q_sample: bad sizes B=%d per_sample=%d T=%d", B, per_sample, T);
  const int bx = cdiv(per_sample, 256) < 256 ? cdiv(per_sample, 256) : 256;
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(q_sample_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream, x0, noise, t, sqrt_ab, sqrt_1mab,
                     xt, per_sample, T);
  HDIFF_CHECK_LAUNCH("q_sample_kernel");
  return HDIFF_OK;
}

int hdiff_sq_err(const float* a, const float* b, float* out, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(a && b && out, "sq_err: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(sq_err_kernel, dim3(grid_floor_2k(n)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  HDIFF_CHECK_LAUNCH("sq_err_kernel");
  return HDIFF_OK;
}

int hdiff_linear_rows_multi(const float* x0, const float* x1, const hdiff_linear_job* jobs, int njobs, int total_n, int B,
                            int K, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x0 && jobs && njobs > 0 && total_n > 0 && B > 0 && K > 0, "linear_rows_multi: bad arguments");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int64_t waves = (int64_t)B * total_n;
  hipLaunchKernelGGL(linear_rows_multi_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x0, x1,
                     jobs, njobs, total_n, B, K);
  HDIFF_CHECK_LAUNCH("linear_rows_multi_kernel");
  return HDIFF_OK;
}

int hdiff_clip(const float* x, float* y, float lo, float hi, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && y, "clip: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(clip_kernel, dim3(grid_floor_2k(n)), dim3(256), 0, (hipStream_t)stream, x, y, lo, hi, n);
  HDIFF_CHECK_LAUNCH("clip_kernel");
  return HDIFF_OK;
}

int hdiff_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(out, "randn: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(randn_kernel, dim3(grid_floor_2k(n, 4)), dim3(256), 0, (hipStream_t)stream, out, n, seed, offset);
  HDIFF_CHECK_LAUNCH("randn_kernel");
  return HDIFF_OK;
}

int hdiff_axpby(float a, const float* x, float b, const float* y, float* out, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && out, "axpby: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_floor_2k(n)), dim3(256), 0, (hipStream_t)stream, a, x, b, y, out, n);
  HDIFF_CHECK_LAUNCH("axpby_kernel");
  return HDIFF_OK;
}

int hdiff_linear_rows_bwd(const float* x, const int64_t* idx, int n_rows, const float* W, const float* dy, float* dx,
                          float* dW, float* db, int B, int K, int N, int swish_input, int accumulate, int pad_row,
                          hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && W && dy, "linear_rows_bwd: null pointer");
  HDIFF_CHECK_ARG(B > 0 && K > 0 && N > 0, "linear_rows_bwd: bad sizes");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  if (dW)
    hipLaunchKernelGGL(linear_rows_bwd_w_kernel, dim3(cdiv(N * K, 256)), dim3(256), 0, (hipStream_t)stream, x, idx, n_rows, dy,
                       dW, db, B, K, N, swish_input, accumulate);
  if (dx)
    hipLaunchKernelGGL(linear_rows_bwd_x_kernel, dim3(cdiv(idx ? K : B * K, 256)), dim3(256), 0, (hipStream_t)stream, x, idx,
                       n_rows, W, dy, dx, B, K, N, swish_input, pad_row);
  HDIFF_CHECK_LAUNCH("linear_rows_bwd kernels");
  return HDIFF_OK;
}

int hdiff_sq_err_bwd(const float* a, const float* b, const float* dloss, float* da, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(a && b && dloss && da, "sq_err_bwd: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(sq_err_bwd_kernel, dim3(grid_floor_2k(n)), dim3(256), 0, (hipStream_t)stream, a, b, dloss, da, n);
  HDIFF_CHECK_LAUNCH("sq_err_bwd_kernel");
  return HDIFF_OK;
}

int hdiff_dropout_mask(float* out, int64_t n, float keep, uint64_t seed, uint64_t offset, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(out && keep > 0.f && keep <= 1.f, "dropout_mask: bad arguments");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_floor_2k(n, 4)), dim3(256), 0, (hipStream_t)stream, out, n, keep, seed, offset);
  HDIFF_CHECK_LAUNCH("dropout_mask_kernel");
  return HDIFF_OK;
}

int hdiff_dropout_keep_bits(uint32_t* bits, int64_t n, float keep, uint64_t seed, uint64_t offset, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(bits, "dropout_keep_bits: null pointer");
  HDIFF_CHECK_ARG(n > 0, "dropout_keep_bits: n = %lld is not positive", (long long)n);
  HDIFF_CHECK_ARG(keep > 0.f && keep <= 1.f, "dropout_keep_bits: keep = %g is outside (0, 1]", (double)keep);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(dropout_keep_bits_kernel, dim3(grid_floor_2k((n + 31) >> 5)), dim3(256), 0, (hipStream_t)stream, bits, n, keep, seed,
                     offset);
  HDIFF_CHECK_LAUNCH("dropout_keep_bits_kernel");
  return HDIFF_OK;
}

int hdiff_mul(const float* a, const float* b, float* out, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(a && b && out, "mul: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(mul_kernel, dim3(grid_floor_2k(n)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  HDIFF_CHECK_LAUNCH("mul_kernel");
  return HDIFF_OK;
}

}  // extern "C"
