// The per-step kernels of both samplers (gfx950): the seven update kernels -- ancestral DDPM, strided DDIM and DPM-Solver++(2M) of
// the label-conditioned sampler (DiffusionFreeGuidence/DiffusionCondition.py; classifier-free guidance and the captured loop's
// bookkeeping), DDIM and DPM-Solver++(2M) of the image-conditioned one (diffusion/Diffusion.py), untiled and over overlapping
// windows -- and what a step runs around them: the time-vector fills, the counter decrement and the window crop.  Behind them the
// three kernels of multi-sample posterior sampling: the DDIM update with its stochastic term (eta), the per-sample normal fill and
// the mean / spread over an image's samples -- and the conversion that lets a v-prediction network feed any of the image-conditioned
// updates.  All HBM- or latency-bound streaming kernels, one launch beside a whole UNet evaluation.
//
// Every update must round exactly like separate fp32 tensor ops (the reference's mul / sub / add; for the added solvers a plain
// torch program of the same lines): one rounding per written operation.  fma contraction is forbidden in this file (hipcc
// defaults to -ffp-contract=fast for device code, and HIP's __fmul_rn is a plain, contractible '*'): the Makefile compiles it with
// -ffp-contract=off and the pragma repeats it.  Clamps of x0 are written with compares: a NaN stays a NaN (torch.clamp), fminf /
// fmaxf would swallow it.
//
// The pieces the kernels share come first and exist once; each kernel keeps its own memory-access shape (the DDPM and CFG-DDIM
// steps guarded scalar accesses, the DPM++ steps ld4 / st4, the window kernels one float per thread) and each launcher its own
// grid arithmetic (grid_floor_2k / grid_ceil_8k of common.h).
#include "common.h"
#include "device.h"
#include "philox.h"

#pragma clang fp contract(off)

using namespace hdiff;

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------------------------------------------------------------------------------------------------------------
// Device side: the shared pieces
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a device-resident counter's value as an index into a table of `count` rows: never outside it, whatever the counter holds
__device__ __forceinline__ int step_index(int k, int count) { return k < 0 ? 0 : (k >= count ? count - 1 : k); }

// a time step read from device memory as an index into a table of T rows: never outside it
__device__ __forceinline__ int time_index(int64_t t, int T) { return t < 0 ? 0 : (t >= T ? T - 1 : (int)t); }

// the NaN check of the reference's per-step assert, evaluated once after the loop from this flag: one atomic per wave that saw one
__device__ __forceinline__ void flag_nan(bool bad, int32_t* nan_flag) {
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
  }
}

// classifier-free guidance: (1 + w) * eps_c - w * eps_u, w1 = (float)(1 + w) formed on the host in double
__device__ __forceinline__ float guided_eps(float w1, float eps_c, float w, float eps_u) { return w1 * eps_c - w * eps_u; }

// The noise of one step: read element by element from `injected`, or drawn a quad at a time -- Philox counter (q, k) under `seed`,
// which is elements 4q .. 4q + 3 of hdiff_randn(n, seed, offset = k).  Zeros when the step adds none.
struct StepNoise {
  bool on; const float* injected; uint64_t seed; int k;
  __device__ __forceinline__ void draw(int64_t q, float (&z)[4]) const {
    z[0] = z[1] = z[2] = z[3] = 0.f;
    if (on && injected == nullptr) {
      const float4 zz = normal4(seed, (uint64_t)q, (uint64_t)(uint32_t)k);
      z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w;
    }
  }
  __device__ __forceinline__ float at(int64_t i, float drawn) const { return on && injected != nullptr ? injected[i] : drawn; }
};

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

// Where the label-conditioned sampler's new state goes: the state buffer and, in the captured loop, the two halves of the next
// UNet input (both optional).  Element form and quad form.
struct XNext {
  float* x_next; float* dup0; float* dup1;
  __device__ __forceinline__ void store(int64_t i, float v) const {
    x_next[i] = v;
    if (dup0) dup0[i] = v;
    if (dup1) dup1[i] = v;
  }
  __device__ __forceinline__ void store4(int64_t i0, int64_t n, bool wide, const float (&v)[4]) const {
    st4(x_next, i0, n, wide, v);
    if (dup0) st4(dup0, i0, n, wide, v);
    if (dup1) st4(dup1, i0, n, wide, v);
  }
};

// Loop bookkeeping of the captured sampler step (DiffusionCondition.py:87-89: `for time_step in reversed(range(T))`,
// `t = x_t.new_ones([B]) * time_step`), run at the end of an update kernel: the workgroup that finishes LAST -- every other one
// has read *step_ptr by then -- decrements the device-resident step and writes the next step's time vector: the step itself
// (never below 0) without `t_tab`, else t_tab[step] of a table of `nsteps` entries.  The counter wraps back to 0 by itself.
// Nothing happens without a `done_counter` (the single-step entry points).
__device__ __forceinline__ void advance_loop(unsigned* done_counter, int32_t* step_ptr, int64_t* t_next, int t_count,
                                             const int64_t* t_tab, int nsteps) {
  if (done_counter == nullptr) return;
  __shared__ int is_last;
  __syncthreads();
  if (threadIdx.x == 0) is_last = atomicInc(done_counter, gridDim.x - 1) == gridDim.x - 1;
  __syncthreads();
  if (is_last) {
    const int next = *step_ptr - 1;
    if (t_count > 0) {
      const int64_t t = t_tab != nullptr ? t_tab[step_index(next, nsteps)] : (int64_t)(next < 0 ? 0 : next);
      for (int i = threadIdx.x; i < t_count; i += blockDim.x) t_next[i] = t;
    }
    if (threadIdx.x == 0) *step_ptr = next;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Time vectors and the counter of the image-conditioned sampler's step (its update kernels carry no bookkeeping)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void fill_t_kernel(int64_t* t, const int32_t* step_ptr, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) t[i] = (int64_t)(*step_ptr);
}
__global__ void fill_from_table_kernel(int64_t* dst, const int32_t* __restrict__ table, const int32_t* __restrict__ idx,
                                       int table_len, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = step_index(*idx, table_len);
  if (i < n) dst[i] = (int64_t)table[k];
}
__global__ void step_decrement_kernel(int32_t* step_ptr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step_ptr = *step_ptr - 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Ancestral DDPM step with classifier-free guidance (DiffusionCondition.py:78-79, 95):
//   x_next = coeff1[t]*x - coeff2[t]*((1+w)*eps_c - w*eps_u) + sigma[t]*z
// in the reference's order, so that the CPU oracle and this kernel round identically given identical eps.
// x and x_next may be the same buffer (the sampler updates in place): neither is __restrict__.
// ---------------------------------------------------------------------------------------------------------------------
struct DdpmStepK {
  const float* x; const float* eps_c; const float* eps_u; const float* noise; float* x_next;
  const float* coeff1; const float* coeff2; const float* sigma;
  int32_t* step_ptr; int T; float w1, w; uint64_t seed; int32_t* nan_flag; int64_t n;
  float* x_dup0; float* x_dup1; int64_t* t_next; int t_count; unsigned* done_counter;     // loop bookkeeping (all optional)
};
__global__ void ddpm_step_kernel(const DdpmStepK p) {
  const int step = step_index(*p.step_ptr, p.T);
  const float c1 = p.coeff1[step], c2 = p.coeff2[step], sg = p.sigma[step];
  const bool add_noise = step > 0;
  const StepNoise noise{add_noise, p.noise, p.seed, step};
  const float* x = p.x;
  const XNext out{p.x_next, p.x_dup0, p.x_dup1};
  bool bad = false;
  const int64_t n = p.n, nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    float z[4];
    noise.draw(q, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = i0 + e;
      if (i < n) {
        const float eps = guided_eps(p.w1, p.eps_c[i], p.w, p.eps_u[i]);
        const float mean = c1 * x[i] - c2 * eps;
        const float v = add_noise ? mean + sg * noise.at(i, z[e]) : mean;
        bad |= (v != v);
        out.store(i, v);
      }
    }
  }
  flag_nan(bad, p.nan_flag);
  advance_loop(p.done_counter, p.step_ptr, p.t_next, p.t_count, nullptr, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// One strided DDIM step with classifier-free guidance (Song et al. 2021, eq. 12, on a sub-sequence tau of the T training steps):
//   eps = (1+w)*eps_c - w*eps_u ; x0 = (x - eps*s1m) / sa ; [x0 = clamp(x0, -1, 1) ; eps = (x - sa*x0) / s1m]
//   v = san*x0 + c2*eps (+ sigma*z when k > 0 and sigma > 0),   tab[k] = {s1m, sa, san, c2, sigma} of position k in tau
// The counter is the position k, the next time vector tau[k - 1] from t_tab.  x and x_next may be the same buffer.
// ---------------------------------------------------------------------------------------------------------------------
struct CfgDdimStepK {
  const float* x; const float* eps_c; const float* eps_u; const float* noise; float* x_next;
  const float* tab; const int64_t* t_tab; int32_t* step_ptr; int nsteps; int clip_x0; float w1, w; uint64_t seed;
  int32_t* nan_flag; int64_t n;
  float* x_dup0; float* x_dup1; int64_t* t_next; int t_count; unsigned* done_counter;     // loop bookkeeping (all optional)
};
__global__ void cfg_ddim_step_kernel(const CfgDdimStepK p) {
  const int k = step_index(*p.step_ptr, p.nsteps);
  const float* row = p.tab + 5 * (size_t)k;
  const float s1m = row[0], sa = row[1], san = row[2], c2 = row[3], sg = row[4];
  const bool add_noise = k > 0 && sg > 0.f;
  const StepNoise noise{add_noise, p.noise, p.seed, k};
  const bool clip = p.clip_x0 != 0;
  const float* x = p.x;
  const XNext out{p.x_next, p.x_dup0, p.x_dup1};
  bool bad = false;
  const int64_t n = p.n, nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    float z[4];
    noise.draw(q, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = i0 + e;
      if (i < n) {
        const float xi = x[i];
        float eps = guided_eps(p.w1, p.eps_c[i], p.w, p.eps_u[i]);
        float x0 = (xi - eps * s1m) / sa;
        if (clip) {
          x0 = x0 < -1.f ? -1.f : (x0 > 1.f ? 1.f : x0);
          eps = (xi - sa * x0) / s1m;
        }
        float v = san * x0 + c2 * eps;
        if (add_noise) v = v + sg * noise.at(i, z[e]);
        bad |= (v != v);
        out.store(i, v);
      }
    }
  }
  flag_nan(bad, p.nan_flag);
  advance_loop(p.done_counter, p.step_ptr, p.t_next, p.t_count, p.t_tab, p.nsteps);
}

// ---------------------------------------------------------------------------------------------------------------------
// DPM-Solver++(2M) (Lu et al. 2022, data-prediction form, multistep), the update of three kernels:
//   x0 = (x - eps * s1m) / sa ; [x0 = clamp(x0, -1, 1)] ; v = A * x + B * x0 ; [C != 0:  v = v + C * x0_prev] ; x0_prev = x0 ; x = v
// tab[k] = {s1m, sa, A, B, C} of position k in the time-step list (dpmpp_table).  HBM traffic: the DDIM update's plus one read and
// one write of the x0 history (8 bytes per element).  The branch on C is uniform per launch and is not an optimisation: at the
// first step of a loop (and at the closing one) C is 0 and x0_prev holds whatever the last call left, which must not be read
// into the sum (0 * NaN is NaN).  Every element is read and written by the same thread, so x, x_next and the history update in
// place.
// ---------------------------------------------------------------------------------------------------------------------
struct DpmppRow {
  float s1m, sa, A, B, C;
  bool clip, use_prev;
};
__device__ __forceinline__ DpmppRow load_row(const float* __restrict__ tab, const int32_t* step_ptr, int nsteps, int clip_x0) {
  const float* row = tab + 5 * (size_t)step_index(*step_ptr, nsteps);
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

// Label-conditioned sampler: guidance, the update and the strided DDIM step's bookkeeping.  x and x_next may be the same buffer.
struct CfgDpmppStepK {
  const float* x; const float* eps_c; const float* eps_u; float* x_next; float* x0_prev;
  const float* tab; const int64_t* t_tab; int32_t* step_ptr; int nsteps; int clip_x0; float w1, w;
  int32_t* nan_flag; int64_t n; int vec;                     // vec: every float buffer is 16-byte aligned
  float* x_dup0; float* x_dup1; int64_t* t_next; int t_count; unsigned* done_counter;     // loop bookkeeping (all optional)
};
__global__ void cfg_dpmpp_step_kernel(const CfgDpmppStepK p) {
  const DpmppRow r = load_row(p.tab, p.step_ptr, p.nsteps, p.clip_x0);
  const XNext out{p.x_next, p.x_dup0, p.x_dup1};
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
      v[e] = dpmpp_update(xv[e], guided_eps(p.w1, ec[e], p.w, eu[e]), pv[e], r, x0[e]);
      bad |= (i0 + e < n) && (v[e] != v[e]);
    }
    st4(p.x0_prev, i0, n, wide, x0);
    out.store4(i0, n, wide, v);
  }
  flag_nan(bad, p.nan_flag);
  advance_loop(p.done_counter, p.step_ptr, p.t_next, p.t_count, p.t_tab, p.nsteps);
}

// ---------------------------------------------------------------------------------------------------------------------
// Image-conditioned sampler, untiled: eps as the model gives it.  y and y_next may be the same buffer (the sampler updates in
// place): neither is __restrict__.
// ---------------------------------------------------------------------------------------------------------------------
// Diffusion.py:259-263 with eta = 0:
//   y0 = (y - eps * sqrt(1 - at)) / sqrt(at) ;  y' = sqrt(at_next) * y0 + c2 * eps        (c1 * randn = 0 is dropped: x + 0 = x)
// tab[k] = {sqrt(1 - at), sqrt(at), sqrt(at_next), c2} of DDIM step k, formed on the host with the reference's fp32 ops.
struct DdimRow { float s1m, sa, san, c2; };
__device__ __forceinline__ DdimRow load_ddim_row(const float* __restrict__ tab, const int32_t* step_ptr, int nsteps) {
  const int k = step_index(*step_ptr, nsteps);
  return {tab[4 * k + 0], tab[4 * k + 1], tab[4 * k + 2], tab[4 * k + 3]};
}
__device__ __forceinline__ float ddim_update(float y, float eps, const DdimRow& r) {
  const float y0 = (y - eps * r.s1m) / r.sa;
  return r.san * y0 + r.c2 * eps;
}

__global__ void ddim_step_kernel(const float* y, const float* __restrict__ eps, float* y_next,
                                 const float* __restrict__ tab, const int32_t* __restrict__ step_ptr, int nsteps,
                                 int32_t* __restrict__ nan_flag, int64_t n) {
  const DdimRow r = load_ddim_row(tab, step_ptr, nsteps);
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float e = eps[i];
    const float v = ddim_update(y[i], e, r);
    bad |= (v != v);
    y_next[i] = v;
  }
  flag_nan(bad, nan_flag);
}

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
  flag_nan(bad, nan_flag);
}

// ---------------------------------------------------------------------------------------------------------------------
// Multi-sample posterior sampling of the image-conditioned sampler (diffusion/Diffusion.py, `posterior` and `eta=`): a batch is
// `rows` samples of n_per floats, and every sample draws ALL its noise from a Philox stream of its own -- seeds[row], quads counted
// WITHIN the row -- so that a sample's numbers depend on neither its place in the batch nor on the batch's size.
// ---------------------------------------------------------------------------------------------------------------------
// row r = hdiff_randn(n_per, seeds[r], offset), bit for bit: quad q of a row is Philox counter (q, offset) under the row's seed; the
// last quad of a row with n_per % 4 != 0 is partly used and the next row starts a fresh one.  `wide`: out is 16-byte aligned and
// n_per % 4 == 0, so every quad of every row is one aligned 16-byte store.
__global__ void randn_rows_kernel(float* __restrict__ out, int64_t n_per, int64_t nq_row, int64_t nq,
                                  const uint64_t* __restrict__ seeds, uint64_t offset, int wide) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nq; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = g / nq_row, q = g - r * nq_row;
    const float4 zz = normal4(seeds[r], (uint64_t)q, offset);
    const float z[4] = {zz.x, zz.y, zz.z, zz.w};
    st4(out + r * n_per, q << 2, n_per, wide != 0, z);
  }
}

// Diffusion.py:259-267 with the reference's stochastic term kept (eta != 0 there):
//   y0 = (y - eps * sqrt(1 - at)) / sqrt(at) ;  y' = ((sqrt(at_next) * y0) + (c1 * z)) + (c2 * eps)
// tab[k] = {sqrt(1 - at), sqrt(at), sqrt(at_next), c1, c2}.  z is read from `noise` or drawn per row: elements 4q .. 4q + 3 of
// hdiff_randn(n_per, seeds[row], offset = k), StepNoise's convention.  The noise is added at every step, the last included, as the
// reference's line does.  Every element is read and written by one thread: y and y_next may be the same buffer.
__global__ void ddim_eta_step_kernel(const float* y, const float* __restrict__ eps, const float* __restrict__ noise, float* y_next,
                                     const float* __restrict__ tab, const uint64_t* __restrict__ seeds, int64_t n_per,
                                     int64_t nq_row, int64_t nq, const int32_t* __restrict__ step_ptr, int nsteps,
                                     int32_t* __restrict__ nan_flag, int vec) {
  const int k = step_index(*step_ptr, nsteps);
  const float* row = tab + 5 * (size_t)k;
  const float s1m = row[0], sa = row[1], san = row[2], c1 = row[3], c2 = row[4];
  bool bad = false;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nq; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = g / nq_row, q = g - r * nq_row, i0 = q << 2, base = r * n_per;
    const bool wide = vec != 0;
    float yv[4], ev[4], z[4], v[4];
    ld4(y + base, i0, n_per, wide, yv);
    ld4(eps + base, i0, n_per, wide, ev);
    if (noise != nullptr) {
      ld4(noise + base, i0, n_per, wide, z);
    } else {
      const float4 zz = normal4(seeds[r], (uint64_t)q, (uint64_t)(uint32_t)k);
      z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float y0 = (yv[e] - ev[e] * s1m) / sa;
      v[e] = ((san * y0) + (c1 * z[e])) + (c2 * ev[e]);
      bad |= (i0 + e < n_per) && (v[e] != v[e]);
    }
    st4(y_next + base, i0, n_per, wide, v);
  }
  flag_nan(bad, nan_flag);
}

// ---------------------------------------------------------------------------------------------------------------------
// A v-prediction network in front of the image-conditioned sampler's updates (Salimans & Ho 2022): the model's output becomes the
// noise estimate every update kernel above and below takes,
//   out = a * out + s * y,   a = sa_tab[t[b]], s = s1m_tab[t[b]]  of the row's own time step
// in place, one launch behind the UNet, two products and one sum rounded apart.  The tables are sqrt(alphas_bar) and
// sqrt(1 - alphas_bar) at the index the model is CALLED with -- the trainer's q_sample indexing, not the DDIM loop's
// alphas_bar[t + 1].  The B rows of n_per floats are walked as one run of quads: a quad may straddle two rows (n_per = 3 H W is odd
// for odd sizes), so the row is tracked per element; 16-byte accesses on aligned buffers, the last quad of the run element by
// element.  HBM traffic: 12 bytes per element.  An element's result depends on its own two inputs alone.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void v_to_eps_kernel(float* out, const float* __restrict__ y, const int64_t* __restrict__ t,
                                const float* __restrict__ sa_tab, const float* __restrict__ s1m_tab, int T, int B, int64_t n_per,
                                int64_t n, int vec) {
  const int64_t nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    const bool wide = vec != 0 && i0 + 3 < n;
    float ov[4], yv[4], v[4];
    ld4(out, i0, n, wide, ov);
    ld4(y, i0, n, wide, yv);
    int64_t b = i0 / n_per, rem = i0 - b * n_per;
    int k = time_index(t[b], T);
    float a = sa_tab[k], s = s1m_tab[k];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (rem == n_per) {                           // the quad runs on into the next row (past the last one: values never stored)
        rem = 0;
        b = b + 1 < B ? b + 1 : B - 1;
        k = time_index(t[b], T);
        a = sa_tab[k];
        s = s1m_tab[k];
      }
      v[e] = a * ov[e] + s * yv[e];
      ++rem;
    }
    st4(out, i0, n, wide, v);
  }
}

// Mean and spread of the K samples of every image, samples [B][K][n] -> mean, std [B][n].  Per element, in double, in replica order:
//   m = (x_0 + x_1 + ... ) / K ;  std = sqrt(((x_0 - m)^2 + (x_1 - m)^2 + ...) / (K - 1)), exactly 0 for K = 1
// each rounded once to fp32.  One thread per element, K coalesced reads twice over (the second pass hits the cache); no atomics, the
// order of the sums is fixed.  An element's result depends on its own K values alone.
__global__ void sample_stats_kernel(const float* __restrict__ x, int K, int64_t n, int64_t total, float* __restrict__ mean,
                                    float* __restrict__ sd) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / n, j = i - b * n;
    const float* p = x + b * K * n + j;
    double s = (double)p[0];
    for (int k = 1; k < K; ++k) s = s + (double)p[(int64_t)k * n];
    const double m = s / (double)K;
    double sq = 0.0;
    if (K > 1) {
      const double d0 = (double)p[0] - m;
      sq = d0 * d0;
      for (int k = 1; k < K; ++k) {
        const double d = (double)p[(int64_t)k * n] - m;
        sq = sq + d * d;
      }
      sq = sqrt(sq / (double)(K - 1));
    }
    mean[i] = (float)m;
    sd[i] = (float)sq;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Image-conditioned sampler over overlapping windows (diffusion/Diffusion.py, `tile=`): the crop of model-sized windows out of
// the full image, and the one full-image kernel of a step -- the weighted blend of the windows' noise estimates fused with the
// update.  One float per thread and iteration, the 64-bit linear index taken apart by division (not profiled on their own: a few
// MB per step beside the UNet's launches).
//
// Layout (tile_origins / tile_weights): per axis a list of window origins; window (b, iy, ix) has index (b * ny + iy) * nx + ix
// and covers rows origin_y[iy] .. + th - 1, columns origin_x[ix] .. + tw - 1.  The windows covering a position are a consecutive
// run first[p] .. first[p] + count[p] - 1 (count <= 3) with normalised weights weight[p][0..2].
// ---------------------------------------------------------------------------------------------------------------------
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

// The blend of element i of the full image [B][C][H][W]: eps = sum over the covering windows (jy outer, jx inner, ascending; the
// first product initialises the sum) of (ay * ax) * eps_w[window][c][py - oy][px - ox].  Gather form: every pixel is formed by one
// thread, the order of the sum is fixed -- bitwise repeatable.  Consecutive threads run along an image row, so each window's
// reads are contiguous runs as well.  Indices are clamped: a bad table gives a wrong blend, never an access outside eps_w.
struct TileBlend {
  const int32_t* first_y; const int32_t* count_y; const float* weight_y; const int32_t* origin_y;
  const int32_t* first_x; const int32_t* count_x; const float* weight_x; const int32_t* origin_x;
  int C, H, W, ny, nx, th, tw;
  __device__ __forceinline__ float eps_at(const float* __restrict__ eps_w, int64_t i) const {
    const int px = (int)(i % W);
    int64_t r = i / W;
    const int py = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int64_t b = r / C;
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
    return e;
  }
};

// One DDIM step on the full image, in place: the blend, then ddim_step_kernel's update with the same table row.
__global__ void tile_ddim_step_kernel(float* y, const float* __restrict__ eps_w,
                                      const int32_t* __restrict__ first_y, const int32_t* __restrict__ count_y,
                                      const float* __restrict__ weight_y, const int32_t* __restrict__ origin_y,
                                      const int32_t* __restrict__ first_x, const int32_t* __restrict__ count_x,
                                      const float* __restrict__ weight_x, const int32_t* __restrict__ origin_x,
                                      const float* __restrict__ tab, const int32_t* __restrict__ step_ptr, int nsteps,
                                      int32_t* __restrict__ nan_flag, int C, int H, int W, int ny, int nx, int th, int tw,
                                      int64_t n) {
  const DdimRow r = load_ddim_row(tab, step_ptr, nsteps);
  const TileBlend blend{first_y, count_y, weight_y, origin_y, first_x, count_x, weight_x, origin_x, C, H, W, ny, nx, th, tw};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = ddim_update(y[i], blend.eps_at(eps_w, i), r);
    bad |= (v != v);
    y[i] = v;
  }
  flag_nan(bad, nan_flag);
}

// The same with the DPM-Solver++(2M) update and a full-size history, in place.
__global__ void tile_dpmpp_step_kernel(float* y, const float* __restrict__ eps_w, float* x0_prev,
                                       const int32_t* __restrict__ first_y, const int32_t* __restrict__ count_y,
                                       const float* __restrict__ weight_y, const int32_t* __restrict__ origin_y,
                                       const int32_t* __restrict__ first_x, const int32_t* __restrict__ count_x,
                                       const float* __restrict__ weight_x, const int32_t* __restrict__ origin_x,
                                       const float* __restrict__ tab, const int32_t* __restrict__ step_ptr, int nsteps,
                                       int clip_x0, int32_t* __restrict__ nan_flag, int C, int H, int W, int ny, int nx, int th,
                                       int tw, int64_t n) {
  const DpmppRow r = load_row(tab, step_ptr, nsteps, clip_x0);
  const TileBlend blend{first_y, count_y, weight_y, origin_y, first_x, count_x, weight_x, origin_x, C, H, W, ny, nx, th, tw};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float e = blend.eps_at(eps_w, i);
    float x0;
    const float v = dpmpp_update(y[i], e, r.use_prev ? x0_prev[i] : 0.f, r, x0);
    bad |= (v != v);
    x0_prev[i] = x0;
    y[i] = v;
  }
  flag_nan(bad, nan_flag);
}

// the argument check of the two window step launchers; `op` prefixes the message
int check_tile_step(const char* op, bool pointers, int B, int C, int H, int W, int ny, int nx, int th, int tw, int nsteps) {
  HDIFF_CHECK_ARG(pointers, "%s: null pointer", op);
  HDIFF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && th > 0 && tw > 0 && nsteps > 0 && th <= H && tw <= W &&
                      (int64_t)B * ny * nx <= 0x7fffffff,
                  "%s: bad sizes (B %d C %d H %d W %d ny %d nx %d th %d tw %d nsteps %d)", op, B, C, H, W, ny, nx, th, tw, nsteps);
  return HDIFF_OK;
}

}  // namespace

extern "C" {

int hdiff_fill_t(int64_t* t, const int32_t* step_ptr, int B, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(t && step_ptr && B > 0, "fill_t: bad arguments");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(fill_t_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, t, step_ptr, B);
  HDIFF_CHECK_LAUNCH("fill_t_kernel");
  return HDIFF_OK;
}

int hdiff_fill_from_table(int64_t* dst, const int32_t* table, const int32_t* idx, int table_len, int n,
                          hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(dst && table && idx && n > 0 && table_len > 0, "fill_from_table: bad arguments");
  (void)hipGetLastError();
  hipLaunchKernelGGL(fill_from_table_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, dst, table, idx, table_len,
                     n);
  HDIFF_CHECK_LAUNCH("fill_from_table_kernel");
  return HDIFF_OK;
}

int hdiff_step_decrement(int32_t* step_ptr, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(step_ptr, "step_decrement: null pointer");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(step_decrement_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_ptr);
  HDIFF_CHECK_LAUNCH("step_decrement_kernel");
  return HDIFF_OK;
}

int hdiff_ddpm_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, float* x_next,
                    const float* coeff1, const float* coeff2, const float* sigma, const int32_t* step_ptr, int T, double w,
                    uint64_t seed, int32_t* nan_flag, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && eps_c && eps_u && x_next && coeff1 && coeff2 && sigma && step_ptr && nan_flag,
                  "ddpm_step: null pointer");
  HDIFF_CHECK_ARG(T > 0 && n > 0, "ddpm_step: bad sizes T=%d n=%lld", T, (long long)n);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  DdpmStepK k{x, eps_c, eps_u, noise, x_next, coeff1, coeff2, sigma, const_cast<int32_t*>(step_ptr), T, (float)(1.0 + w),
              (float)w, seed, nan_flag, n, nullptr, nullptr, nullptr, 0, nullptr};
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_floor_2k(n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("ddpm_step_kernel");
  return HDIFF_OK;
}

int hdiff_ddpm_step_loop(const hdiff_ddpm_loop_desc* d, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(d && d->x && d->eps_c && d->eps_u && d->x_next && d->coeff1 && d->coeff2 && d->sigma && d->step_ptr &&
                      d->nan_flag && d->done_counter,
                  "ddpm_step_loop: null pointer");
  HDIFF_CHECK_ARG(d->T > 0 && d->n > 0 && d->t_count >= 0 && (d->t_count == 0 || d->t_next),
                  "ddpm_step_loop: bad sizes T=%d n=%lld t_count=%d", d->T, (long long)d->n, d->t_count);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  DdpmStepK k{d->x, d->eps_c, d->eps_u, d->noise, d->x_next, d->coeff1, d->coeff2, d->sigma, d->step_ptr, d->T,
              (float)(1.0 + d->w), (float)d->w, d->seed, d->nan_flag, d->n, d->x_dup0, d->x_dup1, d->t_next, d->t_count,
              d->done_counter};
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_floor_2k(d->n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("ddpm_step_kernel");
  return HDIFF_OK;
}

int hdiff_cfg_ddim_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, float* x_next,
                        const float* tab, const int32_t* step_ptr, int nsteps, double w, int clip_x0, uint64_t seed,
                        int32_t* nan_flag, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && eps_c && eps_u && x_next && tab && step_ptr && nan_flag, "cfg_ddim_step: null pointer");
  HDIFF_CHECK_ARG(nsteps > 0 && n > 0, "cfg_ddim_step: bad sizes nsteps=%d n=%lld", nsteps, (long long)n);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  CfgDdimStepK k{x, eps_c, eps_u, noise, x_next, tab, nullptr, const_cast<int32_t*>(step_ptr), nsteps, clip_x0 != 0,
                 (float)(1.0 + w), (float)w, seed, nan_flag, n, nullptr, nullptr, nullptr, 0, nullptr};
  hipLaunchKernelGGL(cfg_ddim_step_kernel, dim3(grid_floor_2k(n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("cfg_ddim_step_kernel");
  return HDIFF_OK;
}

int hdiff_cfg_ddim_step_loop(const hdiff_cfg_ddim_loop_desc* d, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(d && d->x && d->eps_c && d->eps_u && d->x_next && d->tab && d->step_ptr && d->nan_flag && d->done_counter,
                  "cfg_ddim_step_loop: null pointer");
  HDIFF_CHECK_ARG(d->nsteps > 0 && d->n > 0 && d->t_count >= 0 && (d->t_count == 0 || (d->t_next && d->t_tab)),
                  "cfg_ddim_step_loop: bad sizes nsteps=%d n=%lld t_count=%d", d->nsteps, (long long)d->n, d->t_count);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  CfgDdimStepK k{d->x, d->eps_c, d->eps_u, d->noise, d->x_next, d->tab, d->t_tab, d->step_ptr, d->nsteps, d->clip_x0 != 0,
                 (float)(1.0 + d->w), (float)d->w, d->seed, d->nan_flag, d->n, d->x_dup0, d->x_dup1, d->t_next, d->t_count,
                 d->done_counter};
  hipLaunchKernelGGL(cfg_ddim_step_kernel, dim3(grid_floor_2k(d->n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("cfg_ddim_step_kernel");
  return HDIFF_OK;
}

int hdiff_cfg_dpmpp_step(const float* x, const float* eps_c, const float* eps_u, float* x_next, float* x0_prev, const float* tab,
                         const int32_t* step_ptr, int nsteps, double w, int clip_x0, int32_t* nan_flag, int64_t n,
                         hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(x && eps_c && eps_u && x_next && x0_prev && tab && step_ptr && nan_flag, "cfg_dpmpp_step: null pointer");
  HDIFF_CHECK_ARG(nsteps > 0 && n > 0, "cfg_dpmpp_step: bad sizes nsteps=%d n=%lld", nsteps, (long long)n);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int vec = aligned16(x) && aligned16(eps_c) && aligned16(eps_u) && aligned16(x_next) && aligned16(x0_prev);
  CfgDpmppStepK k{x, eps_c, eps_u, x_next, x0_prev, tab, nullptr, const_cast<int32_t*>(step_ptr), nsteps, clip_x0 != 0,
                  (float)(1.0 + w), (float)w, nan_flag, n, vec, nullptr, nullptr, nullptr, 0, nullptr};
  hipLaunchKernelGGL(cfg_dpmpp_step_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, k);
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
  hipLaunchKernelGGL(cfg_dpmpp_step_kernel, dim3(grid_ceil_8k(d->n, 4)), dim3(256), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("cfg_dpmpp_step_kernel");
  return HDIFF_OK;
}

int hdiff_ddim_step(const float* y, const float* eps, float* y_next, const float* tab, const int32_t* step_ptr, int nsteps,
                    int32_t* nan_flag, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(y && eps && y_next && tab && step_ptr && nan_flag && n > 0 && nsteps > 0, "ddim_step: bad arguments");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(ddim_step_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps, y_next, tab, step_ptr,
                     nsteps, nan_flag, n);
  HDIFF_CHECK_LAUNCH("ddim_step_kernel");
  return HDIFF_OK;
}

int hdiff_dpmpp_step(const float* y, const float* eps, float* y_next, float* x0_prev, const float* tab, const int32_t* step_ptr,
                     int nsteps, int clip_x0, int32_t* nan_flag, int64_t n, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(y && eps && y_next && x0_prev && tab && step_ptr && nan_flag && n > 0 && nsteps > 0, "dpmpp_step: bad arguments");
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int vec = aligned16(y) && aligned16(eps) && aligned16(y_next) && aligned16(x0_prev);
  hipLaunchKernelGGL(dpmpp_step_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps, y_next, x0_prev, tab,
                     step_ptr, nsteps, clip_x0, nan_flag, n, vec);
  HDIFF_CHECK_LAUNCH("dpmpp_step_kernel");
  return HDIFF_OK;
}

int hdiff_randn_rows(float* out, int rows, int64_t n_per, const uint64_t* seeds, uint64_t offset, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(out && seeds, "randn_rows: null pointer");
  HDIFF_CHECK_ARG(rows > 0 && n_per > 0, "randn_rows: bad sizes rows=%d n_per=%lld", rows, (long long)n_per);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int64_t nq_row = (n_per + 3) >> 2, nq = nq_row * rows;
  const int wide = aligned16(out) && (n_per & 3) == 0;
  hipLaunchKernelGGL(randn_rows_kernel, dim3(grid_ceil_8k(nq)), dim3(256), 0, (hipStream_t)stream, out, n_per, nq_row, nq, seeds,
                     offset, wide);
  HDIFF_CHECK_LAUNCH("randn_rows_kernel");
  return HDIFF_OK;
}

int hdiff_ddim_eta_step(const float* y, const float* eps, const float* noise, float* y_next, const float* tab,
                        const uint64_t* seeds, int64_t n_per, const int32_t* step_ptr, int nsteps, int32_t* nan_flag, int rows,
                        hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(y && eps && y_next && tab && step_ptr && nan_flag && (noise || seeds), "ddim_eta_step: null pointer");
  HDIFF_CHECK_ARG(rows > 0 && n_per > 0 && nsteps > 0, "ddim_eta_step: bad sizes rows=%d n_per=%lld nsteps=%d", rows,
                  (long long)n_per, nsteps);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int64_t nq_row = (n_per + 3) >> 2, nq = nq_row * rows;
  const int vec = aligned16(y) && aligned16(eps) && aligned16(noise) && aligned16(y_next) && (n_per & 3) == 0;
  hipLaunchKernelGGL(ddim_eta_step_kernel, dim3(grid_ceil_8k(nq)), dim3(256), 0, (hipStream_t)stream, y, eps, noise, y_next, tab,
                     seeds, n_per, nq_row, nq, step_ptr, nsteps, nan_flag, vec);
  HDIFF_CHECK_LAUNCH("ddim_eta_step_kernel");
  return HDIFF_OK;
}

int hdiff_v_to_eps(float* out, const float* y, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab, int T, int B,
                   int64_t n_per, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(out && y && t && sqrt_ab && sqrt_1mab, "v_to_eps: null pointer");
  HDIFF_CHECK_ARG(T > 0 && B > 0 && n_per > 0, "v_to_eps: bad sizes T=%d B=%d n_per=%lld", T, B, (long long)n_per);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int64_t n = (int64_t)B * n_per;
  const int vec = aligned16(out) && aligned16(y);
  hipLaunchKernelGGL(v_to_eps_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, out, y, t, sqrt_ab, sqrt_1mab, T,
                     B, n_per, n, vec);
  HDIFF_CHECK_LAUNCH("v_to_eps_kernel");
  return HDIFF_OK;
}

int hdiff_sample_stats(const float* samples, int B, int K, int64_t n, float* mean, float* std, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(samples && mean && std, "sample_stats: null pointer");
  HDIFF_CHECK_ARG(B > 0 && K > 0 && n > 0, "sample_stats: bad sizes B=%d K=%d n=%lld", B, K, (long long)n);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  const int64_t total = (int64_t)B * n;
  hipLaunchKernelGGL(sample_stats_kernel, dim3(grid_ceil_8k(total)), dim3(256), 0, (hipStream_t)stream, samples, K, n, total, mean,
                     std);
  HDIFF_CHECK_LAUNCH("sample_stats_kernel");
  return HDIFF_OK;
}

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
  hipLaunchKernelGGL(tile_gather_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, x, out, origin_y, origin_x, C,
                     H, W, ny, nx, th, tw, w0, B * ny * nx, n);
  HDIFF_CHECK_LAUNCH("tile_gather_kernel");
  return HDIFF_OK;
}

int hdiff_tile_ddim_step(float* y, const float* eps_w, const int32_t* first_y, const int32_t* count_y, const float* weight_y,
                         const int32_t* origin_y, const int32_t* first_x, const int32_t* count_x, const float* weight_x,
                         const int32_t* origin_x, const float* tab, const int32_t* step_ptr, int nsteps, int32_t* nan_flag,
                         int B, int C, int H, int W, int ny, int nx, int th, int tw, hdiff_stream_t stream) {
  if (const int rc = check_tile_step("tile_ddim_step",
                                     y && eps_w && first_y && count_y && weight_y && origin_y && first_x && count_x && weight_x &&
                                         origin_x && tab && step_ptr && nan_flag,
                                     B, C, H, W, ny, nx, th, tw, nsteps))
    return rc;
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(tile_ddim_step_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps_w, first_y, count_y,
                     weight_y, origin_y, first_x, count_x, weight_x, origin_x, tab, step_ptr, nsteps, nan_flag, C, H, W, ny, nx,
                     th, tw, n);
  HDIFF_CHECK_LAUNCH("tile_ddim_step_kernel");
  return HDIFF_OK;
}

int hdiff_tile_dpmpp_step(float* y, const float* eps_w, float* x0_prev, const int32_t* first_y, const int32_t* count_y,
                          const float* weight_y, const int32_t* origin_y, const int32_t* first_x, const int32_t* count_x,
                          const float* weight_x, const int32_t* origin_x, const float* tab, const int32_t* step_ptr, int nsteps,
                          int clip_x0, int32_t* nan_flag, int B, int C, int H, int W, int ny, int nx, int th, int tw,
                          hdiff_stream_t stream) {
  if (const int rc = check_tile_step("tile_dpmpp_step",
                                     y && eps_w && x0_prev && first_y && count_y && weight_y && origin_y && first_x && count_x &&
                                         weight_x && origin_x && tab && step_ptr && nan_flag,
                                     B, C, H, W, ny, nx, th, tw, nsteps))
    return rc;
  (void)hipGetLastError();
  const int64_t n = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(tile_dpmpp_step_kernel, dim3(grid_ceil_8k(n, 4)), dim3(256), 0, (hipStream_t)stream, y, eps_w, x0_prev, first_y,
                     count_y, weight_y, origin_y, first_x, count_x, weight_x, origin_x, tab, step_ptr, nsteps, clip_x0, nan_flag,
                     C, H, W, ny, nx, th, tw, n);
  HDIFF_CHECK_LAUNCH("tile_dpmpp_step_kernel");
  return HDIFF_OK;
}

}  // extern "C"
