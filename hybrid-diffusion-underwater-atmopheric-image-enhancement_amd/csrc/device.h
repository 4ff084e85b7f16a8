// Device-side helpers shared by the gfx950 kernels: everything here can change a kernel's instructions, and nothing else in a
// header can (common.h is host-side only; conv_x3.h holds the argument structs of the split-operand convolutions and the direct 1x1).  Every helper is
// __device__ __forceinline__ and leaves no symbol behind.  The per-file tile constants (KT, THREADS, KROW ...) are NOT here: they
// coincide in value, not in meaning.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Mutation switch of the parity suite's own sensitivity tests (tests/test_gpu_mutation.py): a library built with
// -DHDIFF_MUTANT=<mask> silently damages ONE low-order piece product per bit, at the 2^-16 / 2^-17 level of the product --
//   bit 0 (1)   the split-bf16 3x3 and 1x1 convolutions: the term w0 x2 dropped (the 3x3's fp16-pair form: the low five bits of
//               every activation's second piece masked)
//   bit 1 (2)   the d_head 32 attention forward (attention_x3p.hip): the low five bits of the second Q piece of the scores masked
//   bit 2 (4)   the d_head 16 attention forward (attention_h2.hip): the same in its score product
//   bit 3 (8)   the d_head 16 attention forward: the low five bits of every second piece of P masked (the P V product)
//   bit 4 (16)  the attention backward (attention_bwd_h2.hip): the cross product o0 v1 of dP = dO V^T dropped
//   bit 5 (32)  the attention backward: the product o1 p0 of dV^T = dO^T P dropped
//   bit 6 (64)  the attention backward: the low five bits of the second fp16 piece of dS masked (2^-17 of dS: dK^T and dQ^T)
// `make mutant` builds bits 0, 1, 2, 4, 5 into build/libhdiff_mutant.so, `make mutant2` bits 3 and 6 into build/libhdiff_mutant2.so (bits 2
// and 3 both end in the d_head 16 forward's output, bits 4 and 6 both in dK / dQ: one library could not tell which of them a red test
// has seen).  The float64 error-class tests must FAIL on them.
#ifndef HDIFF_MUTANT
#define HDIFF_MUTANT 0
#endif

namespace hdiff {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float swishf(float v) { return v / (1.0f + __expf(-v)); }

// Swish with the hardware reciprocal (1 ulp) instead of an IEEE division: the convolutions' prologues run once per staged element
// and, on gfx950, every VALU instruction is issue time taken from the fp32 MFMA stream.
__device__ __forceinline__ float swish_fast(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// XCD-aware tile order for grids of (blocks along the sequence, heads, batch).  Workgroups are handed to the 8 XCDs round
// robin by linear id, and each XCD has its own L2: with the plain order the 8 XCDs all stream the K/V (or Q/dO) of every
// head (measured on the forward: 4.5x the algorithmic HBM bytes).  This bijection gives each (head, sample) pair to ONE XCD
// -- pair p runs on XCD p % 8 -- so its operands are fetched into one L2 only.  Needs heads * batch % 8 == 0 (heads = 8 in
// this model); otherwise the identity.
struct TileId { int x, head, b; };
__device__ __forceinline__ TileId xcd_tile() {
  const unsigned gx = gridDim.x, pairs = gridDim.y * gridDim.z;
  if (pairs % 8u != 0u) return TileId{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
  const unsigned lin = blockIdx.x + gx * (blockIdx.y + gridDim.y * blockIdx.z);
  const unsigned xcd = lin & 7u, idx = lin >> 3;
  const unsigned pair = (idx / gx) * 8u + xcd, x = idx % gx;
  return TileId{(int)x, (int)(pair % gridDim.y), (int)(pair / gridDim.y)};
}

// ---- matrix instructions on packed 16-bit operands held as 32-bit words: 16x16x32 into f32x4, 32x32x16 into f32x16
__device__ __forceinline__ f32x4 mfma_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_f16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- bf16 triples
// (a, b) -> three packed bf16 pairs with a = a0 + a1 + a2 exactly (b likewise): each piece is the top 16 bits of what is
// left (8 significand bits, truncated), the remainders are exact fp32 subtractions.  Only plain VALU instructions
// (v_and, v_sub, v_perm): v_dot2c_f32_bf16 and the packed-fp32 instructions would be fewer, but tools/mfma_bf16_coexec.hip
// shows that those stall against the bf16 MFMA stream instead of running beside it.
__device__ __forceinline__ unsigned pack_hi16(float lo, float hi) {
  return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, hi), __builtin_bit_cast(unsigned, lo), 0x07060302u);
}
__device__ __forceinline__ float top16(float x) {
  return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & 0xffff0000u);
}
__device__ __forceinline__ void split3(float a, float b, unsigned& h0, unsigned& h1, unsigned& h2) {
  h0 = pack_hi16(a, b);
  const float ra = a - top16(a), rb = b - top16(b);
  h1 = pack_hi16(ra, rb);
  const float sa = ra - top16(ra), sb = rb - top16(rb);
  h2 = pack_hi16(sa, sb);
}

// ---- fp16 pairs
// (a, b) -> two packed fp16 pairs with a = h0.lo + h1.lo up to 2^-23 |a| (or 2^-25 absolute), b likewise in the high halves.
// `one` is 1.0f in a register the compiler cannot see through: fma(a, 1, -h) must stay an fma (v_fma_mixlo / mixhi_f16: the
// residual is exact in fp32 and rounded once), a - h would be a conversion and a subtraction.
__device__ __forceinline__ void split2(float a, float b, float one, unsigned& h0, unsigned& h1) {
  const f16x2 p = {(_Float16)a, (_Float16)b};                 // v_cvt_pk_f16_f32: round to nearest even
  unsigned u = __builtin_bit_cast(unsigned, p);
  asm("" : "+v"(u));                                          // the halves are read back out of the packed register
  const f16x2 q = __builtin_bit_cast(f16x2, u);
  const f16x2 r = {(_Float16)__builtin_fmaf(a, one, -(float)q[0]), (_Float16)__builtin_fmaf(b, one, -(float)q[1])};
  h0 = u;
  h1 = __builtin_bit_cast(unsigned, r);
}

// The score operands of the fp16-pair attention kernels, forward and backward: k = k0 + k1, q = q0 + q1 (fp16 roundings of
// K 2^a, Q qscale 2^-a), the second pieces stored times 2^8 and their partners times 2^-8 (attention_h2.hip's header has the why).
constexpr int PAIR_SHIFT = 8;                 // second pieces are stored times 2^8
constexpr unsigned PAIR_DOWN2 = 0x1c001c00u;  // (2^-8, 2^-8) as packed fp16
// (xa, xb) -> the four-piece layout x0, x0 2^-8, x1 2^8, x1 as packed fp16 pairs; `up` = 2^8 in a register.  The fp32 values and the
// packed first pieces are made opaque: left alone the compiler rounds x0 twice -- once from the fp32 product for the stored piece,
// once from the EXACT product (v_fma_mixlo_f16) for the residual -- and where the two differ by an ulp the stored pieces no longer
// add up (found with an operand dump: 4e-4 instead of 5e-7)
__device__ __forceinline__ void pair4(float xa, float xb, float up, unsigned& x0, unsigned& x0s, unsigned& x1s, unsigned& x1) {
  asm("" : "+v"(xa), "+v"(xb));
  unsigned u0 = __builtin_bit_cast(unsigned, f16x2{(_Float16)xa, (_Float16)xb});
  asm("" : "+v"(u0));
  const f16x2 h = __builtin_bit_cast(f16x2, u0);
  const float ra = xa - (float)h[0], rb = xb - (float)h[1];            // exact
  const f16x2 dn = {(_Float16)(1.0f / (1 << PAIR_SHIFT)), (_Float16)(1.0f / (1 << PAIR_SHIFT))};
  x0 = u0;
  x0s = __builtin_bit_cast(unsigned, h * dn);
  x1s = __builtin_bit_cast(unsigned, f16x2{(_Float16)(ra * up), (_Float16)(rb * up)});
  x1 = __builtin_bit_cast(unsigned, f16x2{(_Float16)ra, (_Float16)rb});
}
// The score balance a of one (sample, head) from its maxima max |Q| and max |K| (bits of the fp32 values): k = K 2^a,
// q = Q qscale 2^-a put the two maxima in the same binade; clamped so that every power of two stays a normal float; zero / inf /
// NaN rows get no balance.  The backward recomputes the forward's scaling: both call this.
__device__ __forceinline__ int balance_exp(unsigned qmax_bits, unsigned kmax_bits, float qscale) {
  const float mq = __builtin_bit_cast(float, qmax_bits) * qscale;
  const int eq = (int)((__builtin_bit_cast(unsigned, mq) >> 23) & 0xffu), ek = (int)((kmax_bits >> 23) & 0xffu);
  int a = (eq == 0 || ek == 0 || eq == 255 || ek == 255) ? 0 : (eq - ek) / 2;
  return a < -60 ? -60 : (a > 60 ? 60 : a);
}

// Piece slots of one (sample, head) in the attention FORWARD's pre-split workspace, each L * D fp16 (the backward's own layout is
// in attention_bwd_h2.hip): rows of q (q0, q1 2^8); rows of k (k0, k0 2^-8, k1 2^8, k1); V' = V 2^s as [2][D][L] (v0, v1); the D
// factors 2^-s (fp32) in the last slot
enum { F_Q = 0, F_K = 2, F_V = 6, F_VINV = 8, F_COUNT = 9 };

// Fixed-reference softmax of the fp16 kernels: the reference point enters as P = 2^8 and moves when a lane's P values of one stage
// sum to 2^15 (attention_h2.hip, 'range'); a row sum at or above 2^90 (or NaN) can only come from NaN / inf inputs or, in the fp32 /
// bf16 kernels whose reference never moves, from an overflow: the query block goes to the check pass.
constexpr float OVERFLOW_LIMIT = 1.2379400e27f;   // 2^90
constexpr float P_SHIFT = 8.0f;
constexpr float P_TRIP = 32768.0f;

// ---- abs-max reductions
__device__ __forceinline__ float absmax4(float m, f32x4 v) {
  return fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
}
// max |x| of a row of L floats (L % 4 == 0) by a whole workgroup of 256 threads (tid = threadIdx.x), in two steps: row_absmax_waves
// leaves one maximum per wave in LDS and ends with the barrier, absmax_of_waves reduces them -- in every thread (row_absmax) or in
// the one thread that stores the result (qkv_rowmax).  Who calls whom here is pinned by tools/isa_diff.py: with the shuffle ladder
// in a helper of its own, or row_absmax written out in v_split_h2_kernel, the compiler moves one instruction of the callers.
__device__ __forceinline__ const float* row_absmax_waves(const float* src, int L, int tid) {
  __shared__ float red[4];
  float amax = 0.f;
  for (int i = tid; i < L / 4; i += 256) amax = absmax4(amax, *reinterpret_cast<const f32x4*>(src + 4 * (size_t)i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  return red;
}
__device__ __forceinline__ float absmax_of_waves(const float* red) { return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])); }
__device__ __forceinline__ float row_absmax(const float* src, int L, int tid) { return absmax_of_waves(row_absmax_waves(src, L, tid)); }
// ... of every channel row of qkv [B][3C][L] into rowmax[B][ROWS][C]: grid (ROWS * C, B), the first ROWS of q, k, v
template <int ROWS>
__device__ __forceinline__ void qkv_rowmax(const float* __restrict__ qkv, float* __restrict__ rowmax, int C, int L) {
  const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* red = row_absmax_waves(qkv + ((size_t)b * 3 * C + row) * L, L, tid);
  if (tid == 0) rowmax[(size_t)b * ROWS * C + row] = absmax_of_waves(red);
}

// ---- LDS-DMA
typedef __attribute__((address_space(3))) unsigned char lds_byte;
// One 1 KiB run global -> LDS without staging registers: lane i's 16 bytes at src + voff land at lds_dst + 16 i (global_load_lds_dwordx4).
// M0 is written in the statement that uses it and restored.  The compiler does not count this load: the kernel waits with its own
// s_waitcnt vmcnt(0) in front of the barrier that publishes the tile.
__device__ __forceinline__ void dma_1k(const unsigned char* src, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(src), "s"(lds_dst)
               : "memory");
}

}  // namespace hdiff
