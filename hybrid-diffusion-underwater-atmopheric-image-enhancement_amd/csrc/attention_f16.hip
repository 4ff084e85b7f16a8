// Flash attention forward of the opt-in "f16" contraction mode (HDIFF_CONTRACT_F16): the attention forward of INFERENCE with every
// operand carried as ONE fp16 piece and fp32 accumulation.  Same data layout as attention.hip (reference: nn.MultiheadAttention
// core, ModelCondition.py:189, 204-208); dispatched in front of the fp16-pair kernels (attention_h2.hip / attention_x3p.hip) only
// for calls with lse2 == NULL, d_head 16 / 32, L >= 512, L % 256 == 0 and the workspace of hdiff_mha_flash_fwd_workspace.
//
// FORMAT (tests/_f16_attention_emul.py emulates this text, not the code):
//   q = fp16(Q qscale 2^-a), k = fp16(K 2^a): qscale = log2(e) / sqrt(d); the balance a per (sample, head) from the maxima of the
//       head's Q and K channel rows exactly as qk_split_h2_kernel (balance_exp, device.h): a = (eq - ek) / 2 (C division) of the biased
//       exponents of max |Q| qscale and max |K|, clamped to +-60, 0 when either is zero / inf / NaN.
//   v = fp16(V 2^s), s per channel row with max |V 2^s| in [2^14, 2^15), as v_split_h2_kernel (exponent clamped to [-100, 127]).
//   S = k . q on the fp16 MFMA into an fp32 accumulator that starts from -m;  P = fp16(exp2(S)) by v_cvt_pk_f16_f32 alone;
//   O += v . P in an fp32 accumulator;  l = the row sum of the fp32 P BEFORE rounding (as the pair kernels);  out = (O / l) 2^-s.
//   reference : fp16 ends at 65 504, so the softmax reference MOVES as in attention_h2.hip: it enters as P = 2^8 for the maximum of
//       the query's first 64 keys, and whenever a lane's P values of one stage sum to 2^15 or more the wave makes that stage again
//       from its S accumulators under a reference that puts the row's maximum over the stage at 2^8, after scaling O and l of that
//       query by the exact power of two.  One reference per query.  Rows that do not need it get delta = 0 and the same bits.
//   NaN / inf inputs end in l = NaN (or >= 2^90): the query's output is NaN and the caller's check pass (the overflow-proof fp32
//       kernel) takes the query block, like every kernel of the family.
//   Error class: P and v carry 11 significant bits -- 2^-12 relative per product, random in sign; measured against float64 about
//       2e-4 .. 5e-4 rms of a channel's largest output (3e-3 for near-uniform rows).  No low-order term exists, so there is no
//       mutant bit for this file.
//
// WORKSPACE (inside the first third of the pair kernels' workspace, whose size does not change): per (sample, head) three pieces of
//   L * D fp16: 0: q [L][D], 1: k [L][D], 2: v [D][L]; behind the B * heads triples the 3 C row maxima per sample (fp32, [B][3C]).
//   One maximum pass (3 C rows) and ONE split pass that writes only these three pieces.
//
// KERNELS, 256 queries per workgroup, four waves, two workgroups per CU (two waves per SIMD), plain control flow:
//   d_head 16 : scores S^T = K Q^T on v_mfma_f32_16x16x16_f16 (16 keys x 16 queries, all 16 contraction slots are d), P V on
//       v_mfma_f32_16x16x32_f16 (the accumulator layout of two 16-key score tiles IS the B operand up to a permutation of the
//       slots, which the V reads follow).  Per stage (16 queries x 64 keys) 4 + 2 = 6 MFMAs against 14 of the pair kernel; 40
//       vector instructions per lane against 56 (16 exp, 8 cvt_pk, 16 adds).  K = 16 or K = 32 with zeros in half the slots for the
//       scores: both take the same 16 cycles (tools/mfma_k16_probe.hip), the K = 16 form draws about 80 % of the energy and its A / B
//       operands are 2 registers instead of 4 (no zero registers to keep, half the LDS bytes read per operand) -- on a kernel that
//       sits on the board's power limit the joules decide, so the K = 16 form is the one built; the zero-fed K = 32 form would cost
//       4 x 0.2 of an MFMA's energy more per stage (about 13 % of the stage's matrix energy) and 8 registers.
//       Key tiles of 128 keys: K is one 4 KiB run ([key][32 bytes], unpadded) copied by LDS-DMA, 1 KiB per wave; V (16 padded rows)
//       goes through registers, one 16-byte chunk per thread.  Double buffered.
//   d_head 32 : attention_x3p.hip with one piece: 32 keys x 32 queries on v_mfma_f32_32x32x16_f16, 2 + 2 MFMAs per block against
//       6 + 6; K (padded rows, conflict-free ds_read_b128) and V staged through registers as there.
#include <stdlib.h>

#include "common.h"
#include "device.h"

using namespace hdiff;

namespace {

constexpr int THREADS = 256;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16k16(u32x2 a, u32x2 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned pack_f16(float a, float b) {      // v_cvt_pk_f16_f32: round to nearest even
  return __builtin_bit_cast(unsigned, f16x2{(_Float16)a, (_Float16)b});
}
// 2^-s of a V channel row from its maximum: the inverse of the scale the split pass applied (both are normal numbers)
__device__ __forceinline__ int v_exponent(float amax) {
  int e = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu) - 127;
  return e < -100 ? -100 : (e > 127 ? 127 : e);
}

// ---------------------------------------------------------------------------------------------------------------------
// Pass 1: max |x| of every Q / K / V channel row into rowmax[B][3C] (grid (3C, B)).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void f16_rowmax_kernel(const float* __restrict__ qkv, float* __restrict__ rowmax, int C, int L) {
  qkv_rowmax<3>(qkv, rowmax, C, L);
}

// ---------------------------------------------------------------------------------------------------------------------
// Pass 2: the three fp16 pieces (grid (L / 256, 3 heads, B); thread = one position, all D channels of one of q / k / v).
// An infinite or NaN input stays one in fp16.
// ---------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(THREADS) void f16_split_kernel(const float* __restrict__ qkv, const float* __restrict__ rowmax,
                                                            _Float16* __restrict__ ws, int C, int L, float qscale) {
  const int heads = C / D;
  const int which = blockIdx.y / heads, head = blockIdx.y - which * heads, b = blockIdx.z;
  const int l = blockIdx.x * THREADS + threadIdx.x;
  if (l >= L) return;
  const float* rm = rowmax + (size_t)b * 3 * C;
  const float* src = qkv + ((size_t)b * 3 * C + (size_t)which * C + (size_t)head * D) * L;
  const size_t piece = (size_t)L * D;
  _Float16* dst = ws + (((size_t)b * heads + head) * 3 + which) * piece;
  if (which < 2) {
    // the head's balance: exponents of max |q| qscale and max |k| (2 D row maxima per thread: L2-resident)
    float mq = 0.f, mk = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      mq = fmaxf(mq, rm[head * D + d]);
      mk = fmaxf(mk, rm[C + head * D + d]);
    }
    const int a = balance_exp(__builtin_bit_cast(unsigned, mq), __builtin_bit_cast(unsigned, mk), qscale);      // k 2^a, q 2^-a
    const float sc = which == 0 ? qscale * __builtin_bit_cast(float, (unsigned)(127 - a) << 23) : __builtin_bit_cast(float, (unsigned)(127 + a) << 23);
    unsigned h[D / 2];
#pragma unroll
    for (int j = 0; j < D / 2; ++j) h[j] = pack_f16(src[(size_t)(2 * j) * L + l] * sc, src[(size_t)(2 * j + 1) * L + l] * sc);
    u32x4* o = reinterpret_cast<u32x4*>(dst + (size_t)l * D);
#pragma unroll
    for (int j = 0; j < D / 8; ++j) o[j] = u32x4{h[4 * j], h[4 * j + 1], h[4 * j + 2], h[4 * j + 3]};
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float scale = __builtin_bit_cast(float, (unsigned)(14 - v_exponent(rm[2 * C + head * D + d]) + 127) << 23);
      dst[(size_t)d * L + l] = (_Float16)(src[(size_t)d * L + l] * scale);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------------------
// d_head 16.  Wave = 4 query tiles of 16; key tile = 128 keys = two stages of 64 keys (four 16-key score tiles each).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS, 2) void mha_flash_fwd_f16_d16_kernel(const _Float16* __restrict__ ws, const float* __restrict__ rowmax,
                                                                          float* __restrict__ out, int C, int L) {
  constexpr int D = 16, NQ = 4, KT = 128;
  constexpr int KROWB = D * 2;             // bytes per key (unpadded: the DMA writes runs; a 16-key operand read is 512 contiguous bytes)
  constexpr int KPART = KT * KROWB;        // 4 KiB
  constexpr int VROWB = KT * 2 + 16;       // bytes per d row (+16: 68 words = 4 mod 64, a half-wave's 8-byte reads cover the 64 banks once)
  constexpr int VPART = D * VROWB;
  constexpr int BUFB = KPART + VPART;
  static_assert(D * (KT * 2 / 16) == THREADS, "staging geometry: one 16-byte V chunk per thread");
  static_assert(KPART == 4 * 1024 && THREADS == 256, "LDS-DMA geometry: four 1 KiB runs, one per wave");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][BUFB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const TileId tile = xcd_tile();
  const int head = tile.head, b = tile.b;
  const int heads = gridDim.y;
  const int qblk0 = tile.x * 256 + wave * (16 * NQ);
  const int ntiles = L / KT;
  const size_t piece = (size_t)L * D;
  const _Float16* wsq = ws + ((size_t)b * heads + head) * 3 * piece;

  // Q operands (B of S^T = K Q^T): lane (query i16, group g) holds d = 4 g .. 4 g + 3
  u32x2 qop[NQ];
#pragma unroll
  for (int qt = 0; qt < NQ; ++qt) qop[qt] = *reinterpret_cast<const u32x2*>(wsq + (size_t)(qblk0 + qt * 16 + i16) * D + 4 * g);
  const int kaddr = i16 * KROWB + 8 * g;              // + 16-key tile * 16 * KROWB
  const int vaddr = KPART + i16 * VROWB + 8 * g;      // + 32-key chunk * 64 (+ 32 for the second 16 keys of the chunk)

  // staging: K by LDS-DMA (wave w copies run w of the tile), V chunk tid through a register
  const unsigned char* vsrc;
  int vlds;
  {
    const int d = tid >> 4, seg = tid & 15;
    vsrc = reinterpret_cast<const unsigned char*>(wsq + 2 * piece + (size_t)d * L) + seg * 16;
    vlds = KPART + d * VROWB + seg * 16;
  }
  const unsigned lds0 = (unsigned)(size_t)(lds_byte*)&smem[0][0];
  const unsigned char* kdma = reinterpret_cast<const unsigned char*>(wsq + piece);
  auto dma_k = [&](int t, int buf) {
    const int ws_ = __builtin_amdgcn_readfirstlane(wave);      // the asm operands must be scalar registers
    const unsigned char* src = kdma + (size_t)t * KPART + (size_t)ws_ * 1024;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + buf * BUFB + ws_ * 1024);
    dma_1k(src, lane * 16, dst);
  };
  u32x4 stage;
  auto stage_load = [&](int t) { stage = *reinterpret_cast<const u32x4*>(vsrc + (size_t)t * (KT * 2)); };
  auto stage_store = [&](int buf) { *reinterpret_cast<u32x4*>(&smem[buf][vlds]) = stage; };

  f32x4 O[NQ];
  float negm[NQ], l_run[NQ];
#pragma unroll
  for (int qt = 0; qt < NQ; ++qt) {
    O[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    negm[qt] = 0.f;
    l_run[qt] = 0.f;
  }

  auto load_k = [&](int buf, int st, u32x2 (&kop)[4]) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) kop[kt] = *reinterpret_cast<const u32x2*>(smem[buf] + kaddr + (4 * st + kt) * 16 * KROWB);
  };
  // V operands of the two 32-key chunks of a stage: contraction slot 8 g + 4 j + r  <->  key 32 c + 16 j + 4 g + r
  auto load_v = [&](int buf, int st, u32x4 (&vop)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const unsigned char* src = smem[buf] + vaddr + (2 * st + c) * 64;
      const u32x2 lo = *reinterpret_cast<const u32x2*>(src);
      const u32x2 hi = *reinterpret_cast<const u32x2*>(src + 32);
      vop[c] = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
  };
  auto scores = [&](const u32x2 (&kop)[4], int qt, float nm, f32x4 (&S)[4]) {
    asm volatile("" : "+v"(nm));             // a fresh splat per chain
    const f32x4 c = f32x4{nm, nm, nm, nm};   // the chain starts from -m: the accumulator holds s - m
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) S[kt] = mfma16k16(kop[kt], qop[qt], c);
  };
  // P = fp16(exp2(S)) of one stage packed as the B operands of P V, and the lane's sum of the fp32 P
  auto exp_pack = [&](const f32x4 (&S)[4], u32x4 (&pp)[2], float& sum0, float& sum1) {
    sum0 = 0.f; sum1 = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const float p0 = __builtin_amdgcn_exp2f(S[kt][0]), p1 = __builtin_amdgcn_exp2f(S[kt][1]);
      const float p2 = __builtin_amdgcn_exp2f(S[kt][2]), p3 = __builtin_amdgcn_exp2f(S[kt][3]);
      sum0 += p0 + p2;
      sum1 += p1 + p3;
      const int c = kt >> 1, o = (kt & 1) * 2;
      pp[c][o] = pack_f16(p0, p1);
      pp[c][o + 1] = pack_f16(p2, p3);
    }
  };
  auto stage_max = [&](const f32x4 (&S)[4]) {
    float mx = fmaxf(fmaxf(S[0][0], S[0][1]), fmaxf(S[0][2], S[0][3]));
#pragma unroll
    for (int kt = 1; kt < 4; ++kt) mx = fmaxf(mx, fmaxf(fmaxf(S[kt][0], S[kt][1]), fmaxf(S[kt][2], S[kt][3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    return fmaxf(mx, __shfl_xor(mx, 32, 64));      // over the four lanes that share the query
  };
  auto softmax = [&](f32x4 (&S)[4], int qt, u32x4 (&pp)[2]) {
    float sum0, sum1;
    exp_pack(S, pp, sum0, sum1);
    // any lane whose 16 values sum to 2^15 or more: some P of this stage may not fit fp16 (they are >= 0)
    if (__builtin_amdgcn_ballot_w64(sum0 + sum1 >= P_TRIP) != 0ull) {
      const float mx = stage_max(S);
      const float delta = (mx > P_SHIFT + 1.0f) ? __builtin_ceilf(mx - P_SHIFT) : 0.f;
      const int e = -(int)delta;
#pragma unroll
      for (int r = 0; r < 4; ++r) O[qt][r] = __builtin_ldexpf(O[qt][r], e);
      l_run[qt] = __builtin_ldexpf(l_run[qt], e);
      negm[qt] -= delta;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) S[kt] -= f32x4{delta, delta, delta, delta};
      exp_pack(S, pp, sum0, sum1);
    }
    l_run[qt] += sum0 + sum1;
  };
  // one stage: 64 keys against the wave's four query tiles; two query tiles' score chains are issued before the first one's exp
  // stream so that a wave's own matrix work runs beside its vector work (attention_x3p.hip)
  auto stage_fn = [&](int buf, int st) {
    u32x2 kop[4];
    u32x4 vop[2];
    load_k(buf, st, kop);
    load_v(buf, st, vop);
    f32x4 S[2][4];
    scores(kop, 0, negm[0], S[0]);
#pragma unroll
    for (int qt = 0; qt < NQ; ++qt) {
      if (qt + 1 < NQ) scores(kop, qt + 1, negm[qt + 1], S[(qt + 1) & 1]);
      u32x4 pp[2];
      softmax(S[qt & 1], qt, pp);
#pragma unroll
      for (int c = 0; c < 2; ++c) O[qt] = mfma_f16(vop[c], pp[c], O[qt]);
    }
  };

  stage_load(0);
  dma_k(0, 0);
  stage_store(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  stage_load(ntiles > 1 ? 1 : 0);
  dma_k(ntiles > 1 ? 1 : 0, 1);
  {
    // the reference points: per query, the maximum over its own first 64 keys (scores with C = 0) enters as P = 2^8
    u32x2 k0[4];
    load_k(0, 0, k0);
#pragma unroll
    for (int qt = 0; qt < NQ; ++qt) {
      f32x4 S[4];
      scores(k0, qt, 0.f, S);
      negm[qt] = P_SHIFT - stage_max(S);
    }
  }
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    stage_fn(buf, 0);
    stage_fn(buf, 1);
    stage_store(buf ^ 1);                                  // V of tile t + 1: that buffer was last read before the previous barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's K run of tile t + 1 has landed in buffer buf ^ 1
    __syncthreads();
    const int tn = (t + 2 < ntiles) ? t + 2 : ntiles - 1;
    stage_load(tn);
    dma_k(tn, buf);                                        // buffer buf is free: every wave has passed the barrier
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // no LDS-DMA in flight when the workgroup's LDS is released

  float* obase = out + ((size_t)b * C + (size_t)head * D) * L;
  const float* vmax = rowmax + (size_t)b * 3 * C + 2 * C + head * D;
#pragma unroll
  for (int qt = 0; qt < NQ; ++qt) {
    float lt = l_run[qt];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const bool bad = !(lt < OVERFLOW_LIMIT);            // NaN / inf inputs: hand this query block to the fp32 kernel's check pass
    const float inv = bad ? __builtin_nanf("") : 1.0f / lt;
    const int q = qblk0 + qt * 16 + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 4 * g + r;
      const float vinv = __builtin_bit_cast(float, (unsigned)(v_exponent(vmax[d]) - 14 + 127) << 23);
      obase[(size_t)d * L + q] = (O[qt][r] * inv) * vinv;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// d_head 32.  Wave = 2 query groups of 32; key tile = 64 keys = two blocks of 32 keys.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS, 2) void mha_flash_fwd_f16_d32_kernel(const _Float16* __restrict__ ws, const float* __restrict__ rowmax,
                                                                          float* __restrict__ out, int C, int L) {
  constexpr int D = 32, KT = 64;
  constexpr int KS = D / 16;                   // k-steps of the QK^T product
  constexpr int KROWB = D * 2 + 16;            // bytes per key in LDS (+16: conflict-free ds_read_b128)
  constexpr int KPART = KT * KROWB;
  constexpr int VROWB = KT * 2 + 8;            // bytes per d row (+8: rows spread over the banks)
  constexpr int VPART = D * VROWB;
  constexpr int NKC = KT * D / 8;              // 16-byte chunks of a K tile
  constexpr int NVC = D * 8;                   // 16-byte chunks of a V tile
  static_assert(NKC == THREADS && NVC == THREADS, "staging geometry: one K and one V chunk per thread");
  constexpr int BUFB = (KPART + VPART + 15) / 16 * 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][BUFB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const TileId tile = xcd_tile();
  const int head = tile.head, b = tile.b;
  const int heads = gridDim.y;
  const int qblk0 = tile.x * 256 + wave * 64;
  const size_t piece = (size_t)L * D;
  const _Float16* wsq = ws + ((size_t)b * heads + head) * 3 * piece;
  const int ntiles = L / KT;

  // Q operands (B of S^T = K Q^T): lane (query l31, half h) holds d = 16 s + 8 h .. + 7
  u32x4 qop[2][KS];
#pragma unroll
  for (int G = 0; G < 2; ++G)
#pragma unroll
    for (int s = 0; s < KS; ++s) qop[G][s] = *reinterpret_cast<const u32x4*>(wsq + (size_t)(qblk0 + 32 * G + l31) * D + 16 * s + 8 * h);

  // staging: thread tid carries chunk tid of the K tile and chunk tid of the V tile
  const unsigned char* ksrc = reinterpret_cast<const unsigned char*>(wsq + piece) + (size_t)tid * 16;
  const int klds = (tid >> 2) * KROWB + (tid & 3) * 16;
  const unsigned char* vsrc = reinterpret_cast<const unsigned char*>(wsq + 2 * piece + (size_t)(tid >> 3) * L) + (tid & 7) * 16;
  const int vlds = KPART + (tid >> 3) * VROWB + (tid & 7) * 16;
  u32x4 stage_k, stage_v;
  auto stage_load = [&](int t) {
    stage_k = *reinterpret_cast<const u32x4*>(ksrc + (size_t)t * (KT * D * 2));
    stage_v = *reinterpret_cast<const u32x4*>(vsrc + (size_t)t * (KT * 2));
  };
  auto stage_store = [&](int buf) {
    *reinterpret_cast<u32x4*>(&smem[buf][klds]) = stage_k;
    unsigned char* dst = &smem[buf][vlds];               // V rows are 8-byte aligned: two 8-byte stores
    *reinterpret_cast<u32x2*>(dst) = u32x2{stage_v[0], stage_v[1]};
    *reinterpret_cast<u32x2*>(dst + 8) = u32x2{stage_v[2], stage_v[3]};
  };

  const int kaddr = l31 * KROWB + 16 * h;                  // + key block * 32 * KROWB + k-step * 32
  const int vaddr = KPART + l31 * VROWB + 8 * h;

  f32x16 O[2];
  float l_run[2] = {0.f, 0.f};
  float negm2[2] = {0.f, 0.f};          // -m of the lane's two queries
#pragma unroll
  for (int G = 0; G < 2; ++G)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[G][r] = 0.f;

  auto load_k = [&](int buf, int kb, u32x4 (&kop)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) kop[s] = *reinterpret_cast<const u32x4*>(smem[buf] + kb * 32 * KROWB + kaddr + 32 * s);
  };
  // V operands of the two 16-key halves of a 32-key block: contraction slot 8 h + 4 jj + i  <->  key 16 ab + 8 jj + 4 h + i
  auto load_v = [&](int buf, int kb, u32x4 (&vop)[2]) {
#pragma unroll
    for (int ab = 0; ab < 2; ++ab) {
      const unsigned char* src = smem[buf] + vaddr + kb * 64 + 32 * ab;
      const u32x2 lo = *reinterpret_cast<const u32x2*>(src);
      const u32x2 hi2 = *reinterpret_cast<const u32x2*>(src + 16);
      vop[ab] = u32x4{lo[0], lo[1], hi2[0], hi2[1]};
    }
  };
  auto qk = [&](const u32x4 (&kop)[KS], int G, float nm) {
    asm volatile("" : "+v"(nm));               // a fresh splat per chain: one tuple of registers, not one per query
    f32x16 S;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = nm;    // the chain starts from -m: the accumulator holds s - m
#pragma unroll
    for (int s = 0; s < KS; ++s) S = mfma_f16(kop[s], qop[G][s], S);
    return S;
  };
  auto exp_pack = [&](const f32x16& S, u32x4 (&pop)[2], float& sum0, float& sum1) {
    sum0 = 0.f; sum1 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p0 = __builtin_amdgcn_exp2f(S[4 * j]), p1 = __builtin_amdgcn_exp2f(S[4 * j + 1]);
      const float p2 = __builtin_amdgcn_exp2f(S[4 * j + 2]), p3 = __builtin_amdgcn_exp2f(S[4 * j + 3]);
      sum0 += p0 + p2;
      sum1 += p1 + p3;
      const int ab = j >> 1, o = (j & 1) * 2;
      pop[ab][o] = pack_f16(p0, p1);
      pop[ab][o + 1] = pack_f16(p2, p3);
    }
  };
  auto block_max = [&](const f32x16& S) {
    float mx = fmaxf(fmaxf(S[0], S[1]), fmaxf(S[2], S[3]));
#pragma unroll
    for (int j = 1; j < 4; ++j) mx = fmaxf(mx, fmaxf(fmaxf(S[4 * j], S[4 * j + 1]), fmaxf(S[4 * j + 2], S[4 * j + 3])));
    return fmaxf(mx, __shfl_xor(mx, 32, 64));                       // the two lanes that share the query
  };
  auto softmax = [&](f32x16& S, int G, u32x4 (&pop)[2]) {
    float sum0, sum1;
    exp_pack(S, pop, sum0, sum1);
    // any lane whose 16 values sum to 2^15 or more: some P of this block may not fit fp16 (they are >= 0)
    if (__builtin_amdgcn_ballot_w64(sum0 + sum1 >= P_TRIP) != 0ull) {
      const float mx = block_max(S);
      const float delta = (mx > P_SHIFT + 1.0f) ? __builtin_ceilf(mx - P_SHIFT) : 0.f;
      const int e = -(int)delta;
#pragma unroll
      for (int r = 0; r < 16; ++r) O[G][r] = __builtin_ldexpf(O[G][r], e);
      l_run[G] = __builtin_ldexpf(l_run[G], e);
      negm2[G] -= delta;
#pragma unroll
      for (int r = 0; r < 16; ++r) S[r] -= delta;
      exp_pack(S, pop, sum0, sum1);
    }
    l_run[G] += sum0 + sum1;
  };

  stage_load(0);
  stage_store(0);
  __syncthreads();
  stage_load(ntiles > 1 ? 1 : 0);
  {
    // the reference points: per query, the maximum over its own first block (scores with C = 0) enters as P = 2^8
    u32x4 K0[KS];
    load_k(0, 0, K0);
    negm2[0] = P_SHIFT - block_max(qk(K0, 0, 0.f));
    negm2[1] = P_SHIFT - block_max(qk(K0, 1, 0.f));
  }
  auto block = [&](int buf, int kb) {
    u32x4 kop[KS], vop[2];
    load_k(buf, kb, kop);
    load_v(buf, kb, vop);
    f32x16 S2[2];
#pragma unroll
    for (int G = 0; G < 2; ++G) S2[G] = qk(kop, G, negm2[G]);      // both groups' chains before the first group's exp stream
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      u32x4 pop[2];
      softmax(S2[G], G, pop);
#pragma unroll
      for (int ab = 0; ab < 2; ++ab) O[G] = mfma_f16(vop[ab], pop[ab], O[G]);
    }
  };
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    block(buf, 0);
    block(buf, 1);
    stage_store(buf ^ 1);             // tile t + 1: that buffer was last read before the previous barrier
    __syncthreads();
    stage_load((t + 2 < ntiles) ? t + 2 : ntiles - 1);
  }

  float* obase = out + ((size_t)b * C + (size_t)head * D) * L;
  const float* vmax = rowmax + (size_t)b * 3 * C + 2 * C + head * D;
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    float lt = l_run[G];
    lt += __shfl_xor(lt, 32, 64);
    const bool bad = !(lt < OVERFLOW_LIMIT);            // NaN / inf inputs: hand this query block to the fp32 kernel's check pass
    const float inv = bad ? __builtin_nanf("") : 1.0f / lt;
    const int q = qblk0 + 32 * G + l31;
    // accumulator register r holds row 8 (r / 4) + 4 h + (r % 4) of O^T for query l31
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = 8 * (r >> 2) + 4 * h + (r & 3);
      const float vinv = __builtin_bit_cast(float, (unsigned)(v_exponent(vmax[d]) - 14 + 127) << 23);
      obase[(size_t)d * L + q] = (O[G][r] * inv) * vinv;
    }
  }
}

}  // namespace

namespace hdiff {

// The inference forward of the f16 mode: it writes no log-sum-exp.  Precondition (HDIFF_MHA_FWD_ROUTE_F16_SINGLE): d_head 16 or 32
// and ws holds mha_fwd_x3p_workspace bytes, non-zero for this shape (the pair kernels' size: plans are pooled by it; a third is used).
void launch_mha_fwd_f16(const float* qkv, float* o, int B, int C, int heads, int L, float qscale, void* ws, hipStream_t stream) {
  const int D = C / heads;
  const int64_t pieces = (int64_t)B * 3 * C * L * 2;               // B * heads * 3 pieces of L * D fp16
  // the 3 C row maxima per sample sit right behind the pieces: pieces + 12 B C bytes is far below need = 3 * pieces + tail
  float* rowmax = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(ws) + pieces);
  _Float16* wsh = reinterpret_cast<_Float16*>(ws);
  hipLaunchKernelGGL(f16_rowmax_kernel, dim3(3 * C, B), dim3(THREADS), 0, stream, qkv, rowmax, C, L);
  const dim3 sgrid(L / 256, 3 * heads, B), grid(L / 256, heads, B);
  if (D == 16) {
    hipLaunchKernelGGL((f16_split_kernel<16>), sgrid, dim3(THREADS), 0, stream, qkv, rowmax, wsh, C, L, qscale);
    hipLaunchKernelGGL(mha_flash_fwd_f16_d16_kernel, grid, dim3(THREADS), 0, stream, wsh, rowmax, o, C, L);
  } else {
    hipLaunchKernelGGL((f16_split_kernel<32>), sgrid, dim3(THREADS), 0, stream, qkv, rowmax, wsh, C, L, qscale);
    hipLaunchKernelGGL(mha_flash_fwd_f16_d32_kernel, grid, dim3(THREADS), 0, stream, wsh, rowmax, o, C, L);
  }
}

}  // namespace hdiff
