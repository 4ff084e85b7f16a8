// A dense layer along a short token axis: Y[b, co, l] = bias[co] + sum_ci W[co, ci] X[b, ci, l] on channel-major fp32 tensors
// X (B, Cin, L), Y (B, Cout, L) with L of a few hundred -- the nn.Linear of a ViT as hdiff_amd/dino.py lays its activations out
// (patch embedding, qkv, proj, fc1, fc2 and, on the transposed pack, every input gradient).  The contraction is the split-bf16
// scheme of conv1x1_x3.hip: every fp32 operand as three bf16 pieces (x = x0 + x1 + x2 exactly), the six piece products with
// i + j <= 2 on v_mfma_f32_32x32x16_bf16, small ones first, fp32 accumulation.
//
// Why its own kernel: the 1x1 GEMM kernels want H * W a multiple of 128 / 256 and Cin a multiple of 16 (L = 325 and the patch
// embedding's Cin = 588 are neither), so those layers ran on the fp32-input implicit-GEMM kernel over a 13 x 25 plane with tiles
// 63 % full.  Here every size is free: L, Cin, Cout >= 1.
//
// A wave owns 64 output channels x 32 tokens (two 32x32 accumulators).  Activations do not go through LDS: lane (l31, h) loads
// the 8 channels 16 c + 8 h .. + 7 of token l0 + l31 with 4-byte loads (a row of 325 floats is only 4-byte aligned; the loads
// coalesce over the lanes along L), splits them in registers, and each split value feeds 12 MFMAs.  Weights arrive pre-split from
// hdiff_dense_pack: [ceil(Cin / 16)][3 pieces][CoutPad][8 words], zero-padded in K and in the channels; a lane's A operand is words
// 4 h .. 4 h + 3 of channel row co0 + 32 mt + l31.
// Edges: a token l >= L or a channel ci >= Cin is loaded from a clamped address (inside the image's own rows) and replaced by
// zero -- zero weights alone would not do, 0 * NaN is NaN; stores of l >= L and co >= Cout are masked.
// One launch, no atomics, no split-K, no workspace; chunks, terms and channel tiles accumulate in one fixed order, and a tile
// reads one image only: results are bitwise repeatable and an image's numbers do not depend on its batch.
#include "common.h"
#include "device.h"

using namespace hdiff;

namespace {

constexpr int kTileCo = 64, kTileL = 32;

// split-product terms kept (piece of W, piece of X): all i + j <= 2, small ones first
__device__ constexpr int TERM_W[6] = {2, 1, 0, 1, 0, 0};
__device__ constexpr int TERM_X[6] = {0, 1, 2, 0, 1, 0};

struct DenseK {
  const float* x;
  const unsigned* wp3;
  const float* bias;
  float* y;
  int Cin, Cout, CoutPad, L;
  unsigned ncob, tiles_per_image, tiles;      // channel blocks; token tiles per image and in all
};

// A workgroup is ONE wave.  The grids are small (dinov2_vits14's proj at batch 2: 6 channel blocks x 11 token tiles x 2 images = 132
// tiles on 256 CUs), so every tile should get a SIMD of its own; 2 and 4 waves per workgroup on consecutive token tiles of the same 64
// channels (the same weight operands, from the vector L1 after the first wave) measured within 1 % of this on the whole loss at
// batch 2 and 16, and requesting the operands 2, 3 or 4 chunks ahead instead of 1 changed no layer's time beyond its spread
// (profiles/dino.txt).
__global__ __launch_bounds__(64) void dense_tokens_kernel(const DenseK p) {
  constexpr int MT = 2, DEPTH = 1, RING = DEPTH + 1;
  const int lane = threadIdx.x;
  const int l31 = lane & 31, h = lane >> 5;
  // Workgroup -> (token tile, channel block): the channel blocks of one token tile read the same X rows.  Workgroups go to the 8
  // XCDs round robin by linear id; inside a group of 8 tiles the tile is the fast index, so the blocks of a tile get ids 8 apart --
  // the same XCD, consecutive in time (conv1x1_x3.hip has the same map).  The last group may hold fewer than 8 tiles: still a
  // bijection, only without the locality.
  const unsigned lin = blockIdx.x, per = 8u * p.ncob;
  const unsigned grp = lin / per, r = lin - grp * per;
  const unsigned left = p.tiles - grp * 8u, n = left < 8u ? left : 8u;
  const unsigned tile = grp * 8u + r % n, cob = r / n;
  const int b = (int)(tile / p.tiles_per_image);
  const int l0 = (int)(tile % p.tiles_per_image) * kTileL;
  const int co0 = (int)cob * kTileCo;

  const int l = l0 + l31;
  const bool l_ok = l < p.L;
  const unsigned lmask = l_ok ? 0xffffffffu : 0u;
  const float* xl = p.x + (size_t)b * p.Cin * p.L + (l_ok ? l : p.L - 1);
  const unsigned* wlane = p.wp3 + ((size_t)(co0 + l31) * 8 + h * 4);
  const size_t w_piece = (size_t)p.CoutPad * 8, w_chunk = 3 * w_piece;
  const int nchunks = (p.Cin + 15) / 16;

  f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

  float xr[RING][8];
  u32x4 wr[RING][MT][3];
  auto load_x = [&](float (&x)[8], int c) {
    c = min(c, nchunks - 1);                                       // uniform; the pipeline's overshoot re-reads the last chunk
    const int k0 = 16 * c + 8 * h;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = xl[(unsigned)min(k0 + j, p.Cin - 1) * (unsigned)p.L];      // (Cin * L < 2^31: the launcher's check)
  };
  auto load_w = [&](u32x4 (&w)[MT][3], int c) {
    const unsigned* wb = wlane + (size_t)min(c, nchunks - 1) * w_chunk;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) w[mt][pc] = *reinterpret_cast<const u32x4*>(wb + pc * w_piece + (size_t)mt * 32 * 8);
  };
  // The zeroing of what lies outside Cin x L happens here, where a chunk is used, and is an AND with a mask: a select on a loaded
  // value is compiled to a branch around the load, and a mask applied at the load makes a chunk's loads wait for each other
  // instead of flying together.
  auto mma = [&](const float (&x)[8], const u32x4 (&w)[MT][3], int c) {
    u32x4 xp[3];
    const int k0 = 16 * c + 8 * h;
    float xm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) xm[j] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x[j]) & (k0 + j < p.Cin ? lmask : 0u));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned h0, h1, h2;
      split3(xm[2 * j], xm[2 * j + 1], h0, h1, h2);
      xp[0][j] = h0; xp[1][j] = h1; xp[2][j] = h2;
    }
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma_bf16(w[mt][TERM_W[t]], xp[TERM_X[t]], acc[mt]);
  };

  // X and the weights are requested DEPTH chunks ahead of their use; the ring indices must be compile-time constants
#pragma unroll
  for (int i = 0; i < DEPTH; ++i) {
    load_x(xr[i], i);
    load_w(wr[i], i);
  }
  for (int c = 0; c < nchunks; c += RING) {
#pragma unroll
    for (int i = 0; i < RING; ++i) {
      if (c + i < nchunks) {                                       // uniform
        load_x(xr[(i + DEPTH) % RING], c + i + DEPTH);
        load_w(wr[(i + DEPTH) % RING], c + i + DEPTH);
        mma(xr[i], wr[i], c + i);
      }
    }
  }

  // ---- epilogue: + bias, 4-byte stores coalesced along L.  Accumulator register i of tile mt holds channel
  // co0 + 32 mt + (i & 3) + 8 (i >> 2) + 4 h at token l0 + l31
  // (the bias values are all requested before the first is used, from clamped addresses)
  float* yl = p.y + (size_t)b * p.Cout * p.L + l;
  float add[MT][16];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) add[mt][i] = 0.f;
  if (p.bias) {                                                    // uniform
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) add[mt][i] = p.bias[min(co0 + 32 * mt + (i & 3) + 8 * (i >> 2) + 4 * h, p.Cout - 1)];
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + 32 * mt + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (l_ok && co < p.Cout) yl[(size_t)co * p.L] = acc[mt][i] + add[mt][i];
    }
}

// One thread per (chunk, channel row, word): the two weights of the word, split, to the three piece planes.  The GEMM's rows are
// w's rows (M = Cout, K = Cin) or, transposed, w's columns (M = Cin, K = Cout).
__global__ __launch_bounds__(256) void dense_pack_kernel(const float* __restrict__ w, unsigned* __restrict__ wp3, int Cin, int M, int K,
                                                         int MPad, int transposed, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int word = (int)(i & 7);
    const int64_t row = i >> 3;
    const int m = (int)(row % MPad), c = (int)(row / MPad);
    const int k = 16 * c + 2 * word;
    float a = 0.f, b = 0.f;
    if (m < M) {
      if (k < K) a = transposed ? w[(size_t)k * Cin + m] : w[(size_t)m * Cin + k];
      if (k + 1 < K) b = transposed ? w[(size_t)(k + 1) * Cin + m] : w[(size_t)m * Cin + k + 1];
    }
    unsigned h0, h1, h2;
    split3(a, b, h0, h1, h2);
    unsigned* dst = wp3 + ((size_t)c * 3 * MPad + m) * 8 + word;
    dst[0] = h0;
    dst[(size_t)MPad * 8] = h1;
    dst[(size_t)MPad * 16] = h2;
  }
}

int check_dims(const char* who, int Cout, int Cin) {
  HDIFF_CHECK_ARG(Cout >= 1 && Cin >= 1, "%s: Cout = %d, Cin = %d; both must be at least 1", who, Cout, Cin);
  HDIFF_CHECK_ARG(Cout <= (1 << 24) && Cin <= (1 << 24), "%s: Cout = %d, Cin = %d; at most 2^24 each", who, Cout, Cin);
  return HDIFF_OK;
}

int64_t pad_co(int Cout) { return ((int64_t)Cout + kTileCo - 1) / kTileCo * kTileCo; }
int64_t pack_words(int Cout, int Cin) { return ((int64_t)Cin + 15) / 16 * 3 * pad_co(Cout) * 8; }

}  // namespace

extern "C" {

int hdiff_dense_pack_words(int Cout, int Cin, int64_t* words_out) {
  const int rc = check_dims("dense_pack_words", Cout, Cin);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(words_out, "dense_pack_words: null pointer");
  *words_out = pack_words(Cout, Cin);
  return HDIFF_OK;
}

int hdiff_dense_pack(const float* w, void* wp3, int Cout, int Cin, int transposed, hdiff_stream_t stream) {
  const int rc = check_dims("dense_pack", Cout, Cin);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(w && wp3, "dense_pack: null pointer");
  HDIFF_CHECK_ARG(((uintptr_t)wp3 & 15) == 0, "dense_pack: wp3 must be 16-byte aligned");
  const int M = transposed ? Cin : Cout, K = transposed ? Cout : Cin;
  const int MPad = (int)pad_co(M);
  const int64_t n = pack_words(M, K) / 3;
  (void)hipGetLastError();
  hipLaunchKernelGGL(dense_pack_kernel, dim3(grid_ceil_8k(n)), dim3(256), 0, (hipStream_t)stream, w, (unsigned*)wp3, Cin, M, K, MPad,
                     transposed != 0, n);
  HDIFF_CHECK_LAUNCH("dense_pack kernel");
  return HDIFF_OK;
}

int hdiff_dense_tokens(const float* x, const void* wp3, const float* bias, float* y, int B, int Cin, int Cout, int64_t L,
                       hdiff_stream_t stream) {
  const int rc = check_dims("dense_tokens", Cout, Cin);
  if (rc != HDIFF_OK) return rc;
  HDIFF_CHECK_ARG(B >= 1, "dense_tokens: B = %d; at least 1 image", B);
  HDIFF_CHECK_ARG(L >= 1, "dense_tokens: L = %lld; at least 1 token", (long long)L);
  HDIFF_CHECK_ARG((int64_t)Cin * L < (1ll << 31) && (int64_t)Cout * L < (1ll << 31),
                  "dense_tokens: Cin * L = %lld, Cout * L = %lld; an image's elements are indexed in 31 bits", (long long)Cin * L,
                  (long long)Cout * L);
  HDIFF_CHECK_ARG(x && wp3 && y, "dense_tokens: null pointer");
  HDIFF_CHECK_ARG(((uintptr_t)wp3 & 15) == 0, "dense_tokens: wp3 must be 16-byte aligned");
  DenseK k;
  k.x = x; k.wp3 = (const unsigned*)wp3; k.bias = bias; k.y = y;
  k.Cin = Cin; k.Cout = Cout; k.CoutPad = (int)pad_co(Cout); k.L = (int)L;
  k.ncob = (unsigned)(k.CoutPad / kTileCo);
  const int64_t tpi = (L + kTileL - 1) / kTileL, tiles = tpi * B, wgs = tiles * k.ncob;
  HDIFF_CHECK_ARG(wgs < (1ll << 31), "dense_tokens: %lld workgroups; the grid holds fewer than 2^31", (long long)wgs);
  k.tiles_per_image = (unsigned)tpi;
  k.tiles = (unsigned)tiles;
  (void)hipGetLastError();
  hipLaunchKernelGGL(dense_tokens_kernel, dim3((unsigned)wgs), dim3(64), 0, (hipStream_t)stream, k);
  HDIFF_CHECK_LAUNCH("dense_tokens kernel");
  return HDIFF_OK;
}

}  // extern "C"
