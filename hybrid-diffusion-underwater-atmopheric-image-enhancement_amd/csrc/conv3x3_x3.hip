// 3x3 / stride-1 convolution with fp32 operands carried as three bf16 pieces on the bf16 matrix core
// (v_mfma_f32_32x32x16_bf16, fp32 accumulation) -- the HDIFF_CONTRACT_BF16X3 counterpart of conv_igemm.hip's fast path
// (reference call sites: ModelCondition.py:172, 186, 88 / diffusion/Model.py:275, 288, 184).
//
// Arithmetic: x = x0 + x1 + x2 exactly (top-16-bit truncations of successive exact remainders, attention_x3.hip), and
// w * x = sum over the six piece pairs with i + j <= 2 (dropped terms <= 3 * 2^-24 relative): fp32-class, checked against
// float64 next to the fp32-MFMA kernel in tests/test_gpu_ops.py.  Why it pays more here than in attention: both operands
// are split ONCE per staged element (the weights even once per model, by hdiff_pack_conv_weight_x3) and then used by 9 taps
// x 64 channels, so the split is noise and the kernel gets the 6/16 matrix-time ratio.
//
// Structure per workgroup (64 output channels x 8x32 pixels, 4 waves x 64 pixels), per chunk of 16 input channels:
//   * the (8+2) x (32+2) activation patch: global -> registers (prefetched one chunk ahead) -> GroupNorm affine + Swish ->
//     three bf16 pieces -> LDS as [piece][pixel][16 channels]: a lane's B operand (8 consecutive channels of one pixel) is one
//     16-byte LDS read, and a tap is just a pixel offset;
//   * the weights are not staged: hdiff_pack_conv_weight_x3 lays them out as [chunk][tap][piece][channel][16 ci], so a lane's
//     A operand is one 16-byte global load (L1/L2 resident: every workgroup of the launch reads the same 55 KB per chunk);
//   * per tap 6 piece pairs x (2 x 2) tiles = 24 MFMAs (a wave: 4 output rows x 6, pairs: x 3).
//   * Loop order (in the kernel, "Tap-column order"): the taps form an NDY x NDX rectangle and are walked column by column.  The
//     fp16-pair form reads each of the 4 + NDY - 1 patch rows of a tap column ONCE and feeds every (tap row, output row) that
//     needs it (36 LDS reads per chunk of the 3x3 instead of 72), weights one tap column ahead; the bf16-triple and DROP forms
//     keep one read per (tap, output row) with the weights two taps ahead, in the same column order of taps, so that every
//     accumulator sums in the same order in both (a DROP launch with keep = 1 equals the plain launch bit for bit).
//
// PAIR (round 4): the same kernel with both operands as fp16 PAIRS instead of bf16 triples (v_mfma_f32_32x32x16_f16), for
// convolutions with the GroupNorm + Swish prologue.  fp16 carries 11 significand bits, a pair x' = h0 + h1 holds 22-23 of
// fp32's 24 (attention_h2.hip has the split: v_cvt_pk_f16_f32 + v_fma_mixlo / mixhi_f16, 1.5 instructions per value against
// 5.5), and THREE products (w1 x0, w0 x1, w0 x0; dropped: w1 x1 <= 2^-22) replace six.  What fp16 lacks is range, and here the
// range is known before a single activation is read: the staged value is swish(gamma xhat + beta) with |xhat| <= sqrt(n - 1)
// for a group of n elements, so |value| <= sqrt(n - 1) max |gamma| + max |beta| =: A (hdiff_gn_act_scale evaluates it from the
// GroupNorm weights alone).  Activations are staged times 2^s with A 2^s < 2^15, weights are packed times 2^t with
// max |w| 2^t in [2^14, 2^15) (hdiff_pack_conv_weight_h2); the accumulator leaves through one multiplication by 2^-(s + t).
// Error of an operand: 2^-23 relative, or 2^-25 absolute in the scaled domain for values below 2^-3 there -- i.e. below
// 2^-18 of A resp. max |w|: fp32-class against the sum it enters (tests/test_gpu_ops.py holds the kernel to the bf16-triple
// kernel's gate: error against float64 within 1.5x of the fp32-MFMA kernel's).  The chain has 3 roundings per 16 input
// channels and tap instead of 6, and measures a SMALLER error than the bf16 triples (tools/h2_sim_conv.py).  A caller whose
// gn_scale / gn_shift are not GroupNorm statistics of x can break the bound: the fp16 conversion then yields inf and the
// output NaN -- loud, never silently wrong.
//
// Range sources of the PAIR form: (1) the GroupNorm bound above (act_scale, evaluated at pack time); (2) absmax_in, one word per
// sample with the bits of max |x[b]|, for convolutions WITHOUT a prologue: the workgroup forms 2^s from word blockIdx.z so that
// absmax 2^s lies in [2^14, 2^15).  The word comes out of the epilogue of the kernel that produced x (absmax_out below: no pass
// over memory -- a separate maximum pass costs a fifth of what the pairs save, profiles/r04_rejected_candidates.txt), so
// UpSample's four transposed-conv phases (their input: a ResBlock's residual epilogue), its 3x3 (input: the four phases'
// epilogues, all into the same words) and DownSample's 5x5 / stride 2 (input: the attention out-projection) run on pairs too.
// A word below the true maximum overflows the fp16 conversion: NaN, loud again.  Per SAMPLE, never per launch: a sample's result
// must not depend on what else is in the batch.
// absmax_out (every instantiation): the epilogue takes the maximum of the bit patterns of |v| over what the wave stores,
// reduces it in the wave and combines it into the sample's word by ONE unsigned atomicMax per wave -- order-independent, so
// bitwise reproducible; NaN and inf compare above every finite value and end up in the word.
//
// Strided input (in_s = 2: the four parity planes of a 5x5 / stride-2 / pad-2 conv, out(y, x) = sum w(ky, kx) in(2y + ky - 2,
// 2x + kx - 2)): the taps with ky % 2 == oy, kx % 2 == ox read plane (oy, ox) at (y + dy, x + dx), dy, dx in {-1, 0, 1} -- a
// stride-1 conv of 9 / 6 / 6 / 4 taps over that plane.  Only the staging address changes: pixel (iy, ix) of the grid the kernel
// walks is input element (iy in_s + in_oy, ix in_s + in_ox), bounds taken there.  The dispatcher (conv_igemm.hip) issues the four
// launches inside one call; they accumulate through the residual epilogue (residual_first: the last one adds the bias behind
// the partial sums, so the result is rounded once at its own size).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "conv_x3.h"
#include "device.h"

using namespace hdiff;

namespace {

constexpr int THREADS = 256;
constexpr int PH = 10, PW = 34, PPIX = PH * PW;      // patch of an 8 x 32 tile
constexpr int NSLOT = (4 * PPIX + THREADS - 1) / THREADS;   // (channel quad, pixel) staging slots per thread: 6
constexpr int HALF_WORDS = PPIX * 4;                  // one half-plane: [pixel][4 words] = channel pairs 4h .. 4h+3 of every pixel
constexpr int PIECE_WORDS = 2 * HALF_WORDS;           // 32-bit words of one piece: [half h][pixel][4 channel pairs]
constexpr int PSTRIDE = PIECE_WORDS + 8;              // plane stride: each plane is followed by a dump area ...
constexpr int DUMP_WORD = PIECE_WORDS;                // ... where the unused staging slot of a thread stores (branch-free staging)


// split-product terms kept (piece of W, piece of X): all i + j <= 2, small ones first
__device__ constexpr int TERM_W[6] = {2, 1, 0, 1, 0, 0};
__device__ constexpr int TERM_X[6] = {0, 1, 2, 0, 1, 0};

// NDY x NDX: the tap rectangle of the launch (3x3 = the plain conv; 3x2 / 2x3 / 2x2 = transposed-conv phases and parity planes
// with fewer taps): tap (dyi, dxi) reads pixel (y + dy_min + dyi, x + dx_min + dxi) and its weights are tap tap_idx[dyi * NDX + dxi]
// of the pack.  OUTMAP: the output pixel of (vy, vx) is (vy * out_sy + out_oy, vx * out_sx + out_ox) of an OH x OW plane
// (transposed-conv phases) instead of (vy, vx).
// PAIR: fp16 pairs and three products instead of bf16 triples and six (header); every (rectangle, OUTMAP) the launcher can ask for.
// DROP: train-mode dropout behind the GroupNorm + Swish prologue (nn.Dropout between Swish and the conv, ModelCondition.py:185):
// the keep words of a slot's four channels (one word per channel) are requested while the slot before it is staged, one slot's
// share of MFMAs ahead (a padding slot fetches the word of its channel plane's first element and never looks at it), and the
// staged value is kept ? swish(..) * inv_keep : 0.  A compile-time variant: the instantiations without it carry none of this.
// OCC = 2 for every instantiation: two waves per SIMD are the register bound (256 VGPRs) that all of them are built to.
template <int NDY, int NDX, bool OUTMAP, bool PAIR, int OCC = 2, bool DROP = false>
__global__ __launch_bounds__(THREADS, OCC) void conv3x3_x3_kernel(const ConvX3K p) {
  constexpr int NT = NDY * NDX;
  constexpr int NP = PAIR ? 2 : 3;         // pieces per operand
  __shared__ __attribute__((aligned(16))) unsigned sXbuf[2][NP * PSTRIDE];     // double-buffered: chunk c + 1 is staged beside chunk c's MFMAs
  extern __shared__ __attribute__((aligned(16))) float sG[];     // [2][Cin]: GroupNorm scale | shift of this sample

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int b = blockIdx.z;
  // Workgroup -> (pixel tile, channel block).  The channel blocks of ONE pixel tile read the same activation patch; in grid
  // order they are a whole plane of tiles apart and each fetched it from HBM again (measured on the fp32 kernel: input bytes x
  // Cout / 64).  Workgroups go to the 8 XCDs round robin by linear id, so the channel blocks of a tile are given linear ids
  // 8 apart: same XCD, consecutive in time -- the later ones find the patch in that XCD's L2.
  int tile_id = blockIdx.x, cob = blockIdx.y;
  if ((gridDim.x & 7u) == 0u && gridDim.y > 1u) {
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, per = 8u * gridDim.y;
    const unsigned grp = lin / per, r = lin - grp * per;
    tile_id = (int)(grp * 8u + (r & 7u));
    cob = (int)(r >> 3);
  }
  const int co0 = cob * 64;
  const int tile_y = tile_id / p.tiles_x, tile_x = tile_id - tile_y * p.tiles_x;
  const int vy0 = tile_y * 8, vx0 = tile_x * 32;
  const bool has_gn = p.gn_scale != nullptr;
  const size_t HW = (size_t)p.H * p.W;
  const size_t IHW = (size_t)p.IH * p.IW;      // channel stride of the input (= HW but for a strided input)
  // 2^s of the staged activations and 2^-s: the GroupNorm bound (act_scale), or formed here from the sample's range word
  // (absmax_in, a producer's epilogue maximum): max |x| 2^s in [2^14, 2^15).  The exponent is clamped as in v_split_h2_kernel so
  // that 2^s and 2^-s are normal numbers: a zero or denormal word gives 2^114, a non-finite one 2^-113 (inf / NaN stay what they
  // are in fp16, and a word below the true maximum overflows the conversion: NaN out, never finite wrong values).
  float xs = 1.0f, xinv = 1.0f;
  if constexpr (PAIR) {
    if (p.absmax_in != nullptr) {
      int e = (int)((p.absmax_in[b] >> 23) & 0xffu) - 127;
      e = e < -100 ? -100 : (e > 127 ? 127 : e);
      xs = __builtin_bit_cast(float, (unsigned)(14 - e + 127) << 23);
      xinv = __builtin_bit_cast(float, (unsigned)(e - 14 + 127) << 23);
    } else {
      xs = p.act_scale[0];
      xinv = p.act_scale[1];
    }
  }
  const float one = p.one;

  // LDS layout of a piece: two half-planes [h][pixel][4 words]; word w of half h holds the bf16 pieces of input channels
  // 8h + 2w, 8h + 2w + 1.  A lane's B operand (8 channels of one pixel) is ONE 16-byte read and consecutive lanes read
  // consecutive 16-byte blocks: conflict-free.  (Round 2's [pixel][8 words] put lanes 8 words apart: the operand reads were
  // 2-way and the 4-byte staging stores 8-way bank-conflicted -- SQ_LDS_BANK_CONFLICT was 60 % of the LDS-active cycles.)
  // staging slots: slot e = (channel quad jq = e / 340: channels 4 jq .. 4 jq + 3, patch pixel e % 340); 8-byte stores
  // Per slot ONE register for the global side: the byte offset of (first channel of the quad, pixel) from the chunk's first
  // channel plane, 0 for zero padding / an unused slot, whose bit of s_ok is clear.  The four channel planes and the chunk are
  // wave-uniform and go into the loads' scalar base ((16 channels) * IHW * 4 bytes < 2^31: every launch's input plane is below
  // 2^25 pixels, conv_igemm.hip).  The quad itself is one comparison away (slot i holds quads (256 i) / 340 and the next one).
  unsigned s_voff[NSLOT];
  unsigned s_ok = 0u;
  auto slot_quad = [&](int i) {
    const int lo = (i * THREADS) / PPIX;
    const int jq = lo + (tid + i * THREADS >= (lo + 1) * PPIX ? 1 : 0);
    return jq < 4 ? jq : 3;
  };
  // the LDS side likewise: the word offset inside a piece, (jq >> 1) * HALF_WORDS + (e - 340 jq) * 4 + (jq & 1) * 2 for slot
  // e = t + 256 i, is 4 t plus one of two constants; the dump word for an unused slot (jq = 4).  t is the thread id behind an
  // empty asm of the chunk: six offsets computed where they are used cost three instructions each, kept across the loop six registers.
  auto slot_lds = [&](int i, int t) {
    const int lo = (i * THREADS) / PPIX;
    auto konst = [&](int jq) { return (jq >> 1) * HALF_WORDS + (i * THREADS - jq * PPIX) * 4 + (jq & 1) * 2; };
    const bool next = t + i * THREADS >= (lo + 1) * PPIX;
    if (lo + 1 >= 4) return next ? DUMP_WORD : 4 * t + konst(lo);
    return 4 * t + (next ? konst(lo + 1) : konst(lo));
  };
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int e = tid + i * THREADS;
    const int jq = e / PPIX, pos = e - jq * PPIX;
    const int py = pos / PW, px = pos - py * PW;
    const int iy = vy0 - 1 + py, ix = vx0 - 1 + px;
    const bool used = jq < 4;
    const int gy = iy * p.in_s + p.in_oy, gx = ix * p.in_s + p.in_ox;
    const bool ok = used && iy >= 0 && gy < p.IH && ix >= 0 && gx < p.IW;
    s_voff[i] = ok ? (unsigned)(4 * jq) * (unsigned)(4 * IHW) + (unsigned)(gy * p.IW + gx) * 4u : 0u;
    s_ok |= ok ? 1u << i : 0u;
  }
  if (has_gn) {
    for (int i = tid; i < 2 * p.Cin; i += THREADS)
      sG[i] = (i < p.Cin) ? p.gn_scale[b * p.Cin + i] : p.gn_shift[b * p.Cin + (i - p.Cin)];
  }

  // Wave tile: 32 output channels x 4 pixel rows (wm = channel half, wn = row half of the 64 x (8 x 32) workgroup tile).
  // With all four waves on the same 64 channels (round 2: waves split the pixels only) every wave loaded the SAME weight
  // operands: 24 KB per tap per workgroup through the CU's 64 B/clk vector L1 -- 62 B/clk with two workgroups per CU, and
  // the PMC showed the waves parked on those loads 36 % of their time (MFMA busy 0.47).  The 2 x 2 split halves the
  // weight traffic and doubles the LDS operand reads, of which there is bandwidth to spare.
  const int wm = wave & 1, wn = wave >> 1;
  f32x16 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

  // The raw patch, ONE register set: a slot's registers are free once it is staged, and its values of the chunk after next are
  // requested at the start of the next tap column (chunk loop below) -- most of a chunk ahead of their use, no second set, no copies.
  f32x4 xv[NSLOT];
  // DROP: the four keep words of the slot that is staged NEXT (x1 == NULL and B * Cin * H * W < 2^31: checked on the host),
  // requested while the slot before it is staged -- one slot's share of MFMAs ahead of their use, four registers in flight.  `tie` is a
  // value of the slot just staged: the (empty) asm makes the element index depend on it.  Without it the compiler keeps the
  // 24 per-(slot, channel) parts of the indices as loop invariants and requests a chunk's words all at once, and the kernel --
  // 20 registers to spare at two waves per SIMD -- spills (31 VGPRs in the fp16-pair form).
  unsigned kw[DROP ? 4 : 1];
  unsigned ksh = 0;         // their four bit positions, five bits each
  auto fetch_keep = [&](int i, int c0, unsigned tie) {
    if constexpr (DROP) {
      const unsigned hw = (unsigned)IHW;
      unsigned e = (unsigned)(b * p.Cin + c0) * hw + (s_voff[i] >> 2);
      asm("" : "+v"(e) : "v"(tie));
      ksh = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        kw[k] = p.keep_bits[e >> 5];
        ksh |= (e & 31u) << (5 * k);
        e += hw;
      }
    }
  };
  // a 16-channel chunk never straddles the concat seam (C0 % 16 == 0 is checked on the host); the loads are unconditional: the
  // address is always valid
  auto load_slot = [&](int i, int c0) {
    const float* xbase = (c0 < p.C0) ? p.x0 + ((size_t)b * p.C0 + c0) * IHW : p.x1 + ((size_t)b * p.C1 + (c0 - p.C0)) * IHW;
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[i][k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(xbase + k * IHW) + s_voff[i]);
  };
  auto issue_loads = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) load_slot(i, c0);
  };
  // Branch-free: a slot outside the image stages 0 by a select, a thread's unused last slot writes to a dump word behind the
  // piece planes -- with per-slot branches the GroupNorm table reads of a slot could not be issued before the previous slot
  // had finished, and every slot paid an LDS round trip of its own (11 per chunk and wave).
  auto stage_slot = [&](auto gn_tag, int i, int c0, unsigned* sX, int t) {
    constexpr bool GN = decltype(gn_tag)::value;
    const int lds = slot_lds(i, t);
    f32x4 v = xv[i];
    if (!GN) {                  // (zero padding: the load read a valid address, the value is dropped here)
      const bool inside = (s_ok >> i) & 1u;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = inside ? v[k] : 0.f;
    }
    if (GN) {
      const int ci = c0 + 4 * slot_quad(i);
      const f32x4 sc = *reinterpret_cast<const f32x4*>(&sG[ci]);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(&sG[p.Cin + ci]);
      const bool inside = (s_ok >> i) & 1u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (DROP) {
          const bool kept = (kw[k] >> ((ksh >> (5 * k)) & 31u)) & 1u;
          v[k] = (inside && kept) ? swish_fast(fmaf(v[k], sc[k], sh[k])) * p.inv_keep : 0.f;
        } else {
          v[k] = inside ? swish_fast(fmaf(v[k], sc[k], sh[k])) : 0.f;
        }
      }
      if constexpr (DROP) {                 // slots are staged in order 0 .. NSLOT - 1, chunk after chunk
        const unsigned tie = __builtin_bit_cast(unsigned, v[0]);
        if (i + 1 < NSLOT) fetch_keep(i + 1, c0, tie);
        else fetch_keep(0, c0 + 16 < p.Cin ? c0 + 16 : c0, tie);      // branch-free: the last chunk re-reads its own words, unused
      }
    }
    if constexpr (PAIR) {
      unsigned a0, a1, c0w, c1w;
      split2(v[0] * xs, v[1] * xs, one, a0, a1);
      split2(v[2] * xs, v[3] * xs, one, c0w, c1w);
      if (HDIFF_MUTANT & 1) { a1 &= 0xffe0ffe0u; c1w &= 0xffe0ffe0u; }      // (mutation test: 2^-16 of every activation dropped)
      *reinterpret_cast<u32x2*>(&sX[lds]) = u32x2{a0, c0w};
      *reinterpret_cast<u32x2*>(&sX[PSTRIDE + lds]) = u32x2{a1, c1w};
    } else {
      unsigned a0, a1, a2, c0w, c1w, c2w;
      split3(v[0], v[1], a0, a1, a2);
      split3(v[2], v[3], c0w, c1w, c2w);
      *reinterpret_cast<u32x2*>(&sX[lds]) = u32x2{a0, c0w};
      *reinterpret_cast<u32x2*>(&sX[PSTRIDE + lds]) = u32x2{a1, c1w};
      *reinterpret_cast<u32x2*>(&sX[2 * PSTRIDE + lds]) = u32x2{a2, c2w};
    }
  };
  auto store_staged = [&](auto gn_tag, int c0, unsigned* sX) {
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) stage_slot(gn_tag, i, c0, sX, tid);
  };

  // operand addresses: B = 8 channels (h picks the half) of pixel (row, l31) of this wave's N tile; A = 8 input channels of
  // output channel co0 + mt*32 + l31
  // (bbase: patch row 0 of the wave's rows at the rectangle's first tap; a patch row and a tap column are immediates from there)
  const int bbase = h * HALF_WORDS + ((wn * 4 + p.dy_min + 1) * PW + l31 + p.dx_min + 1) * 4;
  // (a wave-uniform 64-bit base in scalar registers plus ONE 32-bit byte offset per lane: the loads take the base from SGPRs, and
  // no per-tap address pair occupies vector registers)
  const unsigned wlane = (unsigned)((co0 + wm * 32 + l31) * 8 + h * 4) * 4u;
  const size_t w_piece = (size_t)p.CoutPad * 8;            // words between pieces
  const size_t w_tap = NP * w_piece, w_chunk = NT * w_tap;

  // Tap-column order.  The B operand of (tap row dyi, output row nt) is patch row nt + dyi of the tap's column: it depends on
  // nt + dyi only, so per tap column a wave needs NR = 4 + NDY - 1 patch rows, not 4 NDY.  One step = (tap column dxi, patch row r):
  // the row's NP pieces are read from LDS ONCE and feed every (dyi, nt = r - dyi) with 0 <= nt < 4 -- up to NDY accumulators,
  // whose product chains are interleaved (small terms first within each accumulator).  3x3 pairs: 36 reads of 16 bytes per chunk
  // instead of 72.  The per-accumulator summation order is column-major over the taps.
  constexpr int NR = 4 + NDY - 1, STEPS = NDX * NR;
  auto load_wcol = [&](u32x4 (&wc)[NDY][NP], int chunk, int dxi, unsigned wl) {
#pragma unroll
    for (int dyi = 0; dyi < NDY; ++dyi) {
      const unsigned* wb = p.wp3 + (size_t)chunk * w_chunk + (size_t)p.tap_idx[dyi * NDX + dxi] * w_tap;     // (scalar table)
#pragma unroll
      for (int pc = 0; pc < NP; ++pc)
        wc[dyi][pc] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wb + pc * w_piece) + wl);
    }
  };
  auto load_row = [&](u32x4 (&xp)[NP], const unsigned* sX, int dxi, int r) {
#pragma unroll
    for (int pc = 0; pc < NP; ++pc) xp[pc] = *reinterpret_cast<const u32x4*>(&sX[pc * PSTRIDE + bbase + (r * PW + dxi) * 4]);
  };
  auto mma_row = [&](const u32x4 (&wc)[NDY][NP], const u32x4 (&xp)[NP], int r) {
    constexpr int NTERM = PAIR ? 3 : 6;
#pragma unroll
    for (int t = 0; t < NTERM; ++t) {
      const int tw = PAIR ? (t == 0 ? 1 : 0) : TERM_W[t], tx = PAIR ? (t == 1 ? 1 : 0) : TERM_X[t];      // pairs: w1 x0, w0 x1, w0 x0
      if (!PAIR && (HDIFF_MUTANT & 1) && tw == 0 && tx == 2) continue;
#pragma unroll
      for (int dyi = 0; dyi < NDY; ++dyi) {
        const int nt = r - dyi;
        if (nt < 0 || nt >= 4) continue;
        if constexpr (PAIR) acc[nt] = mfma_f16(wc[dyi][tw], xp[tx], acc[nt]);
        else acc[nt] = mfma_bf16(wc[dyi][tw], xp[tx], acc[nt]);
      }
    }
  };

  // Chunk loop, ONE barrier per chunk: while the matrix core works through chunk c (LDS buffer c & 1), the vector pipe turns
  // the raw patch of chunk c + 1 (in registers since the previous chunk) into split pieces in the other buffer, the NSLOT
  // staging slots spread evenly behind the steps' MFMAs; the global loads of chunk c + 2 leave once those registers are free.
  // The B operands run one step ahead.  The weight operands form ONE stream over (chunk, tap column), one column ahead of its
  // use, through two register sets of NDY taps each (a column of the 3x3 pairs is 36 MFMAs = 1 150 cycles: an L2 hit under load
  // takes about a third of that); the last column of a chunk requests the first column of the next one, so that no chunk begins
  // by waiting for its weights.  With an odd NDX that column arrives in set 1 and is moved to set 0 at the end of the chunk.
  u32x4 w[2][NDY][NP];
  auto chunk = [&](auto gn_tag, auto more_tag, int c, int nchunks) {
    constexpr bool more = decltype(more_tag)::value;      // compile time: the staging must not sit in a block of its own
    const unsigned* sX = sXbuf[c & 1];
    unsigned* sNext = sXbuf[(c + 1) & 1];
    u32x4 xp[2][NP];
    // (the thread id and the lane's weight offset behind an empty asm: what is computed from them stays inside the chunk.  Left
    //  loop-invariant, the six LDS offsets and a 64-bit vector address per tap and piece are kept in registers across the loop.)
    int t = tid;
    unsigned wl = wlane;
    asm volatile("" : "+v"(t), "+v"(wl));
    load_row(xp[0], sX, 0, 0);
#pragma unroll
    for (int dxi = 0; dxi < NDX; ++dxi) {
      // the patch registers freed by the column before: their slots of chunk c + 2 (first column: of chunk c + 1, freed by the
      // last column of chunk c - 1; the prologue has loaded all of chunk 1)
      if (dxi == 0 ? (c > 0 && c + 1 < nchunks) : (c + 2 < nchunks)) {
#pragma unroll
        for (int i = 0; i < NSLOT; ++i)
          if ((((i + 1) * STEPS) / NSLOT - 1) / NR == (dxi + NDX - 1) % NDX) load_slot(i, (dxi == 0 ? c + 1 : c + 2) * 16);
      }
      if (dxi + 1 < NDX) load_wcol(w[(dxi + 1) & 1], c, dxi + 1, wl);
      else if (more) load_wcol(w[NDX & 1], c + 1, 0, wl);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int g = dxi * NR + r;
        if (g + 1 < STEPS) load_row(xp[(g + 1) & 1], sX, (g + 1) / NR, (g + 1) % NR);
        mma_row(w[dxi & 1], xp[g & 1], r);
        if (more) {
#pragma unroll
          for (int i = 0; i < NSLOT; ++i)
            if (((i + 1) * STEPS) / NSLOT - 1 == g) stage_slot(gn_tag, i, (c + 1) * 16, sNext, t);
        }
      }
    }
    if (more && (NDX & 1)) {
#pragma unroll
      for (int dyi = 0; dyi < NDY; ++dyi)
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) w[0][dyi][pc] = w[1][dyi][pc];
    }
    __syncthreads();
  };

  // Tap-major order (the bf16-triple and the DROP instantiations: with a column of weight sets in flight beside the column in use
  // they do not fit 256 registers -- profiles/conv_tap_columns.txt).  The taps of the rectangle are walked one by one, COLUMN by
  // column: every accumulator sums in the order of the column form, so the two forms give the same bits.  A tap is four units,
  // one per output row, of NP (NP + 1) / 2 MFMAs each, and every unit has a B read of its own.  The B operands run one unit
  // ahead, the weights two taps ahead through a ring of three sets (WSTREAM: a tap count that is a multiple of three keeps the
  // ring's phase from chunk to chunk); one staging slot behind each tap's MFMAs, its registers reloaded at the start of the
  // next tap.
  constexpr bool WSTREAM = (NT % 3 == 0);
  u32x4 wr[3][NP];
  auto load_w = [&](u32x4 (&wa)[NP], int chunk, int tap, unsigned wl) {
    const unsigned* wb = p.wp3 + (size_t)chunk * w_chunk + (size_t)p.tap_idx[(tap % NDY) * NDX + tap / NDY] * w_tap;
#pragma unroll
    for (int pc = 0; pc < NP; ++pc) wa[pc] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wb + pc * w_piece) + wl);
  };
  auto mma_unit = [&](const u32x4 (&wa)[NP], const u32x4 (&xp)[NP], int nt) {
    if constexpr (PAIR) {                  // small products first
      acc[nt] = mfma_f16(wa[1], xp[0], acc[nt]);
      acc[nt] = mfma_f16(wa[0], xp[1], acc[nt]);
      acc[nt] = mfma_f16(wa[0], xp[0], acc[nt]);
    } else {
#pragma unroll
      for (int t = 0; t < 6; ++t)
        if (!((HDIFF_MUTANT & 1) && TERM_W[t] == 0 && TERM_X[t] == 2)) acc[nt] = mfma_bf16(wa[TERM_W[t]], xp[TERM_X[t]], acc[nt]);
    }
  };
  auto chunk_taps = [&](auto gn_tag, auto more_tag, int c, int nchunks) {
    constexpr bool more = decltype(more_tag)::value;
    const unsigned* sX = sXbuf[c & 1];
    unsigned* sNext = sXbuf[(c + 1) & 1];
    u32x4 xp[2][NP];
    int t = tid;
    unsigned wl = wlane;
    asm volatile("" : "+v"(t), "+v"(wl));
    if (!WSTREAM || c == 0) {
      load_w(wr[0], c, 0, wl);
      load_w(wr[1], c, 1, wl);
    }
    load_row(xp[0], sX, 0, 0);          // unit (tap, nt) reads patch row nt + tap % NDY of tap column tap / NDY
#pragma unroll
    for (int tap = 0; tap < NT; ++tap) {
      // slot i is staged behind tap min(i, NT - 1); its registers take chunk c + 2 at the next tap, those of the last tap chunk
      // c + 1 at the first tap of the next chunk
      if (tap == 0 ? (c > 0 && c + 1 < nchunks) : (c + 2 < nchunks)) {
#pragma unroll
        for (int i = 0; i < NSLOT; ++i)
          if ((i < NT - 1 ? i : NT - 1) == (tap + NT - 1) % NT) load_slot(i, (tap == 0 ? c + 1 : c + 2) * 16);
      }
      if (tap + 2 < NT) load_w(wr[(tap + 2) % 3], c, tap + 2, wl);
      else if (WSTREAM && more) load_w(wr[(tap + 2) % 3], c + 1, tap + 2 - NT, wl);      // the next chunk's first two taps
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int u = tap * 4 + nt;
        if (u + 1 < 4 * NT) load_row(xp[(u + 1) & 1], sX, ((u + 1) / 4) / NDY, (u + 1) % 4 + ((u + 1) / 4) % NDY);
        mma_unit(wr[tap % 3], xp[u & 1], nt);
      }
      if (more) {
#pragma unroll
        for (int i = 0; i < NSLOT; ++i)
          if ((i < NT - 1 ? i : NT - 1) == tap) stage_slot(gn_tag, i, (c + 1) * 16, sNext, t);
      }
    }
    __syncthreads();
  };
  // which of the two: the column order where it fits the registers of two waves per SIMD without scratch
  constexpr bool COLS = PAIR && !DROP;
  auto run_chunk = [&](auto gn_tag, auto more_tag, int c, int nchunks) {
    if constexpr (COLS) chunk(gn_tag, more_tag, c, nchunks);
    else chunk_taps(gn_tag, more_tag, c, nchunks);
  };

  const int nchunks = p.Cin / 16;
  issue_loads(0);
  fetch_keep(0, 0, 0u);
  __syncthreads();     // sG visible
  if (has_gn) store_staged(std::true_type{}, 0, sXbuf[0]);
  else store_staged(std::false_type{}, 0, sXbuf[0]);
  if (nchunks > 1) issue_loads(16);
  if constexpr (COLS) load_wcol(w[0], 0, 0, wlane);
  __syncthreads();
  if (has_gn) {
    for (int c = 0; c + 1 < nchunks; ++c) run_chunk(std::true_type{}, std::true_type{}, c, nchunks);
    run_chunk(std::true_type{}, std::false_type{}, nchunks - 1, nchunks);
  } else {
    for (int c = 0; c + 1 < nchunks; ++c) run_chunk(std::false_type{}, std::true_type{}, c, nchunks);
    run_chunk(std::false_type{}, std::false_type{}, nchunks - 1, nchunks);
  }

  // ---- epilogue: + bias + per-sample channel vector + residual, NCHW store (32 consecutive pixels per register row).
  // A full tile (workgroup-uniform test: everything but edge tiles and a channel tail) takes the branch-free form: the 16
  // bias / vector values of the lane's channels are fetched together, then per pixel row all 16 residual loads are in
  // flight before the first add -- with per-element tests every output waited for its own three loads in turn (64 dependent
  // round trips per lane: a quarter of the kernel's time at 128 channels).
  if constexpr (PAIR) {                    // out of the scaled domain: 2^-(s + t), exact
    const float os = xinv * p.w_scale[1];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] *= os;
  }
  const size_t OHW = OUTMAP ? (size_t)p.OH * p.OW : HW;
  const int osy = OUTMAP ? p.out_sy : 1, ooy = OUTMAP ? p.out_oy : 0, osx = OUTMAP ? p.out_sx : 1, oox = OUTMAP ? p.out_ox : 0;
  const int OW = OUTMAP ? p.OW : p.W;
  // absmax_out: the maximum of |v| over what this wave stores, as bits (non-negative floats order like unsigned integers, NaN
  // above inf above every finite value), reduced over the wave and combined into the sample's word by ONE atomicMax
  // (Behind a workgroup-uniform test: a launch without the word -- most of a step's -- executes none of it.)
  const bool track = p.absmax_out != nullptr;
  unsigned amax = 0u;
  auto post_absmax = [&]() {
    if (!track) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned other = (unsigned)__shfl_xor((int)amax, o, 64);
      amax = other > amax ? other : amax;
    }
    if (lane == 0) atomicMax(&p.absmax_out[b], amax);
  };
  if (co0 + 64 <= p.Cout && vy0 + 8 <= p.H && vx0 + 32 <= p.W) {
    float add[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      float a = 0.f;
      if (p.bias) a += p.bias[co];
      if (p.addvec) a += p.addvec[b * p.Cout + co];
      add[r] = a;
    }
    const size_t lane_base = ((size_t)b * p.Cout + co0 + wm * 32 + 4 * h) * OHW +
                             (size_t)((vy0 + wn * 4) * osy + ooy) * OW + (size_t)(vx0 + l31) * osx + oox;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const size_t row = lane_base + (size_t)(nt * osy) * OW;
      float res[16];
      if (p.residual) {
#pragma unroll
        for (int r = 0; r < 16; ++r) res[r] = p.residual[row + (size_t)((r & 3) + 8 * (r >> 2)) * OHW];
      }
      float vv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v;
        if (p.residual_first) v = (acc[nt][r] + res[r]) + add[r];       // (only with a residual: the parity-plane launches)
        else {
          v = acc[nt][r] + add[r];
          if (p.residual) v += res[r];
        }
        p.out[row + (size_t)((r & 3) + 8 * (r >> 2)) * OHW] = v;
        vv[r] = v;
      }
      if (track) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned vb = __builtin_bit_cast(unsigned, vv[r]) & 0x7fffffffu;
          amax = vb > amax ? vb : amax;
        }
      }
    }
    post_absmax();
    return;
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int vy = vy0 + wn * 4 + nt, vx = vx0 + l31;
    if (vy >= p.H || vx >= p.W) continue;
    const size_t pix = (size_t)(vy * osy + ooy) * OW + (size_t)vx * osx + oox;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co < p.Cout) {
        float a = 0.f;                               // the same order of additions as the full-tile form
        if (p.bias) a += p.bias[co];
        if (p.addvec) a += p.addvec[b * p.Cout + co];
        const size_t o = ((size_t)b * p.Cout + co) * OHW + pix;
        float v;
        if (p.residual_first) v = (acc[nt][r] + p.residual[o]) + a;
        else {
          v = acc[nt][r] + a;
          if (p.residual) v += p.residual[o];
        }
        p.out[o] = v;
        if (track) {
          const unsigned vb = __builtin_bit_cast(unsigned, v) & 0x7fffffffu;
          amax = vb > amax ? vb : amax;
        }
      }
    }
  }
  post_absmax();
}

// fp32 weights -> [Cin/16][tap][piece][CoutPad][8 words]: word j of a row = bf16 pieces of input channels 2j, 2j+1.  Tap t
// reads kernel element (ky[t], kx[t]) of a KH x KW kernel stored [Cout][Cin][KH][KW] (mode 0) or [Cin][Cout][KH][KW] (mode 1:
// nn.ConvTranspose2d's layout, and the layout of a forward weight seen from its input-gradient convolution).
struct PackX3K {
  int mode, Cout, Cin, KH, KW, ntaps, CoutPad;
  int CinPad;        // mode 2 (fp16 pairs only): w is an fp32 pack [KH * KW][CinPad][CoutPad] of hdiff_pack_conv_weight
  int ky[9], kx[9];
};
__global__ void pack_conv_weight_x3_kernel(const float* __restrict__ w, unsigned* __restrict__ wp3, const PackX3K q) {
  const size_t n = (size_t)(q.Cin / 16) * q.ntaps * q.CoutPad * 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % 8);
    size_t r = i / 8;
    const int co = (int)(r % q.CoutPad);
    r /= q.CoutPad;
    const int tap = (int)(r % q.ntaps);
    const int chunk = (int)(r / q.ntaps);
    float a = 0.f, c = 0.f;
    if (co < q.Cout) {
      const int ci = chunk * 16 + 2 * j;
      const size_t k = (size_t)q.ky[tap] * q.KW + q.kx[tap], kk = (size_t)q.KH * q.KW;
      if (q.mode == 1) {
        a = w[((size_t)ci * q.Cout + co) * kk + k];
        c = w[((size_t)(ci + 1) * q.Cout + co) * kk + k];
      } else {
        a = w[((size_t)co * q.Cin + ci) * kk + k];
        c = w[((size_t)co * q.Cin + ci + 1) * kk + k];
      }
    }
    unsigned h0, h1, h2;
    split3(a, c, h0, h1, h2);
    const size_t base = ((size_t)(chunk * q.ntaps + tap) * 3) * q.CoutPad * 8 + (size_t)co * 8 + j;
    wp3[base] = h0;
    wp3[base + (size_t)q.CoutPad * 8] = h1;
    wp3[base + 2 * (size_t)q.CoutPad * 8] = h2;
  }
}

// ---- fp16-pair weights: [Cin/16][tap][2 pieces][CoutPad][8 words] of w 2^t, then a tail of 4 words:
//      {bits of max |w| (scratch of the pack), 2^-t, 2^t, 0}.  Two launches: the maximum, then the split.
__global__ void conv_weight_absmax_kernel(const float* __restrict__ w, size_t n, unsigned* __restrict__ tail) {
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(w[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(tail, __builtin_bit_cast(unsigned, m));      // non-negative floats order like unsigned integers
}
__global__ void pack_conv_weight_h2_kernel(const float* __restrict__ w, unsigned* __restrict__ wp2, unsigned* __restrict__ tail,
                                           const PackX3K q, float one) {
  const size_t n = (size_t)(q.Cin / 16) * q.ntaps * q.CoutPad * 8;
  // 2^t with max |w| 2^t in [2^14, 2^15); an all-zero / denormal / non-finite tensor gets a fixed scale (inf and NaN stay what they are)
  int e = (int)((tail[0] >> 23) & 0xffu) - 127;
  e = e < -60 ? -60 : (e > 60 ? 60 : e);
  const float sc = __builtin_bit_cast(float, (unsigned)(14 - e + 127) << 23);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % 8);
    size_t r = i / 8;
    const int co = (int)(r % q.CoutPad);
    r /= q.CoutPad;
    const int tap = (int)(r % q.ntaps);
    const int chunk = (int)(r / q.ntaps);
    float a = 0.f, c = 0.f;
    if (co < q.Cout) {
      const int ci = chunk * 16 + 2 * j;
      const size_t k = (size_t)q.ky[tap] * q.KW + q.kx[tap], kk = (size_t)q.KH * q.KW;
      if (q.mode == 2) {
        a = w[(k * q.CinPad + ci) * q.CoutPad + co];
        c = w[(k * q.CinPad + ci + 1) * q.CoutPad + co];
      } else if (q.mode == 1) {
        a = w[((size_t)ci * q.Cout + co) * kk + k];
        c = w[((size_t)(ci + 1) * q.Cout + co) * kk + k];
      } else {
        a = w[((size_t)co * q.Cin + ci) * kk + k];
        c = w[((size_t)co * q.Cin + ci + 1) * kk + k];
      }
    }
    unsigned h0, h1;
    split2(a * sc, c * sc, one, h0, h1);
    const size_t base = ((size_t)(chunk * q.ntaps + tap) * 2) * q.CoutPad * 8 + (size_t)co * 8 + j;
    wp2[base] = h0;
    wp2[base + (size_t)q.CoutPad * 8] = h1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {          // (the groups of a plane-grouped pack all write the same values)
    reinterpret_cast<float*>(tail)[1] = __builtin_bit_cast(float, (unsigned)(e - 14 + 127) << 23);
    reinterpret_cast<float*>(tail)[2] = sc;
    tail[3] = 0u;
  }
}

// out[0] = 2^s, out[1] = 2^-s with (sqrt(n - 1) max |gamma| + max |beta|) 2^s in [2^13, 2^14): the bound of a GroupNorm + Swish
// output (header) with a factor of two to spare.  One workgroup.
__global__ void gn_act_scale_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, int C, float sqrt_n1,
                                    float gain, float* __restrict__ out) {
  __shared__ float red[4];
  float m = 0.f;
  for (int i = threadIdx.x; i < C; i += blockDim.x) m = fmaxf(m, fmaf(sqrt_n1, fabsf(gamma[i]), fabsf(beta[i])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * gain;
    int e = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu) - 127;
    e = e < -60 ? -60 : (e > 60 ? 60 : e);           // NaN / inf weights: a fixed scale, the activations are NaN anyway
    out[0] = __builtin_bit_cast(float, (unsigned)(13 - e + 127) << 23);
    out[1] = __builtin_bit_cast(float, (unsigned)(e - 13 + 127) << 23);
  }
}

}  // namespace

namespace hdiff {

void launch_conv3x3_x3(const ConvX3K& k, int B, hipStream_t stream) {
  const int tiles_y = cdiv(k.H, 8);
  dim3 grid(k.tiles_x * tiles_y, cdiv(k.Cout, 64), B);
  const size_t dyn = (size_t)2 * k.Cin * sizeof(float);
  const bool outmap = !(k.out_sy == 1 && k.out_oy == 0 && k.out_sx == 1 && k.out_ox == 0 && k.OH == k.H && k.OW == k.W);
  const int rect = k.ndy * 10 + k.ndx;     // 33, 32, 23 or 22 (conv_tap_rect)
#define HDIFF_X3_LAUNCH(NDY, NDX, ...) \
  hipLaunchKernelGGL((conv3x3_x3_kernel<NDY, NDX, __VA_ARGS__>), grid, dim3(THREADS), dyn, stream, k)
  if (k.keep_bits != nullptr) {            // train-mode dropout in the prologue (hdiff_conv2d_fwd_dropout checked the descriptor)
    if (k.act_scale != nullptr) HDIFF_X3_LAUNCH(3, 3, false, true, 2, true);
    else HDIFF_X3_LAUNCH(3, 3, false, false, 2, true);
    return;
  }
  if (k.act_scale != nullptr || k.absmax_in != nullptr) {      // fp16 pairs: the input's range is known (the dispatcher checked the shape)
    if (rect == 33 && !outmap) HDIFF_X3_LAUNCH(3, 3, false, true);
    else if (rect == 33) HDIFF_X3_LAUNCH(3, 3, true, true);
    else if (rect == 32 && !outmap) HDIFF_X3_LAUNCH(3, 2, false, true);      // (parity planes of the 5x5 / s2 ...
    else if (rect == 23 && !outmap) HDIFF_X3_LAUNCH(2, 3, false, true);
    else if (rect == 22 && !outmap) HDIFF_X3_LAUNCH(2, 2, false, true);
    else if (rect == 32) HDIFF_X3_LAUNCH(3, 2, true, true);                  //  ... transposed-conv phases)
    else if (rect == 23) HDIFF_X3_LAUNCH(2, 3, true, true);
    else HDIFF_X3_LAUNCH(2, 2, true, true);
    return;
  }
  if (rect == 33 && !outmap) HDIFF_X3_LAUNCH(3, 3, false, false);
  else if (rect == 33) HDIFF_X3_LAUNCH(3, 3, true, false);
  else if (rect == 32) HDIFF_X3_LAUNCH(3, 2, true, false);
  else if (rect == 23) HDIFF_X3_LAUNCH(2, 3, true, false);
  else HDIFF_X3_LAUNCH(2, 2, true, false);
#undef HDIFF_X3_LAUNCH
}

// The taps of a launch as a rectangle: fills ndy, ndx, dy_min, dx_min and tap_idx (tap t of the list = tap t of the pack) and
// returns true if the ntaps distinct offsets, all in [-1, 1]^2, are exactly the 3x3, 3x2, 2x3 or 2x2 rectangle they span.
bool conv_tap_rect(ConvTapRect& k, int ntaps, const int* dy, const int* dx) {
  if (ntaps < 1 || ntaps > 9) return false;
  int y0 = 1, y1 = -1, x0 = 1, x1 = -1;
  for (int t = 0; t < ntaps; ++t) {
    if (dy[t] < -1 || dy[t] > 1 || dx[t] < -1 || dx[t] > 1) return false;
    y0 = dy[t] < y0 ? dy[t] : y0; y1 = dy[t] > y1 ? dy[t] : y1;
    x0 = dx[t] < x0 ? dx[t] : x0; x1 = dx[t] > x1 ? dx[t] : x1;
  }
  const int ndy = y1 - y0 + 1, ndx = x1 - x0 + 1;
  if (ndy < 2 || ndx < 2 || ndy * ndx != ntaps) return false;
  for (int i = 0; i < 9; ++i) k.tap_idx[i] = i < ntaps ? -1 : 0;
  for (int t = 0; t < ntaps; ++t) {
    int& slot = k.tap_idx[(dy[t] - y0) * ndx + (dx[t] - x0)];
    if (slot >= 0) return false;               // a tap listed twice
    slot = t;
  }
  k.ntaps = ntaps; k.ndy = ndy; k.ndx = ndx; k.dy_min = y0; k.dx_min = x0;
  return true;
}

}  // namespace hdiff

static int pack_x3(const float* w, void* wp3, int mode, int Cout, int Cin, int KH, int KW, int ntaps, const int* ky, const int* kx,
                   int CoutPad, hipStream_t stream) {
  PackX3K q{};
  q.mode = mode; q.Cout = Cout; q.Cin = Cin; q.KH = KH; q.KW = KW; q.ntaps = ntaps; q.CoutPad = CoutPad;
  for (int t = 0; t < ntaps; ++t) { q.ky[t] = ky[t]; q.kx[t] = kx[t]; }
  const size_t n = (size_t)(Cin / 16) * ntaps * CoutPad * 8;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(pack_conv_weight_x3_kernel, dim3(blocks), dim3(256), 0, stream, w, (unsigned*)wp3, q);
  HDIFF_CHECK_LAUNCH("pack_conv_weight_x3_kernel");
  return HDIFF_OK;
}

extern "C" int hdiff_pack_conv_weight_x3(const float* w, void* wp3, int Cout, int Cin, int CoutPad, int transposed,
                                         hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(w && wp3, "pack_conv_weight_x3: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0,
                  "pack_conv_weight_x3: needs Cin %% 16 == 0 and CoutPad %% 64 == 0 (Cin %d, Cout %d, CoutPad %d)", Cin, Cout, CoutPad);
  int ky[9], kx[9];
  for (int t = 0; t < 9; ++t) {                 // the input-gradient conv reads the forward weight transposed and tap-mirrored
    ky[t] = transposed ? 2 - t / 3 : t / 3;
    kx[t] = transposed ? 2 - t % 3 : t % 3;
  }
  return pack_x3(w, wp3, transposed ? 1 : 0, Cout, Cin, 3, 3, 9, ky, kx, CoutPad, (hipStream_t)stream);
}

extern "C" int hdiff_pack_conv_weight_h2_words(int Cout, int Cin, int CoutPad, int64_t* words_out) {
  HDIFF_CHECK_ARG(words_out, "pack_conv_weight_h2_words: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0,
                  "pack_conv_weight_h2_words: needs Cin %% 16 == 0 and CoutPad %% 64 == 0 (Cin %d, Cout %d, CoutPad %d)", Cin, Cout, CoutPad);
  *words_out = (int64_t)(Cin / 16) * 9 * 2 * CoutPad * 8 + 4;
  return HDIFF_OK;
}

// the maximum over the WHOLE weight tensor, then the split of the listed taps: one 2^t per pack (the phases of one transposed
// conv share it)
static int pack_h2(const char* who, const float* w, void* wp2, int mode, int Cout, int Cin, int KH, int KW, int ntaps, const int* ky,
                   const int* kx, int CoutPad, hipStream_t stream) {
  PackX3K q{};
  q.mode = mode; q.Cout = Cout; q.Cin = Cin; q.KH = KH; q.KW = KW; q.ntaps = ntaps; q.CoutPad = CoutPad;
  for (int t = 0; t < ntaps; ++t) { q.ky[t] = ky[t]; q.kx[t] = kx[t]; }
  const size_t n = (size_t)(Cin / 16) * ntaps * CoutPad * 8, nw = (size_t)Cout * Cin * KH * KW;
  unsigned* tail = (unsigned*)wp2 + 2 * n;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  const int mblocks = (int)((nw + 255) / 256 < 1024 ? (nw + 255) / 256 : 1024);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  if (hipMemsetAsync(tail, 0, 16, stream) != hipSuccess) {
    hdiff::set_error("%s: hipMemsetAsync failed", who);
    return HDIFF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(conv_weight_absmax_kernel, dim3(mblocks), dim3(256), 0, stream, w, nw, tail);
  HDIFF_CHECK_LAUNCH("conv_weight_absmax_kernel");
  hipLaunchKernelGGL(pack_conv_weight_h2_kernel, dim3(blocks), dim3(256), 0, stream, w, (unsigned*)wp2, tail, q, 1.0f);
  HDIFF_CHECK_LAUNCH("pack_conv_weight_h2_kernel");
  return HDIFF_OK;
}

// ---- the 5x5 / stride-2 conv as four stride-1 convs over the input's parity planes (conv_igemm.hip issues them): plane (oy, ox)
//      holds the taps with ky % 2 == oy, kx % 2 == ox, which read plane pixel (y + dy, x + dx) with dy = (ky - 2 - oy) / 2 in
//      {-1, 0, 1} (oy = 0) or {-1, 0} (oy = 1).  Pack: the groups (0,0), (0,1), (1,0), (1,1) with 9 / 6 / 6 / 4 taps one after the
//      other, each [Cin/16][taps][2][CoutPad][8], then ONE tail: one 2^t for all four.
namespace hdiff {
int s2_plane_taps(int oy, int ox, int* ky, int* kx) {
  int n = 0;
  for (int y = oy; y < 5; y += 2)
    for (int x = ox; x < 5; x += 2) { ky[n] = y; kx[n] = x; ++n; }
  return n;
}
}  // namespace hdiff

extern "C" int hdiff_pack_conv_weight_h2_s2_words(int Cout, int Cin, int CoutPad, int64_t* words_out) {
  HDIFF_CHECK_ARG(words_out, "pack_conv_weight_h2_s2_words: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0,
                  "pack_conv_weight_h2_s2_words: needs Cin %% 16 == 0 and CoutPad %% 64 == 0 (Cin %d, Cout %d, CoutPad %d)", Cin, Cout,
                  CoutPad);
  *words_out = (int64_t)(Cin / 16) * 25 * 2 * CoutPad * 8 + 4;
  return HDIFF_OK;
}

extern "C" int hdiff_pack_conv_weight_h2_s2(const float* wp, void* wp2, int Cout, int Cin, int CinPad, int CoutPad, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(wp && wp2, "pack_conv_weight_h2_s2: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CinPad >= Cin && CinPad % 8 == 0 && CoutPad >= Cout && CoutPad % 64 == 0,
                  "pack_conv_weight_h2_s2: needs Cin %% 16 == 0, CinPad %% 8 == 0 and CoutPad %% 64 == 0 (Cin %d, CinPad %d, Cout %d, CoutPad %d)",
                  Cin, CinPad, Cout, CoutPad);
  const size_t per_tap = (size_t)(Cin / 16) * 2 * CoutPad * 8, nw = (size_t)25 * CinPad * CoutPad;
  unsigned* tail = (unsigned*)wp2 + 25 * per_tap;
  const int mblocks = (int)((nw + 255) / 256 < 1024 ? (nw + 255) / 256 : 1024);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  if (hipMemsetAsync(tail, 0, 16, (hipStream_t)stream) != hipSuccess) {
    hdiff::set_error("pack_conv_weight_h2_s2: hipMemsetAsync failed");
    return HDIFF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(conv_weight_absmax_kernel, dim3(mblocks), dim3(256), 0, (hipStream_t)stream, wp, nw, tail);      // (the padding is zero)
  HDIFF_CHECK_LAUNCH("conv_weight_absmax_kernel");
  size_t taps_before = 0;
  for (int g = 0; g < 4; ++g) {
    PackX3K q{};
    q.mode = 2; q.Cout = Cout; q.Cin = Cin; q.KH = 5; q.KW = 5; q.CoutPad = CoutPad; q.CinPad = CinPad;
    q.ntaps = hdiff::s2_plane_taps(g >> 1, g & 1, q.ky, q.kx);
    const size_t n = per_tap / 2 * q.ntaps;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv_weight_h2_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, wp, (unsigned*)wp2 + taps_before * per_tap,
                       tail, q, 1.0f);
    HDIFF_CHECK_LAUNCH("pack_conv_weight_h2_kernel");
    taps_before += q.ntaps;
  }
  return HDIFF_OK;
}

extern "C" int hdiff_pack_conv_weight_h2(const float* w, void* wp2, int Cout, int Cin, int CoutPad, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(w && wp2, "pack_conv_weight_h2: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0,
                  "pack_conv_weight_h2: needs Cin %% 16 == 0 and CoutPad %% 64 == 0 (Cin %d, Cout %d, CoutPad %d)", Cin, Cout, CoutPad);
  int ky[9], kx[9];
  for (int t = 0; t < 9; ++t) { ky[t] = t / 3; kx[t] = t % 3; }
  return pack_h2("pack_conv_weight_h2", w, wp2, 0, Cout, Cin, 3, 3, 9, ky, kx, CoutPad, (hipStream_t)stream);
}

extern "C" int hdiff_pack_conv_weight_h2_taps_words(int Cout, int Cin, int CoutPad, int ntaps, int64_t* words_out) {
  HDIFF_CHECK_ARG(words_out, "pack_conv_weight_h2_taps_words: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0,
                  "pack_conv_weight_h2_taps_words: needs Cin %% 16 == 0 and CoutPad %% 64 == 0 (Cin %d, Cout %d, CoutPad %d)", Cin, Cout,
                  CoutPad);
  HDIFF_CHECK_ARG(ntaps >= 1 && ntaps <= 9, "pack_conv_weight_h2_taps_words: ntaps %d out of range", ntaps);
  *words_out = (int64_t)(Cin / 16) * ntaps * 2 * CoutPad * 8 + 4;
  return HDIFF_OK;
}

extern "C" int hdiff_pack_conv_weight_h2_taps(const float* w, void* wp2, int mode, int Cout, int Cin, int KH, int KW, int ntaps,
                                              const int* tap_ky, const int* tap_kx, int CoutPad, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(w && wp2 && tap_ky && tap_kx, "pack_conv_weight_h2_taps: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0 && (mode == 0 || mode == 1),
                  "pack_conv_weight_h2_taps: needs Cin %% 16 == 0, CoutPad %% 64 == 0, mode 0 / 1 (Cin %d, Cout %d, CoutPad %d, mode %d)",
                  Cin, Cout, CoutPad, mode);
  HDIFF_CHECK_ARG(ntaps >= 1 && ntaps <= 9 && KH > 0 && KW > 0, "pack_conv_weight_h2_taps: ntaps %d out of range", ntaps);
  for (int t = 0; t < ntaps; ++t)
    HDIFF_CHECK_ARG(tap_ky[t] >= 0 && tap_ky[t] < KH && tap_kx[t] >= 0 && tap_kx[t] < KW,
                    "pack_conv_weight_h2_taps: tap %d reads kernel element (%d, %d) of a %d x %d kernel", t, tap_ky[t], tap_kx[t], KH, KW);
  return pack_h2("pack_conv_weight_h2_taps", w, wp2, mode, Cout, Cin, KH, KW, ntaps, tap_ky, tap_kx, CoutPad, (hipStream_t)stream);
}

extern "C" int hdiff_gn_act_scale(const float* gamma, const float* beta, int C, int64_t group_elems, float gain, float* out2,
                                  hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(gamma && beta && out2, "gn_act_scale: null pointer");
  HDIFF_CHECK_ARG(C > 0 && group_elems > 0 && gain >= 1.0f && gain <= 1024.0f, "gn_act_scale: bad sizes (C %d, gain %g)", C, (double)gain);
  (void)hipGetLastError();  // drop any stale error left by another HIP user in this thread
  hipLaunchKernelGGL(gn_act_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, gamma, beta, C,
                     sqrtf((float)(group_elems > 1 ? group_elems - 1 : 1)), gain, out2);
  HDIFF_CHECK_LAUNCH("gn_act_scale_kernel");
  return HDIFF_OK;
}

extern "C" int hdiff_pack_conv_weight_x3_taps(const float* w, void* wp3, int mode, int Cout, int Cin, int KH, int KW, int ntaps,
                                              const int* tap_ky, const int* tap_kx, int CoutPad, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(w && wp3 && tap_ky && tap_kx, "pack_conv_weight_x3_taps: null pointer");
  HDIFF_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 16 == 0 && CoutPad >= Cout && CoutPad % 64 == 0 && (mode == 0 || mode == 1),
                  "pack_conv_weight_x3_taps: needs Cin %% 16 == 0, CoutPad %% 64 == 0, mode 0 / 1 (Cin %d, Cout %d, CoutPad %d, mode %d)",
                  Cin, Cout, CoutPad, mode);
  HDIFF_CHECK_ARG(ntaps >= 1 && ntaps <= 9 && KH > 0 && KW > 0, "pack_conv_weight_x3_taps: ntaps %d out of range", ntaps);
  for (int t = 0; t < ntaps; ++t)
    HDIFF_CHECK_ARG(tap_ky[t] >= 0 && tap_ky[t] < KH && tap_kx[t] >= 0 && tap_kx[t] < KW,
                    "pack_conv_weight_x3_taps: tap %d reads kernel element (%d, %d) of a %d x %d kernel", t, tap_ky[t], tap_kx[t], KH, KW);
  return pack_x3(w, wp3, mode, Cout, Cin, KH, KW, ntaps, tap_ky, tap_kx, CoutPad, (hipStream_t)stream);
}
