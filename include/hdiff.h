/*
 * hdiff.h -- C ABI of the MI355X (gfx950) CFG-DDPM hot path.
 *
 * One shared library (libhdiff.so, built from hybrid-diffusion-underwater-atmopheric-image-enhancement_amd/csrc)
 * exports every operator the reference's hot path calls through PyTorch.  The reference
 * has no FFI of its own for this path: its "operator interface" is the set of ATen call sites listed beside each entry
 * point below (paths relative to the reference checkout).  All entry points
 *   - take plain device pointers, sizes and a HIP stream (void* = hipStream_t); no torch types,
 *   - are stream-ordered and stateless (no allocation, no synchronisation: safe under hipGraph capture),
 *   - return 0 on success or a negative hdiff_status; hdiff_last_error() gives the text,
 *   - compute in fp32 (fp32-input MFMA for every contraction); tensors are fp32 NCHW contiguous, indices int64.
 */
#ifndef HDIFF_H_
#define HDIFF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hdiff_stream_t; /* hipStream_t */

enum hdiff_status {
  HDIFF_OK = 0,
  HDIFF_ERR_INVALID = -1,  /* bad shape / unsupported configuration */
  HDIFF_ERR_LAUNCH = -2,   /* HIP launch error */
  HDIFF_ERR_NO_DEVICE = -3
};

int hdiff_abi_version(void);
const char* hdiff_last_error(void);
/* Number of HIP devices visible (0 without a GPU); never initialises a context. */
int hdiff_device_count(void);
/* How the fp32 matrix contractions of the attention core and of the 3x3 convolutions are carried out (process-wide, read
 * at launch time):
 *   HDIFF_CONTRACT_F32    (0, default)  fp32-input MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2)
 *   HDIFF_CONTRACT_BF16X3 (1)           each fp32 operand as three bf16 pieces, the six products with i+j<=2 on the bf16
 *                                       MFMA with fp32 accumulation: fp32-class error (about 2^-22 relative per product),
 *                                       about 1.5x faster; shapes it does not cover silently use the fp32 kernels
 *                                       (attention: d_head 16/32, L % 64 == 0; conv: 3x3 stride 1 with Cin % 16 == 0 and a
 *                                       descriptor that carries wp_x3).
 *   HDIFF_CONTRACT_F16    (2, opt-in)   a mode for SAMPLING.  Everything runs what HDIFF_CONTRACT_BF16X3 runs, bit for bit,
 *                                       except ONE dispatch: hdiff_mha_flash_fwd_ws called with lse2 == NULL (nobody will
 *                                       differentiate through it), d_head 16 or 32, L >= 512, L % 256 == 0 and a workspace of
 *                                       hdiff_mha_flash_fwd_workspace bytes.  That call carries each operand as ONE fp16 piece
 *                                       (q 2^-a, k 2^a balanced per head, v 2^s per channel row; P = fp16(exp2(S)) under a
 *                                       moving softmax reference) with fp32 accumulation (attention_f16.hip).  What it does
 *                                       NOT change: convolutions, the attention backward, a forward that returns the
 *                                       log-sum-exp (training), other head widths, calls without workspace.  Accuracy class:
 *                                       half-precision operands -- the output's error against float64 is about 1e-4 .. 5e-4
 *                                       rms of a channel's largest output (3e-3 for near-uniform rows), against about 1e-6
 *                                       in the other two modes; NOT an fp32-class result.
 * The initial value comes from the environment variable HDIFF_CONTRACT ("f32" | "bf16x3" | "f16"). */
enum { HDIFF_CONTRACT_F32 = 0, HDIFF_CONTRACT_BF16X3 = 1, HDIFF_CONTRACT_F16 = 2 };
int hdiff_set_contraction_mode(int mode);
int hdiff_get_contraction_mode(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Convolutions (K1-K4).  Replaces nn.Conv2d / nn.ConvTranspose2d call sites
 *   DiffusionFreeGuidence/ModelCondition.py:71-75 (DownSample), :82-88 (UpSample), :172,:186,:192 (ResBlock),
 *   :219 (head), :251 (tail) and the packed in/out projections of nn.MultiheadAttention (:189) viewed as 1x1 convs.
 *
 * Weights are consumed in a packed layout wp[tap][CinPad][CoutPad] (CoutPad % 64 == 0, CinPad % 8 == 0, zero padded),
 * produced on the device by hdiff_pack_conv_weight from the PyTorch layouts.
 * ------------------------------------------------------------------------------------------------------------------ */

#define HDIFF_MAX_TAPS 25

/* mode 0: Conv2d weight [Cout][Cin][KH][KW]; mode 1: ConvTranspose2d weight [Cin][Cout][KH][KW].
 * tap t of the packed tensor takes kernel element (tap_ky[t], tap_kx[t]).  accumulate != 0 adds into wp (used to fold
 * DownSample's 3x3 into the centre of its 5x5: ModelCondition.py:75 computes c1(x)+c2(x) on the same input). */
int hdiff_pack_conv_weight(const float* w, float* wp, int mode, int Cout, int Cin, int KH, int KW, int ntaps,
                           const int* tap_ky, const int* tap_kx, int CinPad, int CoutPad, int accumulate,
                           hdiff_stream_t stream);

/* Weights of a standard 3x3 conv ([Cout][Cin][3][3], Cin % 16 == 0) as three bf16 pieces per value, laid out
 * [Cin/16][tap][piece][CoutPad][16] for conv3x3_x3.hip; wp3 holds (Cin/16)*9*3*CoutPad*8 32-bit words.
 * transposed != 0: w is [Cin][Cout][3][3] and is read with mirrored taps -- the weight of the input-gradient convolution
 * of a 3x3 / stride-1 conv (Cout / Cin are those of the gradient conv: its outputs are the forward's inputs). */
int hdiff_pack_conv_weight_x3(const float* w, void* wp3, int Cout, int Cin, int CoutPad, int transposed,
                              hdiff_stream_t stream);
/* The same pack for any launch of the split-bf16 convolution kernel (taps within the 3x3 neighbourhood): tap t reads kernel
 * element (tap_ky[t], tap_kx[t]) of a KH x KW kernel stored [Cout][Cin][KH][KW] (mode 0) or [Cin][Cout][KH][KW] (mode 1,
 * nn.ConvTranspose2d) -- the four output-parity phases of ConvTranspose2d(5, stride 2) are packed this way (9 / 6 / 6 / 4 taps);
 * wp3 holds (Cin/16)*ntaps*3*CoutPad*8 32-bit words. */
int hdiff_pack_conv_weight_x3_taps(const float* w, void* wp3, int mode, int Cout, int Cin, int KH, int KW, int ntaps,
                                   const int* tap_ky, const int* tap_kx, int CoutPad, hdiff_stream_t stream);
/* (ABI 5) Weights of a standard 3x3 conv ([Cout][Cin][3][3], Cin % 16 == 0) as TWO fp16 pieces of w * 2^t, t chosen on the
 * device so that max |w| 2^t lies in [2^14, 2^15): [Cin/16][tap][piece][CoutPad][16] followed by a 4-word tail
 * {scratch, 2^-t, 2^t, 0}; hdiff_pack_conv_weight_h2_words gives the size in 32-bit words.  For the fp16-pair form of the
 * split-operand 3x3 kernel (hdiff_conv_desc.wp_h2; replaces the weight operand of F.conv2d at ModelCondition.py:172, 186). */
int hdiff_pack_conv_weight_h2_words(int Cout, int Cin, int CoutPad, int64_t* words_out);
int hdiff_pack_conv_weight_h2(const float* w, void* wp2, int Cout, int Cin, int CoutPad, hdiff_stream_t stream);
/* The fp16-pair pack for a tap LIST, the counterpart of hdiff_pack_conv_weight_x3_taps (same arguments, same tap rules):
 * [Cin/16][ntaps][2 pieces][CoutPad][16] of w * 2^t followed by the 4-word tail {scratch, 2^-t, 2^t, 0}.  t comes from the
 * maximum over the WHOLE tensor w, so the packs of the four phases of one transposed conv share it.  For
 * hdiff_conv_range.wp_h2_taps; the descriptor lists the taps in the order of the list given here. */
int hdiff_pack_conv_weight_h2_taps_words(int Cout, int Cin, int CoutPad, int ntaps, int64_t* words_out);
int hdiff_pack_conv_weight_h2_taps(const float* w, void* wp2, int mode, int Cout, int Cin, int KH, int KW, int ntaps,
                                   const int* tap_ky, const int* tap_kx, int CoutPad, hdiff_stream_t stream);
/* The fp16-pair pack of a 5x5 / stride-2 / pad-2 conv, made from its fp32 pack wp[25][CinPad][CoutPad] (hdiff_pack_conv_weight
 * with tap t = (t / 5, t % 5); DownSample's folded c2 + c1, exactly what the fp32 kernel multiplies by).  The conv runs as four
 * stride-1 convs over the parity planes of its input (taps with ky % 2 == oy, kx % 2 == ox read plane (oy, ox): 9 / 6 / 6 / 4
 * taps, all within the plane's 3x3 neighbourhood); the pack holds the four groups (0,0), (0,1), (1,0), (1,1) one after the
 * other, each [Cin/16][taps][2 pieces][CoutPad][16], and ONE tail {scratch, 2^-t, 2^t, 0}.  For hdiff_conv_range.wp_h2_s2. */
int hdiff_pack_conv_weight_h2_s2_words(int Cout, int Cin, int CoutPad, int64_t* words_out);
int hdiff_pack_conv_weight_h2_s2(const float* wp, void* wp2, int Cout, int Cin, int CinPad, int CoutPad, hdiff_stream_t stream);
/* (ABI 5) Range of a GroupNorm + Swish output from the GroupNorm weights alone: |swish(gamma * xhat + beta)| <=
 * sqrt(n - 1) * max |gamma| + max |beta| =: A for groups of n = group_elems elements (a normalised value cannot leave
 * [-sqrt(n - 1), sqrt(n - 1)]).  out2[0] = 2^s, out2[1] = 2^-s with gain * A * 2^s in [2^13, 2^14): the power of two by which
 * the fp16-pair conv stages its activations (hdiff_conv_desc.act_scale); gain = 1, or 1 / keep when a dropout scaled by
 * 1 / keep sits between the activation and the conv (ModelCondition.py:185) -- applied inside the prologue by
 * hdiff_conv2d_fwd_dropout, or by the caller on a materialised tensor.  nn.GroupNorm at ModelCondition.py:169, 182. */
int hdiff_gn_act_scale(const float* gamma, const float* beta, int C, int64_t group_elems, float gain, float* out2,
                       hdiff_stream_t stream);

typedef struct hdiff_conv_desc {
  /* input: virtual channel-concat of x0 [B][C0][H][W] and x1 [B][C1][H][W] (x1 may be NULL with C1 = 0);
   * replaces torch.cat([h, hs.pop()], dim=1) at ModelCondition.py:271 */
  const float* x0;
  const float* x1;
  int C0, C1;
  int B, H, W;
  /* packed weights and optional bias [Cout] */
  const float* wp;
  const float* bias;
  int Cout, CinPad, CoutPad;
  /* optional fused prologue: y = swish(x * gn_scale[b][c] + gn_shift[b][c])  (GroupNorm affine + Swish folded to a
   * per-(sample,channel) scale/shift by hdiff_gn_finalize; zero padding is applied AFTER the activation) */
  const float* gn_scale;
  const float* gn_shift;
  /* optional fused epilogue: + addvec[b][co] (temb/cemb projections, ModelCondition.py:198-200), + residual (h + shortcut(x), :202) */
  const float* addvec;
  const float* residual;
  float* out;      /* [B][Cout][OH][OW] */
  int OH, OW;
  /* geometry: the kernel iterates a virtual output grid VH x VW; input coord = v*in_stride + tap_d; output coord = v*out_s + out_o */
  int VH, VW;
  int in_stride;
  int out_sy, out_oy, out_sx, out_ox;
  int ntaps;
  int tap_dy[HDIFF_MAX_TAPS];
  int tap_dx[HDIFF_MAX_TAPS];
  /* optional split-K workspace (hdiff_conv2d_fwd_workspace floats): small grids with long channel loops are cut into
   * channel slices whose partial sums are reduced in a fixed order; NULL = never split */
  float* splitk_ws;
  int64_t splitk_floats;
  /* optional (ABI 2): the same weights as three bf16 pieces (hdiff_pack_conv_weight_x3).  Used instead of wp when the
   * contraction mode is HDIFF_CONTRACT_BF16X3 and the launch is a stride-1 conv with Cin % 16 == 0 whose taps lie in the 3x3
   * neighbourhood (the plain 3x3 / pad-1 conv; a transposed-conv phase with its (2, py, 2, px) output map), or (ABI 5) a
   * full-resolution 1x1 / stride-1 conv with a ONE-tap pack from hdiff_pack_conv_weight_x3_taps (Cin % 16 == 0, H * W % 256 == 0);
   * NULL = always the fp32-input MFMA.  Tap order: hdiff_pack_conv_weight_x3 stores tap t = (t / 3, t % 3), so a plain 3x3
   * launch must list tap_dy[t] = t / 3 - 1, tap_dx[t] = t % 3 - 1 (any other order of the nine taps, and any list with a
   * repeated tap or one that does not fill the 3x3, 3x2, 2x3 or 2x2 rectangle it spans, runs the fp32 kernel on wp instead); a pack made by hdiff_pack_conv_weight_x3_taps holds the taps in
   * the order of the list it was given, and the descriptor has to list them in that same order. */
  const void* wp_x3;
  /* optional (ABI 5): the fp16-pair form of the same kernel for the plain 3x3 / pad-1 conv WITH the GroupNorm + Swish prologue
   * (three fp16 piece products instead of six bf16 ones).  wp_h2 = hdiff_pack_conv_weight_h2 of the same weights, act_scale =
   * the two floats of hdiff_gn_act_scale for the GroupNorm whose statistics gn_scale / gn_shift carry.  Preferred over wp_x3
   * when both are set, the mode is HDIFF_CONTRACT_BF16X3 and the launch qualifies; either may be NULL.  act_scale is the
   * caller's statement that every staged activation (after the prologue, if any) is below 2^15 / act_scale[0] in magnitude:
   * with gn_scale / gn_shift that are not GroupNorm statistics of x0 / x1 a value can exceed it, the fp16 conversion then gives
   * inf and the output NaN (never silently wrong). */
  const void* wp_h2;
  const float* act_scale;
} hdiff_conv_desc;

int hdiff_conv2d_fwd_workspace(const hdiff_conv_desc* d, int64_t* floats_out);
int hdiff_conv2d_fwd(const hdiff_conv_desc* d, hdiff_stream_t stream);
/* conv(dropout(swish(GroupNorm(x)))) as ONE launch: nn.Dropout in train mode between Swish and block2's conv
 * (ModelCondition.py:184-186).  The staged activation is kept ? swish(x * gn_scale + gn_shift) * inv_keep : 0, where the keep
 * decision of the element with flat NCHW index e of x0 is bit (e & 31) of keep_bits[e >> 5] (hdiff_dropout_keep_bits) and
 * inv_keep is the fp32 1 / keep.  Served by every kernel hdiff_conv2d_fwd dispatches such a conv to (both contraction modes,
 * split-K included; same workspace query).  The descriptor must be a plain 3x3 / stride-1 / pad-1 conv (nine taps in row-major
 * order, output grid = input grid) WITH gn_scale / gn_shift, without x1, C0 % 8 == 0, fewer than 2^31 input elements;
 * act_scale, when set, must have been computed with gain = 1 / keep.  Anything else is HDIFF_ERR_INVALID, nothing is launched.
 * Padding positions stage 0 and use no keep bit; no word outside the ceil(B*C0*H*W / 32) words is read. */
int hdiff_conv2d_fwd_dropout(const hdiff_conv_desc* d, const uint32_t* keep_bits, float inv_keep, hdiff_stream_t stream);

/* Per-sample range words: how a convolution WITHOUT the GroupNorm prologue gets onto the fp16-pair form of the split-operand
 * kernel.  The kernel that produces a tensor leaves max |out[b]| of every sample b in a 32-bit word (its epilogue: no pass over
 * memory), the kernel that consumes the tensor forms its staging scale 2^s from that word.
 *   absmax_out  uint32_t[B] or NULL.  After the call word b holds max(word b before, bits of max |out[b, :, :, :]| over what this
 *               call wrote for sample b) -- an unsigned maximum of fp32 bit patterns, so NaN and inf end up in the word and the
 *               result does not depend on order.  The caller zeroes the words before the first producer of a tensor (the four
 *               phases of a transposed conv all max into the same words).  Filled on every path of the split-operand mode:
 *               in the epilogue of the split-operand kernels, by one small extra launch behind the others.
 *   absmax_in   uint32_t[B] or NULL: word b = bits of (a bound of) max |x[b]| of the input as stored.  With it, a launch that
 *               qualifies for the split-operand 3x3 kernel runs its fp16-pair form: weights from hdiff_conv_desc.wp_h2 (the
 *               plain 3x3 conv) or from wp_h2_taps below (a tap list: the transposed-conv phases), activations staged times 2^s
 *               with absmax 2^s in [2^14, 2^15).  A zero, denormal or non-finite word gives a fixed finite scale.  A word below
 *               the true maximum overflows the fp16 conversion: that sample's output is NaN, never a finite wrong value.
 *               Not allowed together with gn_scale / gn_shift (the word describes x, not the prologue's output).
 *   wp_h2_taps  hdiff_pack_conv_weight_h2_taps of the descriptor's tap list, or NULL; needs absmax_in.
 *   wp_h2_s2    hdiff_pack_conv_weight_h2_s2 of the descriptor's wp, or NULL; needs absmax_in, ntaps = 25 and in_stride = 2.
 *               With it the 5x5 / stride-2 / pad-2 conv (taps in row-major order, no prologue, no residual, Cin % 16 == 0, a
 *               launch large enough to fill the chip) runs as four parity-plane pair convolutions inside this one call: each
 *               adds to what the ones before left in out, the LAST carries bias / addvec (one rounding at the size of the
 *               result).  Any other descriptor keeps the fp32 kernel.
 * Sample b of the output depends on word b alone.  Outside the split-operand modes (HDIFF_CONTRACT_BF16X3 and
 * HDIFF_CONTRACT_F16), that is in HDIFF_CONTRACT_F32, the call IS hdiff_conv2d_fwd(d): the struct is ignored, the words are
 * neither read nor written.  Same workspace query. */
typedef struct hdiff_conv_range {
  uint32_t* absmax_out;
  const uint32_t* absmax_in;
  const void* wp_h2_taps;
  const void* wp_h2_s2;
} hdiff_conv_range;
int hdiff_conv2d_fwd_range(const hdiff_conv_desc* d, const hdiff_conv_range* r, hdiff_stream_t stream);
/* Zeroes n range words (one tiny launch: captured into a graph, every replay starts from zeros). */
int hdiff_range_words_zero(uint32_t* words, int n, hdiff_stream_t stream);

/* Which kernel the three forward entries run a descriptor on, in the contraction mode of the moment.  Host only: nothing is
 * launched, no device is needed, no pointer of the descriptor is dereferenced.  r may be NULL (hdiff_conv2d_fwd); dropout != 0
 * asks for hdiff_conv2d_fwd_dropout (then r must be NULL).  The validation of the entry asked for applies, with its messages.
 * *absmax_tail_out = 1 when the small conv_out_absmax_kernel launch follows the conv (r->absmax_out set in a split-operand mode
 * on a route whose epilogue does not fill the words: IGEMM and DIRECT_1X1), else 0. */
enum {
  HDIFF_CONV_ROUTE_IGEMM = 0,         /* conv_igemm_kernel on wp (fp32-input MFMA), split-K when the workspace query asked for it */
  HDIFF_CONV_ROUTE_DIRECT_1X1 = 1,    /* conv1x1_direct_kernel on wp */
  HDIFF_CONV_ROUTE_X3_1X1 = 2,        /* conv1x1_x3_kernel on the one-tap wp_x3 (bf16 triples) */
  HDIFF_CONV_ROUTE_X3_TRIPLES = 3,    /* conv3x3_x3_kernel on wp_x3 (bf16 triples) */
  HDIFF_CONV_ROUTE_X3_PAIRS_GN = 4,   /* conv3x3_x3_kernel on wp_h2 (fp16 pairs), staging scale from act_scale */
  HDIFF_CONV_ROUTE_X3_PAIRS_WORD = 5, /* conv3x3_x3_kernel on wp_h2 or r->wp_h2_taps (fp16 pairs), staging scale from r->absmax_in */
  HDIFF_CONV_ROUTE_S2_PAIRS_WORD = 6  /* four parity-plane launches of conv3x3_x3_kernel on r->wp_h2_s2, scale from r->absmax_in */
};
int hdiff_conv2d_fwd_route(const hdiff_conv_desc* d, const hdiff_conv_range* r, int dropout, int* route_out, int* absmax_tail_out);

/* Weight gradient of hdiff_conv2d_fwd (autograd of the conv weights, TrainCondition.py:60).  Same geometry fields as the
 * forward descriptor; dy is the gradient of the forward's `out`.  The kernel writes `nsplit` packed partial slabs
 * dwp[nsplit][ntaps][CinPad][CoutPad] (size from hdiff_conv2d_wgrad_workspace); hdiff_conv_wgrad_unpack sums them in a
 * fixed order into the PyTorch layout (mode / taps as in hdiff_pack_conv_weight; tap_ky < 0 skips a tap). */
typedef struct hdiff_conv_wgrad_desc {
  const float* x0;
  const float* x1;
  int C0, C1;
  int B, H, W;
  const float* gn_scale;
  const float* gn_shift;
  const float* dy;      /* [B][Cout][OH][OW] */
  int Cout, CinPad, CoutPad;
  int OH, OW;
  int VH, VW;
  int in_stride;
  int out_sy, out_oy, out_sx, out_ox;
  int ntaps;
  int tap_dy[HDIFF_MAX_TAPS];
  int tap_dx[HDIFF_MAX_TAPS];
} hdiff_conv_wgrad_desc;
int hdiff_conv2d_wgrad_workspace(const hdiff_conv_wgrad_desc* d, int* nsplit_out, int64_t* floats_out);
int hdiff_conv2d_wgrad(const hdiff_conv_wgrad_desc* d, float* dwp, int nsplit, hdiff_stream_t stream);
/* Weight gradient of hdiff_conv2d_fwd_dropout: the activation recomputed from x0 is masked and scaled like the forward's
 * (same descriptor rules, same keep_bits / inv_keep).  Workspace and nsplit from hdiff_conv2d_wgrad_workspace; same slabs and
 * the same ordered reduce (hdiff_conv_wgrad_unpack): no atomics, bitwise repeatable. */
int hdiff_conv2d_wgrad_dropout(const hdiff_conv_wgrad_desc* d, const uint32_t* keep_bits, float inv_keep, float* dwp, int nsplit,
                               hdiff_stream_t stream);
/* Which kernel hdiff_conv2d_wgrad (dropout != 0: hdiff_conv2d_wgrad_dropout) runs a descriptor on.  Host only: nothing is
 * launched, no device is needed, no pointer of the descriptor is dereferenced.  The validation of the entry asked for applies,
 * with its messages, and for the generic kernel the check that its tile fits.  hdiff_conv2d_wgrad_workspace reads the same
 * answer: the fast kernels have their own split counts.  The generic kernel's tile is 2^t columns x 128 / 2^t rows of the
 * virtual output grid, 2^t = VW rounded up to a power of two, 32 at most; at 32 columns each of the four waves owns one tile row
 * (ROWS1 / ROWS2, by in_stride) -- on planes at least as tall as the tile, VH >= 4, only. */
enum {
  HDIFF_WGRAD_ROUTE_FAST_1X1 = 0,       /* conv_wgrad1x1_kernel: plain 1x1 without prologue, H * W and the channel counts aligned */
  HDIFF_WGRAD_ROUTE_FAST_3X3 = 1,       /* conv_wgrad3x3_kernel: plain 3x3 / stride 1, W % 32 == 0, H even, channel counts aligned */
  HDIFF_WGRAD_ROUTE_GENERIC = 2,        /* conv_wgrad_kernel<0>: any tap list, stride and output map; tiles narrower than 32 or taller than the plane */
  HDIFF_WGRAD_ROUTE_GENERIC_ROWS1 = 3,  /* conv_wgrad_kernel<1>: 4 x 32 tile, in_stride 1 */
  HDIFF_WGRAD_ROUTE_GENERIC_ROWS2 = 4   /* conv_wgrad_kernel<2>: 4 x 32 tile, in_stride 2 */
};
int hdiff_conv2d_wgrad_route(const hdiff_conv_wgrad_desc* d, int dropout, int* route_out);
int hdiff_conv_wgrad_unpack(const float* dwp, int nsplit, float* dw, int mode, int Cout, int Cin, int KH, int KW, int ntaps,
                            const int* tap_ky, const int* tap_kx, int CinPad, int CoutPad, int accumulate,
                            hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * GroupNorm statistics (K5).  Replaces nn.GroupNorm(32, C) at ModelCondition.py:170,184,249 (the normalisation itself
 * and the Swish at :22-24 are applied inside the consuming convolution's prologue).
 *   hdiff_gn_stats:    partial (count, mean, M2) per (sample, group, split) over the virtual concat input
 *   hdiff_gn_finalize: combines the partials (Chan) and writes scale[b][c] = rstd*gamma[c], shift[b][c] = beta[c]-mean*scale
 * ws must hold B*G*nsplit*3 floats.  A split covers at least 4096 elements of a plane; with more splits than that
 * allows the rest are empty (count 0) and the merge skips them.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_gn_stats(const float* x0, const float* x1, int C0, int C1, int B, int HW, int G, int nsplit, float* ws,
                   hdiff_stream_t stream);
int hdiff_gn_finalize(const float* ws, int B, int C, int G, int nsplit, const float* gamma, const float* beta, float eps,
                      float* scale, float* shift, float* mean_out /*[B][G] or NULL*/, float* rstd_out /*[B][G] or NULL*/,
                      hdiff_stream_t stream);
/* hdiff_gn_stats + hdiff_gn_finalize behind one entry point.  nsplit == 1 (planes up to 64x64: every (sample, group) is
 * one workgroup) -> ONE launch, the workgroup folds its own statistics into scale / shift; nsplit > 1 -> the streaming
 * pass and the small merge kernel, as two launches of the same call.  Results are bit-identical to the two-call form. */
int hdiff_gn_scale_shift(const float* x0, const float* x1, int C0, int C1, int B, int HW, int G, int nsplit, float* ws,
                         const float* gamma, const float* beta, float eps, float* scale, float* shift,
                         hdiff_stream_t stream);
/* Backward of GroupNorm + Swish (the conv prologue): dA is the gradient w.r.t. the activated tensor [B][C0+C1][HW];
 * mean/rstd [B][G] come from hdiff_gn_finalize.  Writes dx0 [B][C0][HW], dx1 [B][C1][HW], dgamma [C], dbeta [C].
 * ws: 2*B*C + 2*B*G floats. */
int hdiff_gn_swish_bwd(const float* x0, const float* x1, int C0, int C1, int B, int HW, int G, const float* dA,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, float* ws, float* dx0,
                       float* dx1, float* dgamma, float* dbeta, hdiff_stream_t stream);
/* hdiff_gn_swish_bwd behind a dropout (the backward of hdiff_conv2d_fwd_dropout's prologue): dA [B][C][HW] is the gradient
 * w.r.t. the DROPPED activation and is read as kept ? dA * inv_keep : 0 in both passes that use it; x is one tensor.
 * ws: 2*B*C + 2*B*G floats. */
int hdiff_gn_swish_dropout_bwd(const float* x, int C, int B, int HW, int G, const float* dA, const uint32_t* keep_bits,
                               float inv_keep, const float* mean, const float* rstd, const float* gamma, const float* beta,
                               float* ws, float* dx, float* dgamma, float* dbeta, hdiff_stream_t stream);
/* The same for GroupNorm WITHOUT Swish (AttnBlock's pre-norm, ModelCondition.py:103): dY is the gradient w.r.t. the
 * normalised tensor [B][C][HW].  ws: 2*B*C + 2*B*G floats. */
int hdiff_gn_affine_bwd(const float* x, int C, int B, int HW, int G, const float* dY, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, float* ws, float* dx, float* dgamma, float* dbeta,
                        hdiff_stream_t stream);
/* dvec[b][c] = sum_hw dy[b][c][:] (gradient of the per-sample channel vector) and dbias[c] = sum_b dvec[b][c]; either may be NULL */
int hdiff_bias_addvec_grad(const float* dy, int B, int C, int HW, float* dvec, float* dbias, hdiff_stream_t stream);
/* y = x*scale[b][c] + shift[b][c]: GroupNorm without Swish (AttnBlock, ModelCondition.py:103) */
int hdiff_gn_affine_apply(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW,
                          hdiff_stream_t stream);
/* Stand-alone y = swish(x*scale+shift) (a plain Swish with scale 1 / shift 0 in the embedding MLPs; tests build references from it). */
int hdiff_gn_swish_apply(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW,
                         hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-head self-attention core (K9).  Replaces the softmax(QK^T/sqrt(d))V of nn.MultiheadAttention(C, 8) called as
 * attn(h,h,h) at ModelCondition.py:189,204-208.  qkv is the output of the packed in-projection viewed as a 1x1 conv:
 * [B][3C][L] with rows [Q | K | V], head h owning rows h*d..h*d+d-1 of each third.  o is [B][C][L].
 * Flash style: the L x L score matrix is never materialised.  d = C/heads must be one of 4, 8, 12, 16, 24, 32, 48, 64 (48 / 64: slower one-tile-per-wave kernels; not shapes of the default model).
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_mha_flash_fwd(const float* qkv, float* o, float* lse2 /*[B][heads][L] or NULL*/, int B, int C, int heads, int L,
                        hdiff_stream_t stream);
/* The same call with a caller-provided scratch buffer.  In the bf16x3 contraction mode (hdiff_set_contraction_mode) the
 * operands are then split ONCE into three bf16 pieces each (a streaming pass into `ws`) and the attention kernel runs on the
 * pre-split tensors (attention_x3p.hip); without a workspace -- or for a shape the pre-split kernel does not cover, for
 * which the query returns 0 bytes -- the kernels split inside their loop.  In the fp32 mode `ws` is not touched.  The size
 * is a function of the shape only (B * 3C * L * 6 bytes when covered: d_head 16 / 32, L a multiple of 256, L >= 512). */
int hdiff_mha_flash_fwd_workspace(int B, int C, int heads, int L, int64_t* bytes_out);
int hdiff_mha_flash_fwd_ws(const float* qkv, float* o, float* lse2 /*[B][heads][L] or NULL*/, int B, int C, int heads, int L,
                           void* ws, int64_t ws_bytes, hdiff_stream_t stream);
/* Which program the two forward entries run a call on, in the contraction mode of the moment (hdiff_mha_flash_fwd: ws_bytes = 0).
 * Host only: nothing is launched, no device is needed.  The validation of the launching entries applies, with their messages; a
 * refused call writes nothing.  *nq_out: query tiles of 16 per wave of mha_flash_fwd_kernel wherever it runs, as main kernel or
 * as check pass (1 or 4); *check_out = 1: it follows the route's kernel in check mode and redoes the query blocks that kernel
 * flagged (the HDIFF_NO_CHECK_PASS developer knob suppresses that launch, not this answer). */
enum {
  HDIFF_MHA_FWD_ROUTE_RUNNING_MAX = 0, /* mha_flash_fwd_kernel<D, nq> alone (check = 0) */
  HDIFF_MHA_FWD_ROUTE_FAST_F32 = 1,    /* mha_flash_fwd_fast_kernel<D, 4>, then the check pass */
  HDIFF_MHA_FWD_ROUTE_X3_TRIPLES = 2,  /* mha_flash_fwd_x3_kernel (splits in its loop), then the check pass */
  HDIFF_MHA_FWD_ROUTE_H2_PAIRS = 3,    /* d_head 16 on the pre-split workspace, 256 queries per workgroup, then the check pass */
  HDIFF_MHA_FWD_ROUTE_X3P_PAIRS = 4,   /* d_head 32 on the pre-split workspace, then the check pass */
  HDIFF_MHA_FWD_ROUTE_F16_SINGLE = 5,  /* f16 mode, no log-sum-exp, single fp16 pieces, then the check pass */
  HDIFF_MHA_FWD_ROUTE_H2_PAIRS_Q384    /* (6) H2_PAIRS with 384 queries per workgroup, where rounds x queries says it is cheaper: same bits */
};
int hdiff_mha_flash_fwd_route(int B, int C, int heads, int L, int want_lse, int64_t ws_bytes, int* route_out, int* nq_out,
                              int* check_out);
/* hdiff_mha_flash_fwd_ws on a named route (tests, A/B timing): `route` is the one hdiff_mha_flash_fwd_route answers for the call, or
 * the other of H2_PAIRS / H2_PAIRS_Q384 where it answers one of these two; every other value is refused. */
int hdiff_mha_flash_fwd_ws_as(const float* qkv, float* o, float* lse2 /*[B][heads][L] or NULL*/, int B, int C, int heads, int L,
                              void* ws, int64_t ws_bytes, int route, hdiff_stream_t stream);
/* Single-head attention with a head wider than 64 channels: softmax(q k^T * C^-1/2) v with d_head = C, the core of the
 * reference's AttnBlock (ModelCondition.py:109-116; dead code there, built for completeness: one workgroup per query row,
 * L + C floats of LDS).  qkv [B][3C][L] rows [q | k | v], o [B][C][L].  Heads of width <= 64: hdiff_mha_flash_fwd, heads = 1. */
int hdiff_mha_wide_fwd(const float* qkv, float* o, int B, int C, int L, hdiff_stream_t stream);
/* Backward of the single-head core of any width (autograd through AttnBlock.forward, ModelCondition.py:109-116): dqkv
 * [B][3C][L] from dO [B][C][L]; probabilities are recomputed.  ws: 2*B*L floats (log-sum-exp and delta per query). */
int hdiff_mha_wide_bwd(const float* qkv, const float* d_o, float* dqkv, float* ws, int B, int C, int L, hdiff_stream_t stream);
/* Backward of the core (autograd of nn.MultiheadAttention, TrainCondition.py:60): dqkv [B][3C][L] from dO [B][C][L].
 * lse2 is the forward's log2-domain log-sum-exp; delta is a [B][heads][L] workspace (rowsum(dO o O), written here).
 * P is recomputed, never stored; five MFMA products per tile in ONE kernel: a workgroup owns a key range (dK, dV in
 * registers) and adds its dQ tiles to the partial slab of that range in ws, summed in range order afterwards -- every slab
 * word is only ever touched by one thread, in program order: bitwise reproducible.  In the bf16x3 contraction mode at
 * d_head 16 or 32 (L a multiple of 256, >= 512) the five products run on the bf16 matrix core (attention_bwd_x3.hip); ws then
 * also holds the five bf16 piece tensors of Q, K, K^T, V, dO (30 bytes per element of a [B][C][L] tensor) and the slab
 * words after a range's first key block are accumulated by in-order L2 float adds.  hdiff_mha_flash_bwd_workspace gives
 * the size of ws in floats: a function of the shape only, large enough for either contraction mode (0: ws may be NULL). */
int hdiff_mha_flash_bwd_workspace(int B, int C, int heads, int L, int64_t* n_floats);
int hdiff_mha_flash_bwd(const float* qkv, const float* o, const float* d_o, const float* lse2, float* delta, float* dqkv,
                        float* ws, int B, int C, int heads, int L, hdiff_stream_t stream);
/* Which kernels hdiff_mha_flash_bwd runs a call on, in the contraction mode of the moment.  Host only, validated like that entry;
 * a refused call writes nothing.  *nk_out: key tiles of 16 per wave (1, 2 or 4; 0 on H2_PAIRS); *aligned_out = 0: the
 * bounds-checked <D, 1, false> kernel; *nsplit_out: key ranges per (sample, head) pair (HDIFF_BWD_SLAB_GIB bounds it on H2_PAIRS).
 * Not modelled: a device that refuses the H2_PAIRS kernels' 70 KB of LDS (no MI355X does) runs FUSED_F32 on the answer the
 * fp32 mode gets. */
enum {
  HDIFF_MHA_BWD_ROUTE_FUSED_F32 = 0,   /* mha_bwd_fused_kernel<D, nk, aligned> (+ mha_dq_reduce_kernel when nsplit > 1) */
  HDIFF_MHA_BWD_ROUTE_H2_PAIRS = 1     /* absmax + split + mha_bwd_h2p_kernel (d 16) / mha_bwd_h2_kernel<32> (d 32) + its reduce */
};
int hdiff_mha_flash_bwd_route(int B, int C, int heads, int L, int* route_out, int* nk_out, int* aligned_out, int* nsplit_out);

/* ------------------------------------------------------------------------------------------------------------------
 * Small dense layers (K6, K10).  y[b][j] (+)= bias[j] + sum_k W[j][k] * f(x_row(b)[k]),  f = identity or Swish.
 * If idx != NULL the input row is x[idx[b]] (nn.Embedding gather, ModelCondition.py:38,56) with idx clamped to
 * [0, n_rows) so a bad index can never fault the GPU (the host layer raises IndexError like nn.Embedding); otherwise x[b].
 * Replaces nn.Linear / nn.Embedding at ModelCondition.py:38-43, 56-61, 174-181.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_linear_rows(const float* x, const int64_t* idx, int n_rows, const float* W, const float* bias, float* y, int B,
                      int K, int N, int swish_input, int accumulate, hdiff_stream_t stream);
/* Every per-block projection of the time and label embeddings in one launch (ResBlock.forward, ModelCondition.py:199-200):
 *   y_j[b][n] = (sum_k swish(x0[b][k]) w0_j[n][k] + b0_j[n]) + (sum_k swish(x1[b][k]) w1_j[n][k] + b1_j[n]),  j < njobs
 * bit-identical to hdiff_linear_rows(x0 -> y_j, swish) followed by hdiff_linear_rows(x1 -> y_j, swish, accumulate).
 * `jobs` lives in DEVICE memory (pointers to [n][K] weights, [n] biases, the [B][n] output); jobs[j].first = sum of the n
 * of the jobs before j; total_n = sum of all n; w1 / b1 may be NULL (no second term). */
typedef struct hdiff_linear_job {
  const float* w0; const float* b0; const float* w1; const float* b1; float* y;
  int n; int first;
} hdiff_linear_job;
int hdiff_linear_rows_multi(const float* x0 /*[B][K]*/, const float* x1 /*[B][K] or NULL*/, const hdiff_linear_job* jobs,
                            int njobs, int total_n, int B, int K, hdiff_stream_t stream);

/* Backward of hdiff_linear_rows: dW [N][K] (+)= dy^T f(x), db [N] (+)= sum_b dy, and, if dx != NULL, dx = (dy W) o f'(x).
 * With idx != NULL, dx is the [n_rows][K] gradient of the gathered table and is ACCUMULATED into (zero it first); row
 * pad_row (>= 0) gets no gradient (nn.Embedding(padding_idx=0), ModelCondition.py:57). */
int hdiff_linear_rows_bwd(const float* x, const int64_t* idx, int n_rows, const float* W, const float* dy, float* dx,
                          float* dW, float* db, int B, int K, int N, int swish_input, int accumulate, int pad_row,
                          hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Diffusion process (K11-K13), DiffusionFreeGuidence/DiffusionCondition.py.
 * ------------------------------------------------------------------------------------------------------------------ */
/* q_sample (:43-44): x_t = sa[t[b]]*x0 + sb[t[b]]*noise ; sa/sb are the fp32 casts of the float64 schedule buffers, T their
 * length: t[b] is clamped to [0, T) in the kernel (a bad index never faults the GPU; the host raises like extract's gather). */
int hdiff_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                   float* xt, int B, int per_sample, int T, hdiff_stream_t stream);
/* unreduced squared error (:45): loss = (eps_hat - noise)^2 */
int hdiff_sq_err(const float* a, const float* b, float* out, int64_t n, hdiff_stream_t stream);
/* its backward: da = 2*(a-b)*dloss */
int hdiff_sq_err_bwd(const float* a, const float* b, const float* dloss, float* da, int64_t n, hdiff_stream_t stream);
/* One ancestral step (:74-80, :89-96):
 *   eps = (1+w)*eps_c - w*eps_u  (w is the Python float of the reference; (1+w) is formed in double, then cast) ; mean = coeff1[t]*x - coeff2[t]*eps ; x_next = mean + sigma[t]*z  (z = 0 when t == 0)
 * step_ptr points at the device-resident current time step (int32) so the launch is hipGraph-replayable; when
 * noise == NULL z is drawn in-kernel (Philox4x32-10 + Box-Muller, counter = (seed, step, element)).  nan_flag (int32)
 * is OR-ed with 1 if any output is NaN (the reference's per-step assert, :96, evaluated once after the loop). */
int hdiff_ddpm_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, float* x_next,
                    const float* coeff1, const float* coeff2, const float* sigma, const int32_t* step_ptr,
                    int T /* length of the three tables: the step read from step_ptr is clamped into [0, T) */, double w,
                    uint64_t seed, int32_t* nan_flag, int64_t n, hdiff_stream_t stream);
/* The same update with the loop's bookkeeping folded in, so that one captured denoising step is the UNet launches plus
 * this ONE kernel (DiffusionCondition.py:87-96).  After the update the workgroup that finishes last
 *   - writes the next time step, *step_ptr - 1, to *step_ptr and (clamped at 0) to t_next[0 .. t_count): the time vector
 *     `t = x_t.new_ones([B]) * time_step` (:89) of the next replay;
 * and every workgroup also stores x_next to x_dup0 / x_dup1 when they are given (the two halves of the 2B-batched
 * cond + uncond UNet input of the next step, :76-77).  done_counter: one uint32 in device memory, zero before the first
 * launch; it counts finished workgroups and wraps back to zero by itself (no reset between replays). */
typedef struct hdiff_ddpm_loop_desc {
  const float* x; const float* eps_c; const float* eps_u;
  const float* noise;                 /* NULL: in-kernel Philox noise */
  float* x_next;
  const float* coeff1; const float* coeff2; const float* sigma;   /* [T] fp32 */
  int32_t* step_ptr;
  int T;
  double w;
  uint64_t seed;
  int32_t* nan_flag;
  int64_t n;
  float* x_dup0; float* x_dup1;       /* optional */
  int64_t* t_next; int t_count;       /* optional (t_count = 0) */
  uint32_t* done_counter;
} hdiff_ddpm_loop_desc;
int hdiff_ddpm_step_loop(const hdiff_ddpm_loop_desc* d, hdiff_stream_t stream);
/* One STRIDED DDIM step with classifier-free guidance for the same sampler (no call site in the reference, whose label-conditioned
 * tree only has the T-step ancestral loop; Song et al. 2021, eq. 12 on a sub-sequence tau_0 < ... < tau_(S-1) of the time steps).
 * k = *step_ptr (int32, device resident, clamped into [0, nsteps)) is the POSITION in tau; tab[k] = {sqrt(1 - a), sqrt(a),
 * sqrt(a'), sqrt(max(1 - a' - sigma^2, 0)), sigma} in fp32 with a = alphas_bar[tau_k], a' = alphas_bar[tau_(k-1)] (1 at k = 0):
 *   eps = (1+w)*eps_c - w*eps_u ; x0 = (x - eps*tab[k][0]) / tab[k][1]
 *   clip_x0 != 0:  x0 = clamp(x0, -1, 1) (a NaN stays a NaN) ; eps = (x - tab[k][1]*x0) / tab[k][0]
 *   x_next = tab[k][2]*x0 + tab[k][3]*eps  (+ tab[k][4]*z  when k > 0 and tab[k][4] > 0)
 * each written operation rounded once, w cast as in hdiff_ddpm_step.  z: noise[i], or with noise == NULL the in-kernel Philox
 * stream of hdiff_ddpm_step with counter (seed, k, element).  nan_flag is OR-ed with 1 on a NaN output.  x and x_next may alias. */
int hdiff_cfg_ddim_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, float* x_next,
                        const float* tab /* [nsteps][5] */, const int32_t* step_ptr, int nsteps, double w, int clip_x0,
                        uint64_t seed, int32_t* nan_flag, int64_t n, hdiff_stream_t stream);
/* The same update with the loop's bookkeeping folded in, as hdiff_ddpm_step_loop does for the ancestral step: ONE launch per step.
 * Every workgroup also stores x_next to x_dup0 / x_dup1 when given; the workgroup that finishes last writes *step_ptr - 1 to
 * *step_ptr and t_tab[max(*step_ptr - 1, 0)] (t_tab[k] = tau_k, int64) to t_next[0 .. t_count).  done_counter: one uint32, zero
 * before the first launch; it wraps back to zero by itself. */
typedef struct hdiff_cfg_ddim_loop_desc {
  const float* x; const float* eps_c; const float* eps_u;
  const float* noise;                 /* NULL: in-kernel Philox noise */
  float* x_next;
  const float* tab;                   /* [nsteps][5] fp32 */
  const int64_t* t_tab;               /* [nsteps]; may be NULL when t_count = 0 */
  int32_t* step_ptr;
  int nsteps;
  int clip_x0;
  double w;
  uint64_t seed;
  int32_t* nan_flag;
  int64_t n;
  float* x_dup0; float* x_dup1;       /* optional */
  int64_t* t_next; int t_count;       /* optional (t_count = 0) */
  uint32_t* done_counter;
} hdiff_cfg_ddim_loop_desc;
int hdiff_cfg_ddim_step_loop(const hdiff_cfg_ddim_loop_desc* d, hdiff_stream_t stream);
/* One DPM-Solver++(2M) step (Lu et al. 2022, data-prediction form, multistep) with classifier-free guidance for the same sampler:
 * one model evaluation per step like DDIM, second order through one history tensor.  k = *step_ptr (clamped into [0, nsteps)) is
 * the POSITION in tau; tab[k] = {s1m, sa, A, B, C} in fp32 (DiffusionCondition.py: dpmpp_table -- s1m = sqrt(1 - a), sa = sqrt(a),
 * A = sqrt(1 - a') / sqrt(1 - a), B and C the data-prediction weights of x0 and of the previous x0; C = 0 on first-order rows):
 *   eps = (1+w)*eps_c - w*eps_u ; x0 = (x - eps*tab[k][0]) / tab[k][1]
 *   clip_x0 != 0:  x0 = clamp(x0, -1, 1) (a NaN stays a NaN)
 *   v = tab[k][2]*x + tab[k][3]*x0 ; tab[k][4] != 0:  v = v + tab[k][4]*x0_prev ; x0_prev = x0 ; x_next = v
 * each written operation rounded once, w cast as in hdiff_ddpm_step.  x0_prev [n] is the caller's persistent history: it is NOT
 * read when tab[k][4] == 0 (the first step of a loop, where it holds whatever the last call left, and the closing one) and always
 * written.  Deterministic: no noise, no seed.  nan_flag is OR-ed with 1 on a NaN output.  x and x_next may alias.  Buffers that are
 * all 16-byte aligned are accessed four floats at a time, with the same result. */
int hdiff_cfg_dpmpp_step(const float* x, const float* eps_c, const float* eps_u, float* x_next, float* x0_prev,
                         const float* tab /* [nsteps][5] */, const int32_t* step_ptr, int nsteps, double w, int clip_x0,
                         int32_t* nan_flag, int64_t n, hdiff_stream_t stream);
/* The same update with hdiff_cfg_ddim_step_loop's bookkeeping folded in (x_dup0 / x_dup1, the last workgroup's decrement of
 * *step_ptr, t_tab[max(*step_ptr - 1, 0)] to t_next, the self-wrapping done_counter): ONE launch per step. */
typedef struct hdiff_cfg_dpmpp_loop_desc {
  const float* x; const float* eps_c; const float* eps_u;
  float* x_next;
  float* x0_prev;                     /* [n] fp32 history, read only when tab[k][4] != 0 */
  const float* tab;                   /* [nsteps][5] fp32 */
  const int64_t* t_tab;               /* [nsteps]; may be NULL when t_count = 0 */
  int32_t* step_ptr;
  int nsteps;
  int clip_x0;
  double w;
  int32_t* nan_flag;
  int64_t n;
  float* x_dup0; float* x_dup1;       /* optional */
  int64_t* t_next; int t_count;       /* optional (t_count = 0) */
  uint32_t* done_counter;
} hdiff_cfg_dpmpp_loop_desc;
int hdiff_cfg_dpmpp_step_loop(const hdiff_cfg_dpmpp_loop_desc* d, hdiff_stream_t stream);
/* step bookkeeping for the captured loop: t[b] = *step for all b (int64 vector for the embedding gather) */
int hdiff_fill_t(int64_t* t, const int32_t* step_ptr, int B, hdiff_stream_t stream);
int hdiff_step_decrement(int32_t* step_ptr, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * Image-conditioned sampler of the reference's second tree (diffusion/Diffusion.py:182-269, diffusion/Model.py).
 *   hdiff_ddim_step        one deterministic DDIM update (Diffusion.py:259-263, eta = 0):
 *                          y0 = (y - eps*tab[k][0]) / tab[k][1] ; y_next = tab[k][2]*y0 + tab[k][3]*eps, k = *step_ptr;
 *                          tab[k] = {sqrt(1-at), sqrt(at), sqrt(at_next), sqrt(1-at_next)} in fp32 (host builds it with the
 *                          reference's own tensor ops); nan_flag is OR-ed with 1 on a NaN output
 *   hdiff_fill_from_table  dst[i] = table[*idx] for i < n: the DDIM time-step vector t of step k (Diffusion.py:249)
 *   hdiff_resize_nearest   F.interpolate(mode="nearest") of [BC][H][W] to [BC][OH][OW] (skip tensors, Model.py:503-504)
 *   hdiff_avgpool_global   nn.AdaptiveAvgPool2d((1,1)) of [BC][HW] -> [BC] (ConditionalEmbedding, Model.py:124,150)
 *   hdiff_concat2          out[b] = [a[b] (n0 floats) | b[b] (n1 floats)]: torch.cat([input_image, y_t], dim=1) of
 *                          Diffusion.py:229,252 (3 + 3 channels: too narrow for the conv's two-pointer input)
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_ddim_step(const float* y, const float* eps, float* y_next, const float* tab, const int32_t* step_ptr,
                    int nsteps /* rows of tab: k = *step_ptr is clamped into [0, nsteps) */, int32_t* nan_flag, int64_t n,
                    hdiff_stream_t stream);
int hdiff_fill_from_table(int64_t* dst, const int32_t* table, const int32_t* idx, int table_len /* *idx is clamped */, int n,
                          hdiff_stream_t stream);
int hdiff_resize_nearest(const float* x, float* y, int BC, int H, int W, int OH, int OW, hdiff_stream_t stream);
int hdiff_avgpool_global(const float* x, float* y, int BC, int HW, hdiff_stream_t stream);
int hdiff_concat2(const float* a, const float* b, float* out, int B, int64_t n0, int64_t n1, hdiff_stream_t stream);
/* One DPM-Solver++(2M) update of the same sampler (an addition to the reference; hdiff_cfg_dpmpp_step's update with eps as the model
 * gives it): y0 = (y - eps*tab[k][0]) / tab[k][1] ; clip_x0 != 0: y0 = clamp(y0, -1, 1) ; v = tab[k][2]*y + tab[k][3]*y0 ;
 * tab[k][4] != 0: v = v + tab[k][4]*x0_prev ; x0_prev = y0 ; y_next = v, with k = *step_ptr clamped into [0, nsteps) and
 * tab[k] = {s1m, sa, A, B, C} in fp32 (dpmpp_table with shift = 1, final_alpha_bar = alphas_bar[0]).  x0_prev [n] is the caller's
 * persistent history, not read when tab[k][4] == 0 and always written; nan_flag is OR-ed with 1 on a NaN output; y and y_next may
 * alias. */
int hdiff_dpmpp_step(const float* y, const float* eps, float* y_next, float* x0_prev, const float* tab /* [nsteps][5] */,
                     const int32_t* step_ptr, int nsteps, int clip_x0, int32_t* nan_flag, int64_t n, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * Multi-sample posterior sampling of the same sampler (`posterior`, `eta=`; additions to the reference and to ABI 6).  A batch is
 * `rows` samples of n_per floats; sample r draws ALL its noise from the Philox stream of seeds[r] (device memory), quads counted
 * WITHIN the row, so a sample's numbers depend on neither its place in the batch nor on the batch's size.
 *   hdiff_randn_rows      row r of out [rows][n_per] is hdiff_randn(n_per, seeds[r], offset) bit for bit; with n_per % 4 != 0 the last
 *                         quad of a row is partly used and the next row starts a fresh one
 *   hdiff_ddim_eta_step   Diffusion.py:259-267 with the stochastic term kept: y0 = (y - eps*tab[k][0]) / tab[k][1] ;
 *                         y_next = ((tab[k][2]*y0) + (tab[k][3]*z)) + (tab[k][4]*eps), one fp32 rounding per written operation,
 *                         k = *step_ptr clamped into [0, nsteps), tab[k] = {sqrt(1-at), sqrt(at), sqrt(at_next), c1, c2}.  z is
 *                         read from `noise` [rows][n_per] or, with noise == NULL, drawn: row r is hdiff_randn(n_per, seeds[r],
 *                         offset = k).  Noise is added at every step, k = 0 included.  y and y_next may alias; any 4-byte aligned
 *                         pointers; nan_flag is OR-ed with 1 on a NaN output; with tab[k][3] == 0 and finite z the result equals
 *                         hdiff_ddim_step's
 *   hdiff_sample_stats    samples [B][K][n] -> mean, std [B][n]: per element, in double, in replica order, m = (sum x_k) / K and
 *                         std = sqrt(sum (x_k - m)^2 / (K - 1)), exactly 0 for K = 1; each rounded once to fp32
 * One launch each; no allocation, no synchronisation, no float atomics: legal under stream capture, bitwise repeatable.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_randn_rows(float* out, int rows, int64_t n_per, const uint64_t* seeds, uint64_t offset, hdiff_stream_t stream);
int hdiff_ddim_eta_step(const float* y, const float* eps, const float* noise /* or NULL */, float* y_next,
                        const float* tab /* [nsteps][5] */, const uint64_t* seeds /* [rows]; may be NULL with noise */,
                        int64_t n_per, const int32_t* step_ptr, int nsteps, int32_t* nan_flag, int rows, hdiff_stream_t stream);
int hdiff_sample_stats(const float* samples, int B, int K, int64_t n, float* mean, float* std, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * A v-prediction network (v = sqrt(ab) * noise - sqrt(1 - ab) * x_0, Salimans & Ho 2022) in front of the same sampler's updates (the
 * sampler's `prediction="v"`; an addition to the reference and to ABI 6).
 *   hdiff_v_to_eps   row b of out [B][n_per], in place:  out = sqrt_ab[t[b]] * out + sqrt_1mab[t[b]] * y  -- the noise estimate that
 *                    every update above takes, two products and one sum, one fp32 rounding each.  sqrt_ab / sqrt_1mab: fp32 tables
 *                    of length T at the index the model was CALLED with (the trainer's alphas_bar[t], not the DDIM loop's
 *                    alphas_bar[t + 1]); t[b] is clamped into [0, T).  y [B][n_per] is the state the model saw.  Any 4-byte aligned
 *                    pointers and any n_per; an element's result depends on its own two inputs alone
 * One launch; no allocation, no synchronisation, no atomics: legal under stream capture, bitwise repeatable.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_v_to_eps(float* out, const float* y, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab, int T, int B,
                   int64_t n_per, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * Overlapping-window DDIM sampling of the second tree's sampler (the `tile=` argument; an addition to the reference).
 * Layout: per axis a table of window origins (origin_y[ny], origin_x[nx]); window (b, iy, ix) has index (b*ny + iy)*nx + ix
 * and covers rows origin_y[iy] .. + th - 1 and columns origin_x[ix] .. + tw - 1 of a [B][C][H][W] tensor (th <= H, tw <= W).
 * The windows covering row py are the consecutive run first_y[py] .. first_y[py] + count_y[py] - 1 (count <= 3) with the
 * normalised fp32 weights weight_y[py][0..2]; columns likewise.  The weight of window (iy, ix) at a pixel is ay * ax.
 *   hdiff_tile_gather      out[slot] = the [C][th][tw] crop of window min(w0 + slot, B*ny*nx - 1) for slot < n_slots (slots past
 *                          the last window repeat it: the padding of a short final chunk); origins are clamped into the
 *                          tensor in the kernel.  With ny = nx = 1, th = H, tw = W it is a copy of samples w0 .. w0 + n_slots - 1
 *   hdiff_tile_ddim_step   one DDIM step on the full image y [B][C][H][W], in place, from the windows' noise estimates
 *                          eps_w [B*ny*nx][C][th][tw]: eps = sum over jy (outer), jx (inner), ascending, of
 *                          (ay * ax) * eps_w[window][c][py - oy][px - ox], the first product initialising the sum; then
 *                          hdiff_ddim_step's update with the same tab / step_ptr / nsteps / nan_flag (one atomicOr per wave).
 *                          fp32, no contraction, no atomics on y: bitwise repeatable; one window of weight 1.0 gives
 *                          hdiff_ddim_step bit for bit.  Table entries are clamped: no access leaves eps_w
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_tile_gather(const float* x, float* out, const int32_t* origin_y, const int32_t* origin_x, int B, int C, int H, int W,
                      int ny, int nx, int th, int tw, int w0 /* first window, 0 <= w0 < B*ny*nx */, int n_slots,
                      hdiff_stream_t stream);
int hdiff_tile_ddim_step(float* y, const float* eps_w, const int32_t* first_y, const int32_t* count_y,
                         const float* weight_y /* [H][3] */, const int32_t* origin_y, const int32_t* first_x,
                         const int32_t* count_x, const float* weight_x /* [W][3] */, const int32_t* origin_x, const float* tab,
                         const int32_t* step_ptr, int nsteps, int32_t* nan_flag, int B, int C, int H, int W, int ny, int nx,
                         int th, int tw, hdiff_stream_t stream);
/* hdiff_tile_ddim_step's blend of the windows' noise estimates, in its fixed order, followed by hdiff_dpmpp_step's update on the full
 * image y [B][C][H][W], in place, with a full-size history x0_prev [B][C][H][W] (every pixel is read and written by one thread).
 * Same tables, clamping and repeatability; one window of weight 1.0 gives hdiff_dpmpp_step bit for bit. */
int hdiff_tile_dpmpp_step(float* y, const float* eps_w, float* x0_prev, const int32_t* first_y, const int32_t* count_y,
                          const float* weight_y /* [H][3] */, const int32_t* origin_y, const int32_t* first_x,
                          const int32_t* count_x, const float* weight_x /* [W][3] */, const int32_t* origin_x,
                          const float* tab /* [nsteps][5] */, const int32_t* step_ptr, int nsteps, int clip_x0, int32_t* nan_flag,
                          int B, int C, int H, int W, int ny, int nx, int th, int tw, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * Trainer of the second tree (diffusion/Diffusion.py:26-180) and the backward passes of its image encoder / skip resize.
 *   hdiff_train_b_loss_fwd   from noise_pred, noise, y_t, gt [B][3][HW] and t: mse = (noise_pred - noise)^2,
 *                            y0_pred = ((1 / sqrt_ab[t]) * (y_t - sqrt_1mab[t] * noise_pred)) / 255 (the reference's trailing
 *                            / 255 kept), col[0] = 1 - mean over pixels of cosine_similarity(normalize(y0_pred), normalize(gt))
 *                            over the channel axis (eps 1e-12 / 1e-8 as torch).  sqrt_ab / sqrt_1mab: fp32 tables of length T,
 *                            t[b] clamped into [0, T).  workspace: hdiff_train_b_loss_workspace(B * HW) bytes (per-block
 *                            partial sums, reduced in a fixed order: bitwise reproducible)
 *   hdiff_train_b_loss_bwd   d_noise_pred from d_mse [B][3][HW], d_y0 (an external dL/dy0_pred) and d_col (device scalar),
 *                            each of which may be NULL, in one pass
 *   hdiff_train_b_tail_fwd / _bwd   the same pair (the same kernels) with what the network's output `out` stands for, an optional
 *                            weight of the squared error and the y0 divisor as arguments (additions to the reference and to ABI 6).
 *                            With a = sqrt_ab[t], s = sqrt_1mab[t], one fp32 rounding per written operation:
 *                              HDIFF_PREDICT_EPS  target = noise               y0_pred = ((1 / a) * (y_t - s * out)) / y0_div
 *                                                 dy0/dout = -(1 / a) * s / y0_div
 *                              HDIFF_PREDICT_V    target = a * noise - s * gt  y0_pred = (a * y_t - s * out) / y0_div
 *                                                 dy0/dout = -s / y0_div                            (Salimans & Ho 2022)
 *                            mse = weight_tab[t] * (out - target)^2 with a table of length T, (out - target)^2 with NULL (no multiply
 *                            is executed); the weight reaches the mse term alone, forward and backward.  y0_div: any number but
 *                            0.  (HDIFF_PREDICT_EPS, NULL, 255.0f) is hdiff_train_b_loss_fwd / _bwd, which forward here
 *   hdiff_avgpool_global_bwd dx[bc][i] = dy[bc] / HW (AdaptiveAvgPool2d((1,1)), Model.py:150)
 *   hdiff_resize_nearest_bwd the backward of hdiff_resize_nearest ([BC][H][W] -> [BC][OH][OW]) in gather form: dx[bc][iy][ix] =
 *                            the sum, in increasing output order, of the dy elements that read it (no atomics)
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_train_b_loss_workspace(int64_t pixels, int64_t* bytes);
int hdiff_train_b_loss_fwd(const float* noise_pred, const float* noise, const float* y_t, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, float* mse, float* y0_pred,
                           float* col, void* workspace, hdiff_stream_t stream);
int hdiff_train_b_loss_bwd(const float* noise_pred, const float* noise, const float* y0_pred, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, const float* d_mse,
                           const float* d_y0, const float* d_col, float* d_noise_pred, hdiff_stream_t stream);
enum { HDIFF_PREDICT_EPS = 0, HDIFF_PREDICT_V = 1 };
int hdiff_train_b_tail_fwd(const float* out, const float* noise, const float* y_t, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, float* mse, float* y0_pred,
                           float* col, void* workspace, int prediction, const float* weight_tab /* [T] or NULL */, float y0_div,
                           hdiff_stream_t stream);
int hdiff_train_b_tail_bwd(const float* out, const float* noise, const float* y0_pred, const float* gt, const int64_t* t,
                           const float* sqrt_ab, const float* sqrt_1mab, int T, int B, int HW, const float* d_mse,
                           const float* d_y0, const float* d_col, float* d_out, int prediction,
                           const float* weight_tab /* [T] or NULL */, float y0_div, hdiff_stream_t stream);
int hdiff_avgpool_global_bwd(const float* dy, float* dx, int BC, int HW, hdiff_stream_t stream);
int hdiff_resize_nearest_bwd(const float* dy, float* dx, int BC, int H, int W, int OH, int OW, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * MS-SSIM + L1 loss of the second tree's trainer (Loss/loss.py:269-283 through kornia's MS_SSIMLoss; diffusion/Diffusion.py:171-172)
 * and its gradient with respect to the prediction x (csrc/msssim.hip).  x, y: [B][3][H][W], any H, W >= 1.
 *   A pair p filters channel pair_chan[p] with the 1-D Gaussian of scale pair_scale[p] (zero padding): l_p and cs_p from the five
 *   moments.  Per pixel: PIcs = prod cs_p^pair_cs_pow[p], lM = prod l_p^pair_l_pow[p], ms = 1 - lM PIcs,
 *   l1 = mean over channels of G_{l1_scale} * |x - y|, loss = compensation (alpha ms + (1 - alpha) l1 / data_range), then the mean
 *   (mean != 0) or the sum over [B][H][W], in a fixed two-stage order (bitwise repeatable).
 *   weights: HOST pointer, [nscales][window] normalised 1-D windows (window odd, <= 33); taps whose weight is at most 1e-12 beyond a
 *   radius of 4 / 8 are skipped (csrc/msssim.hip).
 *   hdiff_msssim_l1_workspace  saved_bytes: the moments the forward writes and the backward reads (B H W npairs 5 floats);
 *                              scratch_bytes: enough for either call, free to reuse once the call's kernels have run
 *   hdiff_msssim_l1_fwd        loss[0]; three launches
 *   hdiff_msssim_l1_bwd        dx = d_loss[0] (device scalar) * d loss / d x from the forward's `saved`; two launches; sign(0) = 0
 * Arguments are validated on the host before any launch (C != 3, more than 5 scales, a window above 33, null pointers: -1).
 * ------------------------------------------------------------------------------------------------------------------ */
#define HDIFF_MSSSIM_MAX_PAIRS 15
#define HDIFF_MSSSIM_MAX_SCALES 5
#define HDIFF_MSSSIM_MAX_WINDOW 33
typedef struct hdiff_msssim_desc {
  int B, C, H, W;
  int nscales, window;
  const float* weights;
  int npairs;
  int pair_chan[HDIFF_MSSSIM_MAX_PAIRS], pair_scale[HDIFF_MSSSIM_MAX_PAIRS];
  int pair_cs_pow[HDIFF_MSSSIM_MAX_PAIRS], pair_l_pow[HDIFF_MSSSIM_MAX_PAIRS];
  int l1_scale;
  float C1, C2, alpha, compensation, data_range;
  int mean;
} hdiff_msssim_desc;
int hdiff_msssim_l1_workspace(const hdiff_msssim_desc* d, int64_t* saved_bytes, int64_t* scratch_bytes);
int hdiff_msssim_l1_fwd(const hdiff_msssim_desc* d, const float* x, const float* y, float* loss, void* saved, void* scratch,
                        hdiff_stream_t stream);
int hdiff_msssim_l1_bwd(const hdiff_msssim_desc* d, const float* x, const float* y, const float* d_loss, const void* saved,
                        void* scratch, float* dx, hdiff_stream_t stream);
/* Per-image quality scores of the evaluation (csrc/quality.hip; the reference's utils/rotinas.py:916-928).  a, b: fp32 [N][3][H][W],
 * nominal range [0, 1]; every score is taken on v = min(max(x, 0), 1) * 255 in fp32.  Outputs are float64 device rows.
 *   hdiff_quality_workspace  bytes of `scratch` for either call at (N, H, W)
 *   hdiff_psnr_ssim          out[n] = {PSNR (dB, range 255; +inf for identical images), SSIM (7x7 uniform window, interior positions,
 *                            sample covariance, channels averaged)}; H, W >= 7; two launches
 *   hdiff_uiqm               out[n] = {UICM, UISM, UIConM, UIQM = 0.0282 UICM + 0.2953 UISM + 3.5753 UIConM}; H, W >= 8; twelve launches;
 *                            an image with a constant channel has UISM = UIQM = NaN (the definition divides by the largest gradient)
 * N in [1, 65535], H * W <= 2^30.  A non-finite input value makes the scores of ITS image NaN.  No allocation, no synchronisation, no
 * float atomics: legal under stream capture, bitwise repeatable, and an image's scores do not depend on N or its place in the batch. */
int hdiff_quality_workspace(int N, int H, int W, int64_t* bytes);
int hdiff_psnr_ssim(const float* a, const float* b, int N, int H, int W, double* out, void* scratch, hdiff_stream_t stream);
int hdiff_uiqm(const float* a, int N, int H, int W, double* out, void* scratch, hdiff_stream_t stream);
/* UCIQE per image (csrc/uciqe.hip; the UCIQE part of the reference's `nmetrics`, metrics/metrics.py:301-337, called at
 * utils/rotinas.py:923 and :1171).  a: fp32 [N][3][H][W]; rgb = double(min(max(x, 0), 1)) * scale is converted to CIE L*a*b* (D65) in
 * double.  scale = 1 scores the image on its colour range; scale = 255 evaluates what the reference's call evaluates (it hands
 * skimage.color.rgb2lab a float image in [0, 255], which takes floats as being in [0, 1] already).
 *   hdiff_uciqe_workspace    bytes of `scratch` for hdiff_uciqe at (N, H, W) (two double planes per image and the partials; NOT
 *                            covered by hdiff_quality_workspace, which returns what it always did)
 *   hdiff_uciqe              out[n] = {sc = sqrt(mean((chroma - mean chroma)^2)), conl = mean(top largest L) - mean(top smallest L) with
 *                            top = round_half_even(0.01 H W), us = mean(chroma / L, 0 where either is 0),
 *                            UCIQE = 0.4680 sc + 0.2745 conl + 0.2576 us}; top == 0 (H W < 50): conl = UCIQE = NaN; sixteen launches
 * N in [1, 65535], H, W >= 1, H * W <= 2^30, scale finite and > 0.  The cut values of L are selected on the 64-bit key of the double and
 * ties at a cut are counted exactly.  A non-finite input value makes the four scores of ITS image NaN.  No allocation, no
 * synchronisation, no float atomics: legal under stream capture, bitwise repeatable, independent of N and of the place in the batch. */
int hdiff_uciqe_workspace(int N, int H, int W, int64_t* bytes);
int hdiff_uciqe(const float* a, int N, int H, int W, double scale, double* out, void* scratch, hdiff_stream_t stream);
/* Colour difference between a prediction and its target, per image (csrc/color_diff.hip; tests/_color_def.py is the definition the
 * kernels are held to; the reference has no such score).  pred, target: fp32 [N][3][H][W]; rgb = double(min(max(x, 0), 1)) of both is
 * converted to CIE L*a*b* (sRGB, D65, the conversion of hdiff_uciqe) in double.  Per pixel: CIEDE2000 after Sharma, Wu and Dalal 2005
 * with kL = kC = kH = 1 (pinned to their published table by tests/golden/ciede2000_sharma.json), CIE76, and the angle in degrees
 * between the two clipped RGB vectors, atan2(|u x v|, u . v), counted where neither vector is black.
 *   hdiff_color_diff_workspace   bytes of `scratch` for hdiff_color_diff at (N, H, W) (one double plane per image, the histograms and the
 *                                partials)
 *   hdiff_color_diff             out[n] = {mean CIEDE2000, its nearest-rank 95th percentile (element (95 H W + 99) / 100 - 1 of the
 *                                ascending sort), mean CIE76, mean angle over the counted pixels (NaN when there are none)}; map: NULL, or
 *                                fp32 [N][1][H][W] that receives the per-pixel CIEDE2000 rounded once; fifteen launches
 *   hdiff_ciede2000_lab          out[i] = CIEDE2000 of the double rows lab1[i], lab2[i] ([n][3]: L, a, b) through the same device function;
 *                                n in [1, 2^30]; one launch, no scratch
 * N in [1, 65535], H, W >= 1, H * W <= 2^30.  The percentile is selected on the 64-bit key of the double and is exact at ties.  A
 * non-finite input value in either image makes the four scores of ITS image NaN.  No allocation, no synchronisation, no float atomics:
 * legal under stream capture, bitwise repeatable, independent of N and of the place in the batch.  Additions to ABI 6. */
int hdiff_color_diff_workspace(int N, int H, int W, int64_t* bytes);
int hdiff_color_diff(const float* pred, const float* target, int N, int H, int W, double* out, float* map, void* scratch,
                     hdiff_stream_t stream);
int hdiff_ciede2000_lab(const double* lab1, const double* lab2, int64_t n, double* out, hdiff_stream_t stream);
/* NIQE (csrc/niqe.hip; Mittal, Soundararajan, Bovik 2013; tests/_niqe_def.py is the definition the kernels are held to; agreement with
 * the authors' MATLAB release is unpinned).  img: fp32 [N][3][H][W] in [0, 1].  The gray plane (quantize != 0: channels and gray rounded
 * to 8-bit values, as a file holds them) is cropped from the top-left corner to bh = H / patch by bw = W / patch whole blocks; P = bh bw.
 * Per block and scale (block side patch, then patch / 2 on the plane reduced by the 8-tap bicubic): the 18 AGGD features of the
 * mean-subtracted contrast-normalised block and of its four neighbour products (shifted circularly inside the block); a row is the 36
 * features of a block, scale 1 first.  Everything in double.
 *   hdiff_niqe_workspace     bytes of `scratch` for hdiff_niqe_features at (N, H, W, patch): four double planes per image
 *   hdiff_niqe_features      feats [N][P][36], sharp [N][P] (the mean of sigma over the block at scale 1).  A block without negative or
 *                            without positive values (a constant area) has non-finite features; an image with a NaN pixel inside the
 *                            crop has NaN in every feature.  Nine launches, one more while the device's table is not built (the
 *                            table kernel runs on the stream of the first call on a device: a first call on ANOTHER stream at the same
 *                            time must be ordered behind it by the caller)
 *   hdiff_niqe_moments       out [N][36 + 36 * 36 + 1]: mean, unbiased covariance and count of the VALID rows of each image, rows added
 *                            in index order, two passes.  A row is valid if its 36 features are finite and, with sharp_threshold > 0,
 *                            sharp > sharp_threshold * max(sharp of the image).  count < 2: NaN covariance; count = 0: NaN mean.  One launch
 *   hdiff_niqe_keep          keep [N][P] (int, 0 / 1): the validity above, for a bank of rows that outlives its images.  One launch
 *   hdiff_niqe_pool_moments  out [36 + 36 * 36 + 1] over the rows of a bank feats [rows][36] whose keep[r] != 0, in index order: the
 *                            pristine fit over many images, without a copy to the host.  One launch
 * N in [1, 65535]; H, W in [patch, 16384]; patch even, in [8, 512]; P <= 2^22; rows <= 2^26; sharp_threshold in [0, 1) (sharp may be
 * NULL at 0).  No allocation, no synchronisation, no float atomics: legal under stream capture, bitwise repeatable; an image's rows and
 * moments do not depend on N or on its place in the batch.  Deviations from the release, all deliberate: rows with a non-finite
 * feature leave mean AND covariance (the release drops them per column for the mean); the score's pseudo-inverse is taken on the host
 * with numpy's cutoff.  Additions to ABI 6. */
int hdiff_niqe_workspace(int N, int H, int W, int patch, int64_t* bytes);
int hdiff_niqe_features(const float* img, int N, int H, int W, int patch, int quantize, double* feats, double* sharp, void* scratch,
                        hdiff_stream_t stream);
int hdiff_niqe_moments(const double* feats, const double* sharp, int N, int P, double sharp_threshold, double* out,
                       hdiff_stream_t stream);
int hdiff_niqe_keep(const double* feats, const double* sharp, int N, int P, double sharp_threshold, int* keep, hdiff_stream_t stream);
int hdiff_niqe_pool_moments(const double* feats, const int* keep, int rows, double* out, hdiff_stream_t stream);
/* Set-level statistics of feature rows (csrc/distribution.hip; tests/_distribution_def.py is the definition): what a Frechet distance
 * and a KID over a feature extractor need.  Features are fp32, n rows of d values, value (r, i) at feats[r * row_stride + i * ch_stride]
 * (strides in elements, both >= 1), so the class-token view of a channel-major (B, C, L) tensor is read in place.  Outputs are double.
 *   hdiff_feat_moments       mean[i] = (sum over r = 0 .. n-1, in that order, of (double)x[r][i]) / n; cov[i][j] = (sum over r in that
 *                            order of (x[r][i] - mean[i]) * (x[r][j] - mean[j])) / (n - 1), difference, product and sum rounded apart;
 *                            cov is [d][d], both halves written, bit for bit symmetric; n = 1 gives a NaN cov and no error.  Two launches
 *   hdiff_kid_workspace      bytes of `scratch` for hdiff_kid_sums at (n, m)
 *   hdiff_kid_sums           with k(x, y) = (x.y / d + 1)^3, x.y summed over the channels 0 .. d-1 in order, the cube as (t * t) * t:
 *                            out[0] = sum of k(a_i, a_j) over i != j, out[1] = the same over b, out[2] = sum of k(a_i, b_j) over all
 *                            pairs; one partial per workgroup in a slot of its own, added in a fixed order.  A call with a and b
 *                            swapped returns out[1], out[0], out[2] bit for bit.  Four launches
 * n, m in [1, 32768], d in [1, 8192].  A non-finite feature spoils what it touches (the mean and the cov entries of its channel; all
 * three sums a row of its set enters) and raises nothing.  No allocation, no synchronisation, no float atomics: legal under stream
 * capture, bitwise repeatable.  Additions to ABI 6. */
int hdiff_feat_moments(const float* feats, int n, int d, int64_t row_stride, int64_t ch_stride, double* mean, double* cov,
                       hdiff_stream_t stream);
int hdiff_kid_workspace(int n, int m, int64_t* bytes);
int hdiff_kid_sums(const float* a, int n, const float* b, int m, int d, int64_t a_row_stride, int64_t a_ch_stride,
                   int64_t b_row_stride, int64_t b_ch_stride, double* out, void* scratch, hdiff_stream_t stream);
/* What a VGG feature trunk, the losses on its taps and the LPIPS score need beside the conv kernels (csrc/perceptual.hip;
 * hdiff_amd/perceptual.py is the caller, tests/_perceptual_def.py the definitions).  fp32 tensors, dense; every written operation
 * rounds once (no contraction).  n and planes * H * W in [1, 2^40].
 *   hdiff_relu_fwd           y = x > 0 ? x : 0, and a NaN stays a NaN (as torch.relu); y may alias x
 *   hdiff_relu_bwd           dx = y > 0 ? dy : 0: reads the forward OUTPUT, so the forward can run in place; dx aliases neither input
 *   hdiff_maxpool2_fwd       2x2 window, stride 2, floor mode over [planes][H][W] -> [planes][H / 2][W / 2]; H, W >= 2; a last odd row /
 *                            column is dropped; the maximum is the first element in row-major order that no later one exceeds (a NaN counts as
 *                            maximal: a window that holds one gives NaN)
 *   hdiff_maxpool2_bwd       a gather from the forward INPUT x: dx = dy of the window where the element is that first maximal one, else 0
 *                            (0 for the dropped row / column); no index tensor exists
 *   hdiff_l1_mean_workspace  bytes of `scratch` for hdiff_l1_mean_fwd at n
 *   hdiff_l1_mean_fwd        out[0] = (float)(sum_i double(fabsf(a[i] - b[i])) / n): each term rounded to fp32, summed in double in a
 *                            fixed order (per-workgroup partials, then one workgroup), divided once.  b == NULL: mean |a|.  Two launches
 *   hdiff_l1_mean_bwd        da = a > b ? c : a < b ? -c : 0 with c = g[0] / (float)n, g a device scalar (b == NULL: compared with 0);
 *                            b receives no gradient
 *   hdiff_charbonnier_fwd    y = sqrtf(d * d + 1) - 1, d = a - b
 *   hdiff_charbonnier_bwd    da = (dy / divisor) * d / sqrtf(d * d + 1); dy_is_scalar = 1 reads dy[0] for every element (a reduced
 *                            loss: divisor = n for the mean, 1 for the sum); divisor >= 1, and 1 leaves an elementwise dy as it is
 *   hdiff_lpips_layer_workspace   bytes of `scratch` for hdiff_lpips_layer at (N, C, H, W)
 *   hdiff_lpips_layer        f0, f1: [N][C][H][W], w: [C].  out[n] += mean over pixels of sum_c w[c] (f0[c] / (|f0| + 1e-10) -
 *                            f1[c] / (|f1| + 1e-10))^2, |f| the L2 norm over the channels at the pixel; norms, sums and the mean in double,
 *                            fixed order.  out is float64 [N] and is ADDED to: the caller zeroes it, five calls accumulate in call order.
 *                            A non-finite feature makes out[n] of ITS image NaN.  N in [1, 65535], C in [1, 65536], H * W <= 2^30.  Two launches
 *   hdiff_scale_input        y = ((x * mul + add) - shift[c]) / scale[c] over [N][C][H][W] (LPIPS: mul 2, add -1, then its shift / scale)
 * No allocation, no synchronisation, no float atomics: legal under stream capture, bitwise repeatable; a reduction's grid depends on
 * n (per image: on H * W) alone.  Additions to ABI 6. */
int hdiff_relu_fwd(const float* x, float* y, int64_t n, hdiff_stream_t stream);
int hdiff_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, hdiff_stream_t stream);
int hdiff_maxpool2_fwd(const float* x, float* y, int64_t planes, int H, int W, hdiff_stream_t stream);
int hdiff_maxpool2_bwd(const float* x, const float* dy, float* dx, int64_t planes, int H, int W, hdiff_stream_t stream);
int hdiff_l1_mean_workspace(int64_t n, int64_t* bytes);
int hdiff_l1_mean_fwd(const float* a, const float* b, int64_t n, float* out, void* scratch, hdiff_stream_t stream);
int hdiff_l1_mean_bwd(const float* a, const float* b, const float* g, int64_t n, float* da, hdiff_stream_t stream);
int hdiff_charbonnier_fwd(const float* a, const float* b, float* y, int64_t n, hdiff_stream_t stream);
int hdiff_charbonnier_bwd(const float* a, const float* b, const float* dy, int dy_is_scalar, float divisor, float* da, int64_t n,
                          hdiff_stream_t stream);
int hdiff_lpips_layer_workspace(int N, int C, int H, int W, int64_t* bytes);
int hdiff_lpips_layer(const float* f0, const float* f1, const float* w, int N, int C, int H, int W, double* out, void* scratch,
                      hdiff_stream_t stream);
int hdiff_scale_input(const float* x, const float* shift, const float* scale, float mul, float add, float* y, int N, int C, int H,
                      int W, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * The pieces of a frozen DINOv2 ViT trunk around the dense layers (hdiff_conv2d_fwd, one tap) and the attention core
 * (hdiff_mha_flash_*), and the smooth-L1 sums on its taps (csrc/dino.hip; tests/_dino_def.py is the definition; hdiff_amd/dino.py is
 * the caller).  Activations are fp32 [B][C][L], class token at position 0.  No float atomics, fixed summation orders, no allocation,
 * no synchronisation: legal under stream capture; an image's numbers do not depend on the batch.  Additions to ABI 6.
 *   hdiff_dino_unfold      x [B][3][H][W] -> cols [B][588][h*w], h = (H-4)/14, w = (W-4)/14: the 14x14 patches of the window that
 *                          starts 2 pixels in from each edge, rows in Conv2d(3, C, 14, 14).weight order (c, ky, kx).  H - 4 and W - 4
 *                          must be positive multiples of 14.
 *   hdiff_dino_fold        its adjoint as a gather: dx [B][3][H][W] from dcols, zeros on the 2-pixel border.
 *   hdiff_dino_tokens_fwd  tok[b][c][0] = cls[c] + pos[c][0]; tok[b][c][l] = patch[b][c][l-1] + pos[c][l]; pos is [C][L].
 *   hdiff_dino_tokens_bwd  dpatch[b][c][l] = dtok[b][c][l+1].
 *   hdiff_layernorm_fwd    y = (x - mean) * rstd * gamma[c] + beta[c] over C per token; mean / rstd [B][L] in double (both NULL: not
 *                          kept).  Two passes in double: exact at mean = 1e3 x spread; a constant row gives beta exactly.
 *   hdiff_layernorm_bwd    dx = add + rstd * (g - mean_c(g) - xhat * mean_c(g xhat)), g = dy * gamma; add may be NULL or dx itself.
 *   hdiff_gelu_fwd / _bwd  x * Phi(x) and dy * (Phi(x) + x phi(x)), evaluated in double (erfc), rounded once; dx may be dy.
 *   hdiff_layerscale_fwd   s = gamma[c] * x (s may be NULL), y = res + s.   hdiff_layerscale_bwd: dx = gamma[c] * ds (dx may be ds).
 *   hdiff_smooth_l1_tap_*  a tap is B images of n_img elements, element j of image b at [b * img_stride + j * stride].  _fwd writes
 *                          slot[b] = weight / (B n_img) * sum_j smooth_l1(a - t) (beta = 1; double, fixed order; scratch of
 *                          _workspace bytes); _total adds the [ntaps][B] slots per image in slot order, then the images in order, and
 *                          rounds once: out[0], and per_image[B] when not NULL; _bwd writes da_out = da_in + ((g[0] * weight) /
 *                          (float)(B n_img)) * clamp(a - t, -1, 1) in fp32 in that order (da_in NULL: 0; da_in may be da_out).
 *                          At most 256 images per call.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_dino_unfold(const float* x, float* cols, int B, int H, int W, hdiff_stream_t stream);
int hdiff_dino_fold(const float* dcols, float* dx, int B, int H, int W, hdiff_stream_t stream);
int hdiff_dino_tokens_fwd(const float* patch, const float* cls, const float* pos, float* tok, int B, int C, int L,
                          hdiff_stream_t stream);
int hdiff_dino_tokens_bwd(const float* dtok, float* dpatch, int B, int C, int L, hdiff_stream_t stream);
int hdiff_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, double* mean, double* rstd, int B,
                        int C, int L, hdiff_stream_t stream);
int hdiff_layernorm_bwd(const float* x, const float* gamma, const double* mean, const double* rstd, const float* dy, const float* add,
                        float* dx, int B, int C, int L, hdiff_stream_t stream);
int hdiff_gelu_fwd(const float* x, float* y, int64_t n, hdiff_stream_t stream);
int hdiff_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, hdiff_stream_t stream);
int hdiff_layerscale_fwd(const float* x, const float* gamma, const float* res, float* s, float* y, int B, int C, int L,
                         hdiff_stream_t stream);
int hdiff_layerscale_bwd(const float* ds, const float* gamma, float* dx, int B, int C, int L, hdiff_stream_t stream);
int hdiff_smooth_l1_tap_workspace(int B, int64_t n_img, int64_t* bytes);
int hdiff_smooth_l1_tap_fwd(const float* a, const float* t, int B, int64_t n_img, int64_t stride, int64_t img_stride, double weight,
                            double* slot, void* scratch, hdiff_stream_t stream);
int hdiff_smooth_l1_tap_total(const double* slots, int ntaps, int B, float* out, float* per_image, hdiff_stream_t stream);
int hdiff_smooth_l1_tap_bwd(const float* a, const float* t, const float* g, int B, int64_t n_img, int64_t stride, int64_t img_stride,
                            float weight, const float* da_in, float* da_out, hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * A dense layer along a token axis of any length (csrc/dense_tokens.hip): y[b, co, l] = bias[co] + sum_ci w[co, ci] x[b, ci, l] on
 * fp32 channel-major x (B, Cin, L), y (B, Cout, L); bias may be NULL.  The contraction is the bf16-triple scheme of
 * HDIFF_CONTRACT_BF16X3 (six piece products with i + j <= 2, fp32 accumulation) WHATEVER the contraction mode is: the caller chooses
 * this entry or a convolution.  Any Cin, Cout, L >= 1 with Cin * L and Cout * L below 2^31.
 *   hdiff_dense_pack_words  the 32-bit words of the pack of a GEMM with Cout outputs and Cin inputs: ceil(Cin / 16) * 3 * 64
 *                           ceil(Cout / 64) * 8 (6 bytes per padded weight).
 *   hdiff_dense_pack        w [Cout][Cin] (device, fp32) -> the pre-split operand wp3 (device, 16-byte aligned), K padded to 16 and the
 *                           channels to 64 with zeros.  transposed != 0 packs w^T: a GEMM with Cin outputs and Cout inputs, the operand
 *                           of the input gradient dx = w^T dy; its size is hdiff_dense_pack_words(Cin, Cout).
 *   hdiff_dense_tokens      Cin, Cout are the GEMM's own (for the input gradient: Cin = rows of w, Cout = columns of w).  x values
 *                           outside Cin x L are never multiplied (a NaN beside the tensor stays outside), nothing outside y is written.
 * One launch each, no atomics, no workspace, a fixed accumulation order: bitwise repeatable, an image's numbers do not depend on its
 * batch; legal under stream capture.  Additions to ABI 6.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_dense_pack_words(int Cout, int Cin, int64_t* words_out);
int hdiff_dense_pack(const float* w, void* wp3, int Cout, int Cin, int transposed, hdiff_stream_t stream);
int hdiff_dense_tokens(const float* x, const void* wp3, const float* bias, float* y, int B, int Cin, int Cout, int64_t L,
                       hdiff_stream_t stream);
/* ------------------------------------------------------------------------------------------------------------------
 * Guided full-resolution transfer (csrc/transfer.hip; tests/_transfer_def.py is the definition; hdiff_amd/transfer.py is the caller):
 * the model's 256 x 256 result decides what the enhancement IS, as one affine colour map per pixel neighbourhood (He et al.'s guided
 * filter with a colour guide, "fast" form), and the smoothly upsampled map is applied to the file at its own size.
 *   hdiff_resample_workspace  bytes of `scratch` for hdiff_resample_u8 at (H, W) -> (h, w): the [H][w][3] intermediate in double
 *   hdiff_resample_u8         img uint8 [H][W][3] (interleaved) -> out float [3][h][w] in [0, 255].  A triangle filter of support
 *                             max(in / out, 1) per axis, horizontal pass first: output o has centre c = (o + 0.5) in / out, taps k from
 *                             max(int(c - support + 0.5), 0) to min(int(c + support + 0.5), in) - 1, weights max(0, 1 - |(k + 0.5 - c) /
 *                             support|) normalised to sum 1 in double, products added in tap order in double, one rounding to fp32
 *                             (Pillow's BILINEAR reduce without its 8-bit rounding between the passes).  Equal sizes copy the bytes.
 *                             H, W in [1, 16384]; h, w in [1, 4096].  Two launches
 *   hdiff_guided_workspace    bytes of `scratch` for hdiff_guided_fit at (N, h, w): 21 + 12 double planes per image
 *   hdiff_guided_fit          I, p: float [N][3][h][w] (guide and target, [0, 1] units) -> coef float [N][12][h][w], planes a[0][0..2],
 *                             a[1][0..2], a[2][0..2], b[0..2].  Window of (y, x): [y-r, y+r] x [x-r, x+r] clipped to the image; a mean is
 *                             the sum over it divided by its pixel count, the sum separable (x, then y) and DIRECT, in index order.
 *                             Sigma = mean(I I^T) - mean(I) mean(I)^T + eps U, C[j][c] = mean(I_j p_c) - mean(I_j) mean(p_c), a[c] =
 *                             Sigma^-1 C[:, c] (Cholesky), b[c] = mean(p_c) - a[c] . mean(I); then the same window mean of the twelve
 *                             values.  Double from the loads to the one final rounding.  N in [1, 65535]; h, w in [1, 4096]; r in
 *                             [1, 128]; eps finite and > 0.  Four launches
 *   hdiff_guided_apply_f32    coef [N][12][h][w], full and out float [N][3][H][W]: out_c = A_c0 F_0 + A_c1 F_1 + A_c2 F_2 + b_c, each of
 *                             the twelve planes interpolated at sy = clamp((Y + 0.5) h / H - 0.5, 0, h - 1), y0 = floor(sy), y1 =
 *                             min(y0 + 1, h - 1), fy = sy - y0 and the same in x: along x at both rows, then along y.  clamp != 0: to
 *                             [0, 1].  fp32; the tap is taken in integers, its weight from the integer remainder.  One launch
 *   hdiff_guided_apply_u8     ONE image: coef [12][h][w], full and out uint8 [H][W][3]; F = (float)byte / 255.0f, out =
 *                             rintf(255 * clamp(q, 0, 1)), half to even.  Rows may start on any byte.  One launch
 *                             Both: h, w in [1, 4096]; H, W in [1, 16384]; H * W <= 2^30; (f32) N in [1, 65535].  out == full is allowed.
 * A non-finite input value spoils its own image only.  No allocation, no synchronisation, no atomics: legal under stream capture,
 * bitwise repeatable; an image's numbers do not depend on N or on its place in the batch.  Additions to ABI 6.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_resample_workspace(int H, int W, int h, int w, int64_t* bytes);
int hdiff_resample_u8(const uint8_t* img, int H, int W, float* out, int h, int w, void* scratch, hdiff_stream_t stream);
int hdiff_guided_workspace(int N, int h, int w, int64_t* bytes);
int hdiff_guided_fit(const float* I, const float* p, int N, int h, int w, int r, double eps, float* coef, void* scratch,
                     hdiff_stream_t stream);
int hdiff_guided_apply_f32(const float* coef, int h, int w, const float* full, float* out, int N, int H, int W, int clamp,
                           hdiff_stream_t stream);
int hdiff_guided_apply_u8(const float* coef, int h, int w, const uint8_t* full, uint8_t* out, int H, int W, hdiff_stream_t stream);
/* final clip (:98) */
int hdiff_clip(const float* x, float* y, float lo, float hi, int64_t n, hdiff_stream_t stream);
/* out = a*x + b*y (y may be NULL): bias merges and other weight-preparation arithmetic */
int hdiff_axpby(float a, const float* x, float b, const float* y, float* out, int64_t n, hdiff_stream_t stream);

/* (ABI 6) The tail of an optimizer step over a LIST of tensors, replacing the caller's torch.nn.utils.clip_grad_norm_(params, grad_clip) and
 * torch.optim.AdamW.step() (reference call sites: DiffusionFreeGuidence/TrainCondition.py:61-63, :39-40).  `table` (device) holds one entry per
 * tensor; `chunks` (device, 2 ints per chunk: tensor index, chunk index inside the tensor) cuts the work into pieces of hdiff_opt_chunk()
 * elements -- both built once by the host.  Pointers need 4-byte alignment only.
 *   hdiff_grad_norm_clip_coef: partial[nchunks] scratch; norm_coef[0] = sqrt(sum g^2) over all tensors (fixed summation order, float64 final
 *                              sum), norm_coef[1] = min(1, max_norm / (norm + 1e-6)).
 *   hdiff_adamw_step:          g *= norm_coef[1] (in place, skipped when norm_coef is NULL); p *= 1 - lr wd; m += (g - m)(1 - beta1);
 *                              v = beta2 v + (1 - beta2) g^2; p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *                              (torch.optim.AdamW's single-tensor formulas in its order of operations; step counts from 1). */
typedef struct { float* p; float* g; float* m; float* v; long long n; } hdiff_opt_tensor;
int hdiff_opt_chunk(void);
int hdiff_grad_norm_clip_coef(const hdiff_opt_tensor* table, const int* chunks, int nchunks, float* partial, float max_norm,
                              float* norm_coef, hdiff_stream_t stream);
int hdiff_adamw_step(const hdiff_opt_tensor* table, const int* chunks, int nchunks, const float* norm_coef, double lr, double beta1,
                     double beta2, double eps, double weight_decay, int64_t step, hdiff_stream_t stream);
/* The exponential moving average of the weights that a diffusion run samples from, over a LIST of tensors in one launch:
 *   avg = avg + (p - avg) * w,  w = (float)(1.0 - decay)
 * in fp32, as three separately rounded operations (no contraction).  `table` (device) holds one entry per tensor, `chunks` (device) is cut
 * as for hdiff_adamw_step: 2 ints per chunk (tensor index, chunk index inside the tensor), hdiff_opt_chunk() elements each, both built once
 * by the host (hdiff_amd.optim.EMA).  Pointers need 4-byte alignment only; avg and p of one entry must not overlap.  decay in [0, 1];
 * decay == 1 leaves avg bit for bit (nothing is launched).  No atomics, no reduction, no synchronisation, no allocation: legal under
 * stream capture.  An addition to ABI 6. */
typedef struct { float* avg; const float* p; long long n; } hdiff_ema_tensor;
int hdiff_ema_update(const hdiff_ema_tensor* table, const int* chunks, int nchunks, double decay, hdiff_stream_t stream);
/* nn.Dropout (train mode, ModelCondition.py:185) in its unfused form: keep-mask scaled by 1/keep from the Philox stream, and out = a*b
 * (the training path uses the keep bits below; these two remain for callers that want the tensors) */
int hdiff_dropout_mask(float* out, int64_t n, float keep, uint64_t seed, uint64_t offset, hdiff_stream_t stream);
int hdiff_mul(const float* a, const float* b, float* out, int64_t n, hdiff_stream_t stream);
/* The keep decisions of hdiff_dropout_mask(out, n, keep, seed, offset) as one bit each: bit (i & 31) of bits[i >> 5] is 1 exactly
 * where that call writes a non-zero value for element i (same Philox stream, same compare); ceil(n / 32) words, unused bits
 * of the last word are 0.  What the fused dropout entries (hdiff_conv2d_fwd_dropout, hdiff_conv2d_wgrad_dropout,
 * hdiff_gn_swish_dropout_bwd) read, and all that a training step keeps of a dropout.  n > 0, keep in (0, 1]. */
int hdiff_dropout_keep_bits(uint32_t* bits, int64_t n, float keep, uint64_t seed, uint64_t offset, hdiff_stream_t stream);
/* standard-normal fill with the same Philox stream (used for in-graph noise and for tests of the generator) */
int hdiff_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * One batch of image pairs gathered from a device-resident uint8 cache, with one geometric transform per pair (csrc/batch_assemble.hip;
 * tests/_augment_def.py is the definition, matched bit for bit; hdiff_amd/device_data.py is the caller).  a, b: [N][3][H][W] (b may
 * equal a), idx: B int64 sample indices on the device, each in [0, N) -- NOT checked on the device; out_a, out_b: [B][3][H][W].
 * Sample i at `epoch` draws A = philox4x32_10(seed, i, 2 epoch) and R = philox4x32_10(seed, i, 2 epoch + 1) (the generator of
 * hdiff_randn: key = the halves of seed, counter = the two 64-bit words).  An event happens iff its word is < its threshold, a
 * probability scaled to [0, 2^32]: hflip A[0] < th_hflip, vflip A[1] < th_vflip, cropped A[3] < th_crop; k = A[2] >> 30 quarter turns if
 * rot90.  A crop box has height ch = crop_lo_h + ((R[0] (H - crop_lo_h + 1)) >> 32), width cw = clamp((2 ch W + H) / (2 H), 1, W), origin
 * y0 = (R[1] (H - ch + 1)) >> 32, x0 = (R[2] (W - cw + 1)) >> 32, and is magnified back to H x W bilinearly with half-pixel centres in
 * integer arithmetic (taps clamped to the box, round half up).  Output = rot90(vflip(hflip(resize(box))), k), the same for all three
 * channels and both images.  With all thresholds 0 and rot90 = 0 the output is a[idx], b[idx] byte for byte.
 * Refused: null pointers; B < 1; N < 1; H or W outside [1, 4096]; a threshold above 2^32; crop_lo_h outside [1, H]; rot90 with H != W;
 * epoch >= 2^31.  One launch, no atomics, no scratch, no allocation, no synchronisation: legal under stream capture; the bytes of
 * sample j depend on (a, b, idx[j], seed, epoch, settings) alone.  An addition to ABI 6.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_batch_assemble(const uint8_t* a, const uint8_t* b, const int64_t* idx, int B, int64_t N, int H, int W, uint64_t seed,
                         uint32_t epoch, uint64_t th_hflip, uint64_t th_vflip, int rot90, uint64_t th_crop, int crop_lo_h,
                         uint8_t* out_a, uint8_t* out_b, hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Synthetic degradation: the degraded input of a pair drawn from its clean target on the device (csrc/synth_degrade.hip;
 * tests/_synth_def.py is the definition; hdiff_amd/synth.py is the caller).  Two launches per batch.
 *
 * hdiff_synth_params fills table [B][HDIFF_SYNTH_PARAMS] (double, the columns below) and zseeds [B].  Sample i = idx[j] at `epoch`
 * reads w_k = philox4x32_10(seed, i, 2^32 + 8 epoch + k), k < 8 -- counters hdiff_batch_assemble (2 epoch, 2 epoch + 1 < 2^32) never
 * uses.  A uniform draw is u(r) = (r + 0.5) 2^-32, a range draw lo + (hi - lo) u(r) in three separately rounded double operations, a
 * switch is r < threshold (a probability scaled to [0, 2^32]), a choice among n is (r n) >> 32:
 *   selected w0[0] < th_select, medium w0[1] < th_medium, exposure w0[2] < th_exposure, noise w0[3] < th_noise;
 *   n_types > 0: type = (w1[0] n_types) >> 32, beta_c = type_beta[type][c]; else type = -1, beta_c = beta(w1[1]) for all c;
 *   veil_c = clamp01(airlight(w1[2]) + veil[c](w2[c]));  d_lo, d_hi = min, max of depth(w1[3]), depth(w2[3]);
 *   m = field_mean(w3[0]), gx = field_grad(w3[1]), gy = field_grad(w3[2]), gamma = gamma(w3[3]);
 *   a_k = field_amp(w4[k]), gain = gain(w4[3]);  fx_k = w5[k] >> 30, shot = shot(w5[3]);  fy_k = w6[k] >> 30, read = read(w6[3]);
 *   phi_k = 0 + (2 pi - 0) u(w7[k]), 2 pi = 6.283185307179586.
 * A stage that is switched off leaves beta_c = 0, (gamma, gain) = (1, 1), (shot, read) = (0, 0) in the table.  zseeds[j] =
 * mix(mix(mix(mix(0x73796E74685F7A31) ^ seed) ^ i) ^ epoch), mix the splitmix64 step.  The table equals the definition bit for bit.
 * Refused: null pointers; B < 1; a threshold above 2^32; epoch >= 2^31; n_types outside [0, HDIFF_SYNTH_MAX_TYPES]; a range that is not
 * finite with lo <= hi; a negative beta, depth, gain, shot or read; gamma <= 0.
 *
 * hdiff_synth_apply overwrites inp[j] ([B][3][H][W] uint8) for every sample whose `selected` column is 1 and leaves the others as they
 * are.  Per pixel (x, y) and channel c, in double, in this order:
 *   J = label / 255, u = (x + 0.5) / W, v = (y + 0.5) / H
 *   s = clamp01(((m + gx (u - 0.5)) + gy (v - 0.5)) + sum_k a_k cos(2 pi (fx_k u + fy_k v) + phi_k)),  d = d_lo + (d_hi - d_lo) s
 *   T = exp(-(beta_c d)), I = J T + veil_c (1 - T);   I = gain pow(I, gamma) (no pow when gamma == 1);
 *   I = I + sqrt(max(shot I, 0) + read^2) z;   byte = floor(255 clamp01(I) + 0.5)
 * with z element (c H + y) W + x of the row hdiff_randn_rows gives for zseeds[j] at offset HDIFF_SYNTH_Z_OFFSET (the same fp32 bits,
 * widened).  Refused: null pointers; B < 1; H or W outside [1, 4096].  No atomics, no scratch, no allocation, no synchronisation: both
 * entries are legal under stream capture; the bytes of sample j depend on (label[j], idx[j], seed, epoch, settings) alone.
 * Additions to ABI 6.
 * ------------------------------------------------------------------------------------------------------------------ */
#define HDIFF_SYNTH_MAX_TYPES 16
#define HDIFF_SYNTH_Z_OFFSET (1ull << 33)
enum {
  HDIFF_SYNTH_SELECTED = 0, HDIFF_SYNTH_TYPE = 1, HDIFF_SYNTH_M = 2, HDIFF_SYNTH_GX = 3, HDIFF_SYNTH_GY = 4, HDIFF_SYNTH_AMP = 5,
  HDIFF_SYNTH_FX = 8, HDIFF_SYNTH_FY = 11, HDIFF_SYNTH_PHI = 14, HDIFF_SYNTH_D_LO = 17, HDIFF_SYNTH_D_HI = 18, HDIFF_SYNTH_BETA = 19,
  HDIFF_SYNTH_VEIL = 22, HDIFF_SYNTH_GAMMA = 25, HDIFF_SYNTH_GAIN = 26, HDIFF_SYNTH_SHOT = 27, HDIFF_SYNTH_READ = 28,
  HDIFF_SYNTH_PARAMS = 29
};
typedef struct {
  int n_types;                                        /* 0: beta is drawn from `beta`, one value for the three channels */
  double type_beta[HDIFF_SYNTH_MAX_TYPES][3];         /* attenuation per metre of each water type: -ln N(red, green, blue) */
  double beta[2], airlight[2], veil[3][2], depth[2];  /* every range is {lo, hi} */
  double field_mean[2], field_grad[2], field_amp[2];
  double gamma[2], gain[2], shot[2], read[2];
} hdiff_synth_settings;
int hdiff_synth_params(const int64_t* idx, int B, uint64_t seed, uint32_t epoch, const hdiff_synth_settings* settings,
                       uint64_t th_select, uint64_t th_medium, uint64_t th_exposure, uint64_t th_noise, double* table,
                       uint64_t* zseeds, hdiff_stream_t stream);
int hdiff_synth_apply(const uint8_t* label, const double* table, const uint64_t* zseeds, int B, int H, int W, uint8_t* inp,
                      hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Classical baselines: the dark-channel prior and its variants, gray-world / shades-of-gray white balance (csrc/classical.hip;
 * tests/_classical_def.py is the definition; hdiff_amd/classical.py is the caller).  Images are float [N][3][H][W], clipped to [0, 1]
 * in fp32 as they are read (a NaN clips to 0); `invert` reads X = fp32(1 - clip(I)) in their place.  N <= 65535, H W <= 2^30.
 *
 *   hdiff_classical_point_min   out[n][y][x] = min over the channel set (channels = 3: R, G, B; 2: G, B) of X_c, or, with `airlight`
 *                               ([N][3], every entry > 0), of fp32(double(X_c) / double(A_c)).  One launch.
 *   hdiff_classical_window_min  out = the minimum of `in` ([N][H][W]) over the (2 r + 1)^2 window clipped at the border, r = patch / 2,
 *                               patch odd in [1, 63]; with affine != 0, out = fp32(1 - omega double(min)).  `in` and `out` must not
 *                               overlap.  One launch, 32 x 32 output tiles with a halo of r.
 *   hdiff_classical_airlight    `dark` [N][H][W] finite.  cut[n] = the element of ascending rank H W - n_top of dark[n] (1 <= n_top <=
 *                               H W; radix select on the fp32 key, three digits); among the pixels with dark >= cut the one with the
 *                               largest (double(X_R) + double(X_G)) + double(X_B), the lowest index at equal sums;
 *                               airlight[n][c] = max(X_c there, fp32(1 / 255)).  Nine launches; integer atomics only.
 *   hdiff_classical_recover     out_c = fp32(clamp((double(X_c) - A_c) / max(double(t), t0) + A_c, 0, 1)), t [N][H][W], t0 > 0; with
 *                               `invert`, out_c = fp32(1 - that).  One launch.
 *   hdiff_white_balance         m_c = (mean of double(X_c)^p)^(1 / p) per image and channel (fixed-order double sums; no pow at p = 1;
 *                               the exact maximum at p = inf), g_c = ((m_0 + m_1) + m_2) / 3 / max(m_c, 1e-6) -> gains [N][3] (double),
 *                               out_c = fp32(clamp(double(X_c) g_c, 0, 1)).  p >= 1.  Three launches.
 * No float atomics, no allocation, no synchronisation: every entry is legal under stream capture, and image n of every output depends
 * on image n of the inputs alone.  Additions to ABI 6.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_classical_point_min(const float* img, int N, int H, int W, int channels, int invert, const float* airlight, float* out,
                              hdiff_stream_t stream);
int hdiff_classical_window_min(const float* in, int N, int H, int W, int patch, int affine, double omega, float* out,
                               hdiff_stream_t stream);
int hdiff_classical_airlight_workspace(int N, int H, int W, int64_t* bytes);
int hdiff_classical_airlight(const float* img, const float* dark, int N, int H, int W, int invert, int64_t n_top, float* airlight,
                             float* cut, void* scratch, hdiff_stream_t stream);
int hdiff_classical_recover(const float* img, const float* t, const float* airlight, int N, int H, int W, int invert, double t0,
                            float* out, hdiff_stream_t stream);
int hdiff_white_balance_workspace(int N, int H, int W, int64_t* bytes);
int hdiff_white_balance(const float* img, int N, int H, int W, double p, double* gains, float* out, void* scratch,
                        hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Contrast baselines: CLAHE and global histogram equalisation on 8-bit planes (csrc/contrast.hip; tests/_contrast_def.py is the
 * definition; hdiff_amd/classical.py is the caller).  Images are float [N][3][H][W], clipped to [0, 1] in fp32 as they are read (a NaN
 * clips to 0).  `lab` == 0: P = 3 planes, one per channel; `lab` != 0: P = 1 plane, CIE L* (csrc/lab.h).  N <= 65535, H W <= 2^30.
 *
 *   hdiff_contrast_quantise  q [N][P][H][W] (uint8): q_c = floor(double(X_c) 255 + 0.5), or q = clamp(floor(L 2.55 + 0.5), 0, 255).
 *                            One launch.
 *   hdiff_clahe_luts         lut [N][P][tiles_y][tiles_x][256] (uint8).  1 <= tiles <= 16, H >= tiles_y, W >= tiles_x.  The plane is
 *                            padded right and bottom to multiples of the grid by reflect-101 (read through the index map); th =
 *                            ceil(H / tiles_y), tw = ceil(W / tiles_x), area = th tw.  Per tile: h = the histogram of the padded tile;
 *                            excess = sum(max(h - clip, 0)); h = min(h, clip) + excess / 256; with r = excess % 256 > 0 and step =
 *                            256 / r, h[k step] += 1 for k < r; lut[i] = min(rint(fp32(cumsum(h)[i]) scale), 255), the product in
 *                            fp32, halves to even.  The caller passes clip (1 <= clip <= area; area clips nothing) and scale =
 *                            fp32(255) / fp32(area).  One launch, one workgroup per tile, integer LDS atomics.
 *   hdiff_equalize_luts      lut [N][P][256] (uint8), Pillow's ImageOps.equalize: with fewer than two filled bins, or step = (H W -
 *                            the last filled bin's count) / 255 == 0, the identity; otherwise lut[i] = min((step / 2 + sum(h[:i])) /
 *                            step, 255).  Two launches: per-workgroup histograms in slots of `scratch`, then their sum in index order.
 *   hdiff_contrast_apply     q' = lut[q] (tiles_y == tiles_x == 0: one table per plane), or the blend of four tables: fx = fp32(x) inv_tw
 *                            - 0.5f, x1 = floor(fx), xa = fx - x1, xa1 = 1 - xa, tiles max(x1, 0) and min(x1 + 1, tiles_x - 1), the
 *                            same in y; res = (l11 xa1 + l12 xa) ya1 + (l21 xa1 + l22 xa) ya, seven fp32 roundings; q' =
 *                            clamp(rint(res), 0, 255).  inv_th = fp32(1) / fp32(th) and inv_tw likewise come from the caller.  Then
 *                            out_c = fp32(double(q'_c) / 255), or with `lab` out = fp32(clamp(lab_to_srgb(q' / 2.55, a, b), 0, 1)), a
 *                            and b recomputed from X.  `out` must not be `img`.  One launch.
 * No float atomics, no allocation, no synchronisation: every entry is legal under stream capture, and image n of every output depends
 * on image n of the inputs alone.  Additions to ABI 6.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_contrast_quantise(const float* img, int N, int H, int W, int lab, uint8_t* q, hdiff_stream_t stream);
int hdiff_clahe_luts(const uint8_t* q, int N, int planes, int H, int W, int tiles_y, int tiles_x, int64_t clip, float scale,
                     uint8_t* lut, hdiff_stream_t stream);
int hdiff_equalize_luts_workspace(int N, int planes, int H, int W, int64_t* bytes);
int hdiff_equalize_luts(const uint8_t* q, int N, int planes, int H, int W, uint8_t* lut, void* scratch, hdiff_stream_t stream);
int hdiff_contrast_apply(const float* img, const uint8_t* q, const uint8_t* lut, int N, int H, int W, int lab, int tiles_y, int tiles_x,
                         float inv_th, float inv_tw, float* out, hdiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * hipGraph helpers: capture everything enqueued on `stream` between begin/end, replay it later.
 * ------------------------------------------------------------------------------------------------------------------ */
int hdiff_graph_begin(hdiff_stream_t stream);
int hdiff_graph_end(hdiff_stream_t stream, void** graph_exec_out);
int hdiff_graph_launch(void* graph_exec, hdiff_stream_t stream);
int hdiff_graph_destroy(void* graph_exec);

/* HIP event timing on the launch stream (bench.py's roofline leg) */
int hdiff_event_create(void** ev);
int hdiff_event_record(void* ev, hdiff_stream_t stream);
int hdiff_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
int hdiff_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* HDIFF_H_ */
