// Kernel arguments of the convolutions that live outside their dispatcher's file (conv_igemm.hip): the split-operand kernels
// (conv3x3_x3.hip, conv1x1_x3.hip) and the direct 1x1 (conv1x1_direct.hip).  Each struct is defined here ONCE and passed by value
// to a kernel; the header is included by those four files only: a new field changes these kernels and no others.
#pragma once
#include <hip/hip_runtime.h>

namespace hdiff {

// the taps of a conv3x3_x3.hip launch: an ndy x ndx rectangle (3x3, 3x2, 2x3 or 2x2) of offsets (dy_min + dyi, dx_min + dxi) inside
// [-1, 1]^2; the kernel walks it column by column.  Filled by conv_tap_rect, never by hand.
struct ConvTapRect {
  int ntaps;                       // ndy * ndx: 9, 6 or 4
  int ndy, ndx, dy_min, dx_min;
  int tap_idx[9];                  // [dyi * ndx + dxi]: which tap of the packed weights that offset is (used for the weight address only)
};
// conv3x3_x3.hip: split-bf16 convolution over the 3x3 neighbourhood (plain 3x3 / stride-1 convs, the four output-parity
// phases of the transposed 5x5 / stride-2 conv and the four input-parity planes of the 5x5 / stride-2 conv: every tap offset
// lies in [-1, 1]^2)
struct ConvX3K : ConvTapRect {
  const float* x0;
  const float* x1;
  int C0, C1, Cin, H, W;
  const unsigned* wp3;             // [Cin/16][ntaps][3][CoutPad][8] packed bf16 pairs
  int CoutPad, Cout;
  const float* bias;
  const float* gn_scale;
  const float* gn_shift;
  const float* addvec;
  const float* residual;
  float* out;
  int tiles_x;
  int OH, OW, out_sy, out_oy, out_sx, out_ox;     // output pixel (vy * out_sy + out_oy, vx * out_sx + out_ox) of an OH x OW plane
  // fp16-pair form (plain 3x3 behind GroupNorm + Swish): wp3 then holds [Cin/16][9][2][CoutPad][8] words of w 2^t
  const float* act_scale;          // device {2^s, 2^-s} of the staged activations (hdiff_gn_act_scale), NULL = bf16 triples
  const float* w_scale;            // the pack's tail {bits of max |w|, 2^-t, 2^t, 0} (hdiff_pack_conv_weight_h2)
  float one;                       // 1.0f, opaque to the compiler
  // train-mode dropout between the prologue and the conv (hdiff_conv2d_fwd_dropout; the DROP instantiations only): the staged value
  // is kept ? swish(..) * inv_keep : 0, bit (e & 31) of keep_bits[e >> 5] for the element's flat NCHW index e < 2^31 in x0
  const unsigned* keep_bits;
  float inv_keep;
  // per-sample output range (hdiff_conv2d_fwd_range): word b takes max(word, bits of max |out[b]| over what this launch writes)
  // by one unsigned atomicMax per wave; NULL = not wanted
  unsigned* absmax_out;
  // second source of the fp16-pair form's staging scale: word b = bits of max |x[b]| (a producer's absmax_out); with it the
  // workgroup forms 2^s itself (act_scale is then not read), wp3 is a pair pack of ntaps taps and w_scale its tail
  const unsigned* absmax_in;
  // strided input (the parity planes of a stride-2 conv): pixel (iy, ix) of the H x W grid the kernel walks is element
  // (iy * in_s + in_oy, ix * in_s + in_ox) of an IH x IW plane, zero outside it; the plain case is in_s = 1, offsets 0, IH x IW = H x W
  int in_s, in_oy, in_ox, IH, IW;
  int residual_first;              // != 0: out = (acc + residual) + (bias + addvec) instead of (acc + (bias + addvec)) + residual
};
void launch_conv3x3_x3(const ConvX3K& k, int B, hipStream_t stream);
// the tap list (dy[t], dx[t]), t = its index in the pack, as a rectangle; false (k is then unspecified) if the list is not a full 3x3, 3x2, 2x3 or
// 2x2 rectangle inside [-1, 1]^2 (the kernel has no form for it)
bool conv_tap_rect(ConvTapRect& k, int ntaps, const int* dy, const int* dx);
// taps (ky, kx) of the 5x5 kernel that read input parity plane (oy, ox) of a stride-2 conv, in the order of the plane-grouped
// pair pack (hdiff_pack_conv_weight_h2_s2); returns their number: 9, 6, 6 or 4
int s2_plane_taps(int oy, int ox, int* ky, int* kx);

// conv1x1_x3.hip: the 1x1 / stride-1 convolution on bf16 triples (no LDS; operands split in registers)
struct Conv1x1X3K {
  const float* x0;
  const float* x1;
  int C0, Cin;
  long HW;
  const unsigned* wp3;             // [Cin/16][1][3][CoutPad][8] packed bf16 pairs (hdiff_pack_conv_weight_x3_taps, one tap)
  int CoutPad, Cout;
  const float* bias;
  const float* addvec;
  const float* residual;
  float* out;
  unsigned* absmax_out;            // as ConvX3K::absmax_out
};
void launch_conv1x1_x3(const Conv1x1X3K& k, int B, hipStream_t stream);

// conv1x1_direct.hip: the 1x1 / stride-1 convolution on the fp32-input MFMA (no LDS)
struct Conv1x1K {
  const float* x0;
  const float* x1;
  int C0, Cin;
  long HW;
  const float* wp;                 // [CinPad][CoutPad] (hdiff_pack_conv_weight, one tap)
  int CoutPad, Cout;
  const float* bias;
  const float* addvec;
  const float* residual;
  float* out;
};
void launch_conv1x1_direct(const Conv1x1K& k, int B, hipStream_t stream);

}  // namespace hdiff
