// Host side of the library: error reporting, launch checks and the launchers / workspace queries that one source file offers to
// another.  No device code: what can change a kernel's instructions is in device.h (and conv_x3.h for the split-operand convolutions
// and the direct 1x1; reduce.h and radix_select.h for the score and loss kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/hdiff.h"

namespace hdiff {

void set_error(const char* fmt, ...);

#define HDIFF_CHECK_ARG(cond, ...)            \
  do {                                        \
    if (!(cond)) {                            \
      hdiff::set_error(__VA_ARGS__);          \
      return HDIFF_ERR_INVALID;               \
    }                                         \
  } while (0)

#define HDIFF_CHECK_LAUNCH(what)                                                   \
  do {                                                                             \
    hipError_t e__ = hipGetLastError();                                            \
    if (e__ != hipSuccess) {                                                       \
      hdiff::set_error("%s: %s", what, hipGetErrorString(e__));                    \
      return HDIFF_ERR_LAUNCH;                                                     \
    }                                                                              \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Workgroups of 256 threads for a grid-stride loop over n elements, per_thread of them at a time.  Two formulas are in use; they
// differ in cap and rounding and give different grids above about 2 M elements, so each launcher names the one it was measured with.
// floor(n / per_thread) rounded up to workgroups, at most 2048: small_ops.hip, and the DDPM / CFG-DDIM steps of sampler_step.hip
static inline int grid_floor_2k(int64_t n, int per_thread = 1) {
  int64_t blocks = (n / per_thread + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}
// ceil(n / (256 * per_thread)), at most 8192: model_b_ops.hip, train_b_ops.hip and every other kernel of sampler_step.hip
static inline int grid_ceil_8k(int64_t n, int per_thread = 1) {
  int64_t blocks = (n + (int64_t)256 * per_thread - 1) / ((int64_t)256 * per_thread);
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// ceil(n / per_block) workgroups, each leaving one partial sum, between 1 and cap: the grids of the score and loss reductions.  They
// are functions of the per-image (or per-call) element count alone, which is what makes a result independent of the batch.
static inline int parts_for(int64_t n, int64_t per_block, int cap) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b > cap) b = cap;
  return b < 1 ? 1 : (int)b;
}

static inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// Cuts a caller's workspace into regions that each start on a 256-byte boundary, in the order of the take() calls.  Over a null base it
// only measures (every take() returns null): a workspace query and its launcher run the same layout function.
struct Carver {
  char* base;
  int64_t end = 0;                                              // bytes up to the end of the last region
  explicit Carver(void* p) : base((char*)p) {}
  template <class T>
  T* take(int64_t count) {
    const int64_t at = align256(end);
    end = at + count * (int64_t)sizeof(T);
    return base ? (T*)(base + at) : nullptr;
  }
  int64_t total() const { return align256(end); }               // the workspace size: the last region padded like the others
};

// the image sizes the per-image score kernels take: images on blockIdx.z, pixel indices of one plane in 32 bits
static inline int check_sizes(const char* who, int N, int H, int W, int min_side) {
  HDIFF_CHECK_ARG(N >= 1 && N <= 65535, "%s: N = %d; between 1 and 65535 images", who, N);
  HDIFF_CHECK_ARG(H >= min_side && W >= min_side, "%s: H = %d, W = %d; both sides must be at least %d", who, H, W, min_side);
  HDIFF_CHECK_ARG((int64_t)H * W <= (1ll << 30), "%s: H * W = %lld is too large; at most 2^30 pixels", who, (long long)H * W);
  return HDIFF_OK;
}

// hipFuncSetAttribute is per DEVICE: true the first time the calling site (one `static uint64_t` mask each) runs with the
// current device, so that a process using several GPUs raises the dynamic-LDS limit on each of them.
static inline bool first_use_on_device(uint64_t& mask) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
  const uint64_t bit = 1ull << dev;
  if (mask & bit) return false;
  mask |= bit;
  return true;
}

// conv_wgrad3x3.hip: the 3x3 / stride-1 weight-gradient kernel of the U-Net body (dispatched from conv_wgrad.hip)
bool wgrad3x3_applicable(const hdiff_conv_wgrad_desc* d);
int wgrad3x3_nsplit(const hdiff_conv_wgrad_desc* d);
int launch_wgrad3x3(const hdiff_conv_wgrad_desc* d, float* dwp, int nsplit, hipStream_t stream, const unsigned* keep_bits = nullptr,
                    float inv_keep = 1.0f);      // keep_bits: the dropout form (hdiff_conv2d_wgrad_dropout)
bool wgrad1x1_applicable(const hdiff_conv_wgrad_desc* d);     // same file: the 1x1 / stride-1 convs without a prologue
int wgrad1x1_nsplit(const hdiff_conv_wgrad_desc* d);
int launch_wgrad1x1(const hdiff_conv_wgrad_desc* d, float* dwp, int nsplit, hipStream_t stream);

int contraction_mode();   // HDIFF_CONTRACT_*
// the split-operand family is on (bf16x3, and f16, which is bf16x3 everywhere but in one attention-forward dispatch)
inline bool split_operands_on() { return contraction_mode() != HDIFF_CONTRACT_F32; }

// The head dims the attention kernels are instantiated for, and f(std::integral_constant<int, D>) for one of them
static inline bool mha_head_dim_ok(int D) { return D == 4 || D == 8 || D == 12 || D == 16 || D == 24 || D == 32 || D == 48 || D == 64; }
template <class F>
static inline void with_head_dim(int D, F&& f) {
  switch (D) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 24: return f(std::integral_constant<int, 24>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 48: return f(std::integral_constant<int, 48>{});
    case 64: return f(std::integral_constant<int, 64>{});
  }
}

// Attention backward: the key blocks of a (sample, head) pair cut into `want` ranges at most: blocks per range, and ranges (none empty)
struct KeyRanges { int per, nsplit; };
static inline KeyRanges key_ranges(int nkb_total, int want) {
  if (want > nkb_total) want = nkb_total;
  if (want < 1) want = 1;
  const int per = cdiv(nkb_total, want);
  return {per, cdiv(nkb_total, per)};
}
// attention_bwd_h2.hip: the attention backward at d_head 16 / 32 in the split-operand mode.  mha_bwd_route (attention_bwd.hip) decides
// whether it runs; nothing here looks at the contraction mode.
long long mha_bwd_slab_cap_bytes();                          // upper bound on the dQ partial slabs (HDIFF_BWD_SLAB_GIB)
bool mha_bwd_x3_shape_ok(int B, int C, int heads, int L);     // the shapes it covers
KeyRanges mha_bwd_h2_key_ranges(int B, int heads, int L, int D);
int64_t mha_bwd_x3_workspace_floats(int B, int C, int heads, int L);   // dQ slabs + piece tensors + maxima
bool mha_bwd_h2_lds_granted();                                // asks the current device for the kernels' LDS size (once per device)
void launch_mha_bwd_h2(const float* qkv, const float* d_o, const float* lse2, const float* delta, float* dqkv, float* ws, int B,
                       int C, int heads, int L, KeyRanges g, hipStream_t stream);
// Attention forward in the split-operand mode.  attention_x3p.hip: d_head 32 on operands split ONCE into a workspace (fp16 pairs;
// 0 bytes = shape not covered); attention_h2.hip: d_head 16 likewise, and the split passes of both; attention_x3.hip: the kernel that
// splits in its loop (bf16 triples), for calls without a workspace; attention_f16.hip: the inference forward of the f16 mode, every
// operand ONE fp16 piece, inside the same workspace.  mha_fwd_route (attention.hip) decides which one runs: the launchers check
// nothing, each names its precondition where it is defined.
int64_t mha_fwd_x3p_workspace(int B, int C, int heads, int L);
int64_t mha_fwd_h2_tail_bytes(int B, int C);      // bytes behind the pairs of the workspace (Q / K row maxima)
void launch_mha_fwd_x3p(const float* qkv, float* o, float* lse2, int B, int C, int heads, int L, float qscale, void* ws, hipStream_t stream);
void launch_mha_fwd_h2(const float* qkv, float* o, float* lse2, int B, int C, int heads, int L, float qscale, void* ws, int nq,
                       hipStream_t stream);      // nq: 4 or 6 query tiles per wave (256 / 384 queries per workgroup)
void launch_qk_split_h2(const float* qkv, void* ws, int B, int C, int heads, int L, float qscale, hipStream_t stream);   // Q, K as fp16 score operands
void launch_v_split_h2(const float* qkv, void* ws, int B, int C, int heads, int L, hipStream_t stream);                  // V as fp16 pairs, d_head 16 / 32
void launch_mha_fwd_x3(const float* qkv, float* o, float* lse2, int B, int C, int heads, int L, float qscale, hipStream_t stream);
void launch_mha_fwd_f16(const float* qkv, float* o, int B, int C, int heads, int L, float qscale, void* ws, hipStream_t stream);

}  // namespace hdiff
