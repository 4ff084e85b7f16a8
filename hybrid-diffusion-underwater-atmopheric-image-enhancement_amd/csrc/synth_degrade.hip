// Synthetic degradation of a clean batch on the device (hdiff_amd/synth.py): the degraded INPUT of a training pair is drawn from its
// clean TARGET by the image-formation model -- a procedural range field, a scattering medium (underwater and haze share one formula),
// an exposure curve and sensor noise -- so that clean images alone can feed the image-conditioned tree.  tests/_synth_def.py is the
// definition both kernels are held to: the parameter table bit for bit, the bytes everywhere.
//
// hdiff_synth_params: one thread per sample.  Sample i (its index in the cache) at epoch e reads eight Philox words quadruples
// w_k = philox4x32_10(seed, i, 2^32 + 8 e + k), k < 8.  hdiff_batch_assemble uses the counters 2 e and 2 e + 1 < 2^32 under the same
// seed: the two sets never meet.  A uniform draw is u(r) = (r + 0.5) 2^-32 (exact in double), a range draw lo + (hi - lo) u(r) (three
// rounded operations, never contracted: the file is compiled with -ffp-contract=off), a choice among n is (r n) >> 32, a switch is
// r < threshold (thresholds of 2^32).  The words:
//   w0 = selected, medium on, exposure on, noise on          w4 = a_0, a_1, a_2, gain
//   w1 = water type, beta, airlight, range (first)           w5 = fx_0, fx_1, fx_2, shot
//   w2 = veil_r, veil_g, veil_b, range (second)              w6 = fy_0, fy_1, fy_2, read
//   w3 = m, gx, gy, gamma                                    w7 = phi_0, phi_1, phi_2, (unused)
// Row j of the table (kP doubles, the columns in hdiff.h) holds the EFFECTIVE values: a stage that is switched off has beta = 0,
// (gamma, gain) = (1, 1), (shot, read) = (0, 0).  The sample's noise seed, mix(mix(mix(mix(tag) ^ seed) ^ i) ^ e) with mix the
// splitmix64 step, goes to zseeds[j].
//
// hdiff_synth_apply: a streaming pass, kVec consecutive x of one row per thread, the three channels together (the range field is
// computed once per pixel).  Per pixel in double, in this order:
//   J = label / 255, u = (x + 0.5) / W, v = (y + 0.5) / H
//   s = clamp01(((m + gx (u - 0.5)) + gy (v - 0.5)) + a_0 cos(2 pi (fx_0 u + fy_0 v) + phi_0) + a_1 ... + a_2 ...),  d = d_lo + (d_hi - d_lo) s
//   T = exp(-(beta d)), I = J T + B (1 - T)                    (skipped when beta == 0: T is exactly 1 and I exactly J)
//   I = gain * pow(I, gamma)                                   (no pow when gamma == 1)
//   I = I + sqrt(max(shot I, 0) + read read) z                 (skipped when shot == read == 0)
//   byte = floor(255 clamp01(I) + 0.5)
// z is element (c H + y) W + x of hdiff_randn_rows' row for zseeds[j] at offset kZOffset, the same fp32 bits widened to double.
// Samples whose `selected` column is 0 are not touched: inp keeps what it held.  No atomics, no LDS, no scratch, no allocation, no
// synchronisation: both launches are legal under stream capture, and the bytes of sample j depend on (label[j], idx[j], seed, epoch,
// settings) alone.
#include "common.h"
#include "philox.h"

using namespace hdiff;

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;
constexpr int kMaxSide = 4096;
constexpr int kP = HDIFF_SYNTH_PARAMS;
constexpr uint64_t kCounterBase = 1ull << 32;
constexpr uint64_t kZOffset = HDIFF_SYNTH_Z_OFFSET;
constexpr uint64_t kSeedTag = 0x73796E74685F7A31ull;      // "synth_z1"
constexpr double kTwoPi = 6.283185307179586;

struct ParamsArgs {
  const int64_t* idx;
  double* table;
  uint64_t* zseeds;
  int B;
  uint64_t seed;
  uint32_t epoch;
  uint64_t th_select, th_medium, th_exposure, th_noise;
  hdiff_synth_settings S;
};

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double uniform(uint32_t r) { return ((double)r + 0.5) * (1.0 / 4294967296.0); }

__device__ __forceinline__ double in_range(const double (&range)[2], uint32_t r) {
  const double span = range[1] - range[0];
  const double step = span * uniform(r);
  return range[0] + step;
}

__device__ __forceinline__ double clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

__global__ __launch_bounds__(kThreads) void synth_params_kernel(const ParamsArgs P) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= P.B) return;
  const uint64_t i = (uint64_t)P.idx[j];
  uint32_t w[8][4];
#pragma unroll
  for (int k = 0; k < 8; ++k) philox4x32_10(P.seed, i, kCounterBase + 8ull * P.epoch + (uint64_t)k, w[k]);
  const hdiff_synth_settings& S = P.S;
  double* row = P.table + (size_t)j * kP;

  const bool selected = w[0][0] < P.th_select, medium = w[0][1] < P.th_medium, exposure = w[0][2] < P.th_exposure,
             noise = w[0][3] < P.th_noise;
  row[HDIFF_SYNTH_SELECTED] = selected ? 1.0 : 0.0;

  int type = -1;
  double beta[3];
  if (S.n_types > 0) {
    type = (int)(((uint64_t)w[1][0] * (uint64_t)S.n_types) >> 32);
    for (int c = 0; c < 3; ++c) beta[c] = S.type_beta[type][c];
  } else {
    beta[0] = beta[1] = beta[2] = in_range(S.beta, w[1][1]);
  }
  row[HDIFF_SYNTH_TYPE] = (double)type;
  const double airlight = in_range(S.airlight, w[1][2]);
  for (int c = 0; c < 3; ++c) {
    row[HDIFF_SYNTH_BETA + c] = medium ? beta[c] : 0.0;
    row[HDIFF_SYNTH_VEIL + c] = clamp01(airlight + in_range(S.veil[c], w[2][c]));
  }
  const double d1 = in_range(S.depth, w[1][3]), d2 = in_range(S.depth, w[2][3]);
  row[HDIFF_SYNTH_D_LO] = d1 < d2 ? d1 : d2;
  row[HDIFF_SYNTH_D_HI] = d1 < d2 ? d2 : d1;

  row[HDIFF_SYNTH_M] = in_range(S.field_mean, w[3][0]);
  row[HDIFF_SYNTH_GX] = in_range(S.field_grad, w[3][1]);
  row[HDIFF_SYNTH_GY] = in_range(S.field_grad, w[3][2]);
  const double phase[2] = {0.0, kTwoPi};
  for (int k = 0; k < 3; ++k) {
    row[HDIFF_SYNTH_AMP + k] = in_range(S.field_amp, w[4][k]);
    row[HDIFF_SYNTH_FX + k] = (double)(w[5][k] >> 30);
    row[HDIFF_SYNTH_FY + k] = (double)(w[6][k] >> 30);
    row[HDIFF_SYNTH_PHI + k] = in_range(phase, w[7][k]);
  }
  row[HDIFF_SYNTH_GAMMA] = exposure ? in_range(S.gamma, w[3][3]) : 1.0;
  row[HDIFF_SYNTH_GAIN] = exposure ? in_range(S.gain, w[4][3]) : 1.0;
  row[HDIFF_SYNTH_SHOT] = noise ? in_range(S.shot, w[5][3]) : 0.0;
  row[HDIFF_SYNTH_READ] = noise ? in_range(S.read, w[6][3]) : 0.0;

  P.zseeds[j] = splitmix64(splitmix64(splitmix64(splitmix64(kSeedTag) ^ P.seed) ^ i) ^ (uint64_t)P.epoch);
}

struct ApplyArgs {
  const uint8_t* label;
  const double* table;
  const uint64_t* zseeds;
  uint8_t* inp;
  int B, H, W, groups;      // groups = ceil(W / kVec)
};

__global__ __launch_bounds__(kThreads) void synth_apply_kernel(const ApplyArgs P) {
  const int H = P.H, W = P.W;
  const int64_t HW = (int64_t)H * W;
  const int64_t total = (int64_t)P.B * H * P.groups;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
    const int xg = (int)(t % P.groups);
    const int y = (int)((t / P.groups) % H);
    const int64_t j = t / ((int64_t)P.groups * H);
    const double* row = P.table + (size_t)j * kP;
    if (row[HDIFF_SYNTH_SELECTED] == 0.0) continue;

    const double m = row[HDIFF_SYNTH_M], gx = row[HDIFF_SYNTH_GX], gy = row[HDIFF_SYNTH_GY];
    const double d_lo = row[HDIFF_SYNTH_D_LO], d_span = row[HDIFF_SYNTH_D_HI] - d_lo;
    const double gamma = row[HDIFF_SYNTH_GAMMA], gain = row[HDIFF_SYNTH_GAIN];
    const double shot = row[HDIFF_SYNTH_SHOT], read = row[HDIFF_SYNTH_READ], read2 = read * read;
    const bool noisy = shot != 0.0 || read != 0.0;
    const bool any_medium = row[HDIFF_SYNTH_BETA] != 0.0 || row[HDIFF_SYNTH_BETA + 1] != 0.0 || row[HDIFF_SYNTH_BETA + 2] != 0.0;

    const int xb = xg * kVec;
    const int nx = W - xb < kVec ? W - xb : kVec;
    const double v = ((double)y + 0.5) / (double)H;

    double d[kVec] = {0.0, 0.0, 0.0, 0.0};
    if (any_medium) {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int x = xb + (e < nx ? e : 0);      // the positions past the row's end repeat a valid one and are not stored
        const double u = ((double)x + 0.5) / (double)W;
        double acc = m + gx * (u - 0.5);
        acc = acc + gy * (v - 0.5);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double turns = row[HDIFF_SYNTH_FX + k] * u + row[HDIFF_SYNTH_FY + k] * v;
          acc = acc + row[HDIFF_SYNTH_AMP + k] * cos(kTwoPi * turns + row[HDIFF_SYNTH_PHI + k]);
        }
        d[e] = d_lo + d_span * clamp01(acc);
      }
    }

    const int64_t in_row = ((int64_t)j * 3 * H + y) * W + xb;      // the sample's planes are [3][H][W]; also the offset into inp
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* src = P.label + in_row + c * HW;
      const double beta = row[HDIFF_SYNTH_BETA + c], veil = row[HDIFF_SYNTH_VEIL + c];
      float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f, z3 = 0.0f;
      if (noisy) {
        // elements e0 .. e0 + 3 of the sample's stream sit in at most two quads
        const int64_t e0 = ((int64_t)c * H + y) * W + xb;
        const float4 qa = normal4(P.zseeds[j], (uint64_t)(e0 >> 2), kZOffset);
        if ((e0 & 3) == 0) {
          z0 = qa.x; z1 = qa.y; z2 = qa.z; z3 = qa.w;
        } else {
          const float4 qb = normal4(P.zseeds[j], (uint64_t)(e0 >> 2) + 1ull, kZOffset);
          switch ((int)(e0 & 3)) {
            case 1: z0 = qa.y; z1 = qa.z; z2 = qa.w; z3 = qb.x; break;
            case 2: z0 = qa.z; z1 = qa.w; z2 = qb.x; z3 = qb.y; break;
            default: z0 = qa.w; z1 = qb.x; z2 = qb.y; z3 = qb.z; break;
          }
        }
      }
      uint32_t word = 0u;
#pragma unroll 1      // one copy of the double exp and pow per channel: unrolled, the four interleave and spill
      for (int e = 0; e < kVec; ++e) {
        const double de = e == 0 ? d[0] : (e == 1 ? d[1] : (e == 2 ? d[2] : d[3]));
        const float ze = e == 0 ? z0 : (e == 1 ? z1 : (e == 2 ? z2 : z3));
        double I = (double)src[e < nx ? e : 0] / 255.0;
        if (beta != 0.0) {
          const double T = exp(-(beta * de));
          I = I * T + veil * (1.0 - T);
        }
        if (gamma != 1.0) I = pow(I, gamma);
        I = gain * I;
        if (noisy) {
          const double var = shot * I;
          I = I + sqrt((var > 0.0 ? var : 0.0) + read2) * (double)ze;
        }
        const uint32_t q = (uint32_t)floor(255.0 * clamp01(I) + 0.5);
        word |= q << (8 * e);
      }
      uint8_t* o = P.inp + in_row + c * HW;
      if (nx == kVec && ((uintptr_t)o & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(o) = word;
      } else {
        for (int e = 0; e < nx; ++e) o[e] = (uint8_t)(word >> (8 * e));
      }
    }
  }
}

bool ordered(const double (&r)[2]) { return r[0] <= r[1] && r[0] - r[0] == 0.0 && r[1] - r[1] == 0.0; }      // finite, lo <= hi

}  // namespace

extern "C" {

int hdiff_synth_params(const int64_t* idx, int B, uint64_t seed, uint32_t epoch, const hdiff_synth_settings* settings,
                       uint64_t th_select, uint64_t th_medium, uint64_t th_exposure, uint64_t th_noise, double* table,
                       uint64_t* zseeds, hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(idx && settings && table && zseeds, "synth_params: null pointer");
  HDIFF_CHECK_ARG(B >= 1, "synth_params: B = %d; a batch holds at least 1 sample", B);
  const uint64_t one = 1ull << 32;
  HDIFF_CHECK_ARG(th_select <= one && th_medium <= one && th_exposure <= one && th_noise <= one,
                  "synth_params: thresholds %llu, %llu, %llu, %llu; a probability is at most 2^32", (unsigned long long)th_select,
                  (unsigned long long)th_medium, (unsigned long long)th_exposure, (unsigned long long)th_noise);
  HDIFF_CHECK_ARG(epoch < (1u << 31), "synth_params: epoch = %u; below 2^31", epoch);
  const hdiff_synth_settings& S = *settings;
  HDIFF_CHECK_ARG(S.n_types >= 0 && S.n_types <= HDIFF_SYNTH_MAX_TYPES, "synth_params: n_types = %d; between 0 and %d", S.n_types,
                  HDIFF_SYNTH_MAX_TYPES);
  for (int t = 0; t < S.n_types; ++t)
    for (int c = 0; c < 3; ++c)
      HDIFF_CHECK_ARG(S.type_beta[t][c] >= 0.0 && S.type_beta[t][c] - S.type_beta[t][c] == 0.0,
                      "synth_params: beta of water type %d, channel %d is %g; finite and at least 0", t, c, S.type_beta[t][c]);
  HDIFF_CHECK_ARG(ordered(S.beta) && ordered(S.airlight) && ordered(S.veil[0]) && ordered(S.veil[1]) && ordered(S.veil[2]) &&
                      ordered(S.depth) && ordered(S.field_mean) && ordered(S.field_grad) && ordered(S.field_amp) && ordered(S.gamma) &&
                      ordered(S.gain) && ordered(S.shot) && ordered(S.read),
                  "synth_params: every range is finite with lo <= hi");
  HDIFF_CHECK_ARG(S.beta[0] >= 0.0, "synth_params: beta from %g; at least 0", S.beta[0]);
  HDIFF_CHECK_ARG(S.depth[0] >= 0.0, "synth_params: range from %g; at least 0", S.depth[0]);
  HDIFF_CHECK_ARG(S.gamma[0] > 0.0, "synth_params: gamma from %g; above 0", S.gamma[0]);
  HDIFF_CHECK_ARG(S.gain[0] >= 0.0 && S.shot[0] >= 0.0 && S.read[0] >= 0.0,
                  "synth_params: gain, shot and read from %g, %g, %g; at least 0", S.gain[0], S.shot[0], S.read[0]);
  (void)hipGetLastError();
  ParamsArgs P;
  P.idx = idx; P.table = table; P.zseeds = zseeds; P.B = B; P.seed = seed; P.epoch = epoch;
  P.th_select = th_select; P.th_medium = th_medium; P.th_exposure = th_exposure; P.th_noise = th_noise;
  P.S = S;
  hipLaunchKernelGGL(synth_params_kernel, dim3(cdiv(B, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, P);
  HDIFF_CHECK_LAUNCH("synth_params kernel");
  return HDIFF_OK;
}

int hdiff_synth_apply(const uint8_t* label, const double* table, const uint64_t* zseeds, int B, int H, int W, uint8_t* inp,
                      hdiff_stream_t stream) {
  HDIFF_CHECK_ARG(label && table && zseeds && inp, "synth_apply: null pointer");
  HDIFF_CHECK_ARG(B >= 1, "synth_apply: B = %d; a batch holds at least 1 sample", B);
  HDIFF_CHECK_ARG(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "synth_apply: H = %d, W = %d; both sides between 1 and %d", H, W,
                  kMaxSide);
  (void)hipGetLastError();
  ApplyArgs P;
  P.label = label; P.table = table; P.zseeds = zseeds; P.inp = inp;
  P.B = B; P.H = H; P.W = W; P.groups = cdiv(W, kVec);
  const int64_t total = (int64_t)B * H * P.groups;
  hipLaunchKernelGGL(synth_apply_kernel, dim3(grid_ceil_8k(total)), dim3(kThreads), 0, (hipStream_t)stream, P);
  HDIFF_CHECK_LAUNCH("synth_apply kernel");
  return HDIFF_OK;
}

}  // extern "C"
