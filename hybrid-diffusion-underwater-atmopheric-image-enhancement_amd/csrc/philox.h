// Philox4x32-10 counter-based generator + Box-Muller: 4 normals per counter.  Device code shared by small_ops.hip (randn, the
// dropout masks) and sampler_step.hip (the step kernels' own noise): element i of a stream is component i & 3 of counter
// (i >> 2, offset) under `seed`, whichever kernel draws it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdiff {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

__device__ __forceinline__ void philox4x32_10(uint64_t seed, uint64_t ctr_lo, uint64_t ctr_hi, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), (uint32_t)ctr_hi, (uint32_t)(ctr_hi >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

__device__ __forceinline__ float4 normal4(uint64_t seed, uint64_t ctr_lo, uint64_t ctr_hi) {
  uint32_t r[4];
  philox4x32_10(seed, ctr_lo, ctr_hi, r);
  // u in (0,1]: (r + 1) * 2^-32 ; Box-Muller on two pairs
  const float u0 = ((float)(r[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u1 = ((float)(r[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(r[2] >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u3 = ((float)(r[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
  float s0, c0, s1, c1;
  sincosf(6.283185307179586f * u1, &s0, &c0);
  sincosf(6.283185307179586f * u3, &s1, &c1);
  return make_float4(ra * c0, ra * s0, rb * c1, rb * s1);
}

}  // namespace hdiff
