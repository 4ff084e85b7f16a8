// The radix select of the score kernels: the value at a given rank of a plane of samples, found digit by digit on the order-preserving
// integer key of each sample, exact at ties.  quality.hip runs it on 32-bit keys of fp32 values (UICM's two cuts of two planes: 4 selects
// per image, 3 digits), uciqe.hip on 64-bit keys of doubles (the two cuts of L: 2 selects, 6 digits), color_diff.hip likewise (the 95th
// percentile of the CIEDE2000 plane: 1 select, 6 digits).  Beside device.h, this header, reduce.h and lab.h are the only ones that hold
// device code; no kernel of profiles/roofline_traffic.json reaches any of them.
//
// One digit is two launches of the including file's own kernels, which do its addressing and call in here:
//   histogram  every workgroup counts its samples into an LDS histogram per select -- the file's own loop: the two read different data
//              -- and merges it into the global one (select_flush): integer atomics only, so counts do not depend on arrival order;
//   scan       one workgroup per select finds the bin that holds the select's rank and narrows the select to it (select_scan).
// Selects come in pairs, 2 p the left cut of plane p and 2 p + 1 its right cut.  Before the first digit nothing tells the two apart, so
// they share ONE histogram, kept under the even select: select_hist is that rule for the scan, and each histogram loop counts its
// first digit under the even select only.
// After the last digit `prefix` is the key of the cut value, `less` the samples below it and `eq` its copies.
#pragma once
#include "device.h"

namespace hdiff {

// prefix: the digits found so far; rank: the wanted rank among the samples that share them; less: samples below them; eq: samples in
// the bin chosen last.  The workspaces hold arrays of these: the sizes are part of the layout.
template <class Key>
struct Select { Key prefix; unsigned rank, less, eq; };
static_assert(sizeof(Select<unsigned>) == 16, "the UIQM workspace is laid out for 16-byte selects");
static_assert(sizeof(Select<unsigned long long>) == 24, "the UCIQE workspace is laid out for 24-byte selects");

// order-preserving key of a finite value; -0 and +0 share a key
__device__ __forceinline__ unsigned key_of(float f) {
  if (f == 0.0f) f = 0.0f;
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long key_of(double f) {
  if (f == 0.0) f = 0.0;
  const unsigned long long u = __builtin_bit_cast(unsigned long long, f);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// a select before its first digit: rank `rank` (from 0) of the whole plane
template <class Key>
__device__ __forceinline__ Select<Key> select_start(unsigned rank) {
  Select<Key> s;
  s.prefix = 0; s.rank = rank; s.less = 0u; s.eq = 0u;
  return s;
}

// the select whose histogram select s reads in digit `pass`
__device__ __forceinline__ int select_hist(int pass, int s) { return pass == 0 ? (s & ~1) : s; }

// Adds the workgroup's LDS histogram of n bins to the global one g, after a barrier (every thread's counts have landed).
template <int THREADS>
__device__ __forceinline__ void select_flush(const unsigned* sh, unsigned* __restrict__ g, int n) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += THREADS)
    if (sh[i]) atomicAdd(&g[i], sh[i]);
}

// One workgroup of THREADS threads: h is the histogram (BINS bins, those past 2^bits zero) of the digit just counted for *sel.  Finds the
// bin that holds sel->rank; the thread that owns it writes the prefix extended by that bin, the rank within the bin, the samples below
// and inside it.
template <int THREADS, int BINS, class Key>
__device__ __forceinline__ void select_scan(const unsigned* __restrict__ h, Select<Key>* sel, int bits) {
  __shared__ unsigned cum[THREADS];
  const Select<Key> st = *sel;
  constexpr int per = BINS / THREADS;
  unsigned cnt[per], local = 0u;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    cnt[j] = h[threadIdx.x * per + j];
    local += cnt[j];
  }
  cum[threadIdx.x] = local;
  __syncthreads();
  unsigned before = 0u;
  for (int i = 0; i < (int)threadIdx.x; ++i) before += cum[i];
  if (st.rank < before || st.rank >= before + local) return;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    if (st.rank < before + cnt[j]) {
      Select<Key> o;
      o.prefix = (st.prefix << bits) | (Key)(threadIdx.x * per + j);
      o.rank = st.rank - before; o.less = st.less + before; o.eq = cnt[j];
      *sel = o;
      return;
    }
    before += cnt[j];
  }
}

}  // namespace hdiff
