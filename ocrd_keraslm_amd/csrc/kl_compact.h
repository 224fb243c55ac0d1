// The two shared steps of an ordered compaction (kl_rate_select, kl_word_bounds, kl_segment_select): every workgroup counts the
// selected among its KL_RATE_SELECT_BLOCK consecutive items, ONE workgroup turns the counts into exclusive offsets, and a third
// launch recomputes the flags and places the records.  No atomics, no workgroup waits for another.
#pragma once
#include "keraslm_hip.h"
#include "kl_common.h"

static_assert(KL_RATE_SELECT_SCAN_THREADS == 4 * KL_WAVE, "kl_counts_to_offsets folds four waves");

// lanes below this one whose bit is set in a wave's ballot
__device__ __forceinline__ int kl_lanes_before(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// counts [n_blocks] -> exclusive offsets, in place; total[0] = their sum.  The body of a kernel of ONE workgroup of
// KL_RATE_SELECT_SCAN_THREADS threads: that many blocks per round, with a running carry.
__device__ __forceinline__ void kl_counts_to_offsets(long long* __restrict__ counts, long long n_blocks,
                                                     long long* __restrict__ total) {
  __shared__ long long wave_sum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (long long b0 = 0; b0 < n_blocks; b0 += KL_RATE_SELECT_SCAN_THREADS) {
    const long long i = b0 + threadIdx.x;
    const long long v = i < n_blocks ? counts[i] : 0;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long u = __shfl_up(inc, off);
      if (lane >= off) inc += u;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const long long s = wave_sum[w];
      before += w < wave ? s : 0;
      all += s;
    }
    if (i < n_blocks) counts[i] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = carry;
}
