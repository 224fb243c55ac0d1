// Squared distance of two state vectors by ONE wave: what kl_state_dist2 computes per pair and what kl_edge_decode's history
// clustering compares -- one function, so that the two agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// every lane returns the sum (lane u takes elements u, u + 64, ...; the partial sums are folded in a fixed butterfly)
__device__ __forceinline__ float kl_wave_dist2(const float* __restrict__ pa, const float* __restrict__ pb, int W, int lane) {
  float acc = 0.f;
  for (int u = lane; u < W; u += 64) { const float q = pa[u] - pb[u]; acc += q * q; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  return acc;
}
