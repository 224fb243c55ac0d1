// What the builders of hypothesis rows share (rate_variants.hip, rate_spans.hip): the limits of a row, the staging array of a
// hypothesis in LDS, and the row store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int KL_VAR_MAX_T = 1024;
constexpr int KL_VAR_MAX_CTX = 8;
constexpr long long KL_VAR_MAX_ROWS = 1ll << 22;      // (rows * 256 threads stay below 2^32)
constexpr int KL_VAR_MAX_Q = KL_VAR_MAX_T + 4;        // ids of the staging array
// the longest q: left + 2 + ahead ids with an insertion, left + ahead + 1 <= T <= KL_VAR_MAX_T
static_assert(KL_VAR_MAX_T + 1 <= KL_VAR_MAX_Q, "the staging array holds the longest hypothesis");

// out[0 .. n): four consecutive positions per thread as one 16-byte store from the first 16-byte boundary on, single
// dwords in front of it and behind the last whole group
template <class F>
__device__ __forceinline__ void emit_row(int32_t* __restrict__ out, int n, F value) {
  const int lead = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) >> 2);
  if ((int)threadIdx.x < lead && (int)threadIdx.x < n) out[threadIdx.x] = value((int)threadIdx.x);
  for (int p = lead + 4 * (int)threadIdx.x; p < n; p += 4 * (int)blockDim.x) {
    if (p + 4 <= n) {
      int4 v;
      v.x = value(p);
      v.y = value(p + 1);
      v.z = value(p + 2);
      v.w = value(p + 3);
      *reinterpret_cast<int4*>(out + p) = v;
    } else {
      for (int k = 0; k < 4; ++k)
        if (p + k < n) out[p + k] = value(p + k);
    }
  }
}

}  // namespace
