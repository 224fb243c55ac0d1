// Ordered selection over corpus-order rating results (kl_rate_select): the positions whose character the model does not
// believe -- rank >= min_rank and probability <= max_prob --, packed in ascending position with their records.
//
// The order must not depend on how workgroups are scheduled, and no workgroup waits for another: three plain launches.
//   1. rate_select_count_kernel: every workgroup owns KL_RATE_SELECT_BLOCK consecutive positions and writes how many of them
//      are selected (ballot and popcount per wave, the waves' counts folded through LDS);
//   2. rate_select_offsets_kernel: ONE workgroup turns the counts into exclusive offsets in place, KL_RATE_SELECT_SCAN_THREADS
//      blocks per round with a running carry, and writes the total;
//   3. rate_select_place_kernel: recomputes the flags; a selected position goes to its block's offset + the selected positions
//      of the block before it (waves of earlier rounds and lower waves of its round from LDS, lower lanes by mbcnt of the
//      round's ballot), and its record is written if that index lies below `capacity`.
// No atomics, no look-back, no spinning; 64-bit indices throughout.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_compact.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / KL_WAVE;
constexpr int SEL_ROUNDS = KL_RATE_SELECT_BLOCK / SEL_THREADS;
static_assert(SEL_ROUNDS * SEL_THREADS == KL_RATE_SELECT_BLOCK, "a block is a whole number of rounds");

// the selection rule, in f32: a NaN probability compares false
__device__ __forceinline__ bool selected(const float* __restrict__ probs, const int* __restrict__ rank, long long j, long long n,
                                         float max_prob, int min_rank) {
  return j < n && rank[j] >= min_rank && probs[j] <= max_prob;
}

__global__ void __launch_bounds__(SEL_THREADS) rate_select_count_kernel(const float* __restrict__ probs,
                                                                         const int* __restrict__ rank, long long n,
                                                                         float max_prob, int min_rank,
                                                                         long long* __restrict__ counts) {
  __shared__ int wave_n[SEL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * KL_RATE_SELECT_BLOCK;
  int c = 0;
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r)
    c += __popcll(__ballot(selected(probs, rank, base + r * SEL_THREADS + threadIdx.x, n, max_prob, min_rank)));
  if (lane == 0) wave_n[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) all += wave_n[w];
    counts[blockIdx.x] = all;
  }
}

// counts [n_blocks] -> exclusive offsets, in place; total[0] = their sum
__global__ void __launch_bounds__(KL_RATE_SELECT_SCAN_THREADS) rate_select_offsets_kernel(long long* __restrict__ counts,
                                                                                          long long n_blocks,
                                                                                          long long* __restrict__ total) {
  kl_counts_to_offsets(counts, n_blocks, total);
}

__global__ void __launch_bounds__(SEL_THREADS) rate_select_place_kernel(
    const float* __restrict__ probs, const int* __restrict__ rank, const uint32_t* __restrict__ alt_id,
    const uint32_t* __restrict__ alt_p, long long n, int K, float max_prob, int min_rank, long long capacity,
    const long long* __restrict__ offsets, long long* __restrict__ sel_pos, uint32_t* __restrict__ sel_prob,
    int* __restrict__ sel_rank, uint32_t* __restrict__ sel_alt_id, uint32_t* __restrict__ sel_alt_p) {
  __shared__ int wave_n[SEL_ROUNDS][SEL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * KL_RATE_SELECT_BLOCK;
  bool flag[SEL_ROUNDS];
  unsigned long long mask[SEL_ROUNDS];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    flag[r] = selected(probs, rank, base + r * SEL_THREADS + threadIdx.x, n, max_prob, min_rank);
    mask[r] = __ballot(flag[r]);
    if (lane == 0) wave_n[r][wave] = __popcll(mask[r]);
  }
  __syncthreads();
  long long at = offsets[blockIdx.x];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) {
      const int c = wave_n[r][w];
      before += w < wave ? c : 0;
      all += c;
    }
    const long long to = at + before + kl_lanes_before(mask[r]);
    if (flag[r] && to < capacity) {
      const long long j = base + r * SEL_THREADS + threadIdx.x;
      sel_pos[to] = j;
      sel_prob[to] = __float_as_uint(probs[j]);
      sel_rank[to] = rank[j];
      for (int k = 0; k < K; ++k) {
        sel_alt_id[to * K + k] = alt_id[j * K + k];
        sel_alt_p[to * K + k] = alt_p[j * K + k];
      }
    }
    at += all;
  }
}

inline long long select_blocks(size_t n) { return (long long)((n + KL_RATE_SELECT_BLOCK - 1) / KL_RATE_SELECT_BLOCK); }

}  // namespace

extern "C" size_t kl_rate_select_workspace_bytes(size_t n) {
  if (n < 1 || n > (size_t)1 << 40) return 0;
  return ((size_t)select_blocks(n) * sizeof(long long) + 255) / 256 * 256;
}

extern "C" int kl_rate_select(const float* probs, const int32_t* rank, const int32_t* alt_id, const float* alt_p, size_t n, int K,
                              float max_prob, int min_rank, size_t capacity, int64_t* sel_pos, float* sel_prob,
                              int32_t* sel_rank, int32_t* sel_alt_id, float* sel_alt_p, int64_t* count, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!probs || !rank || !alt_id || !alt_p || !count || !ws) return KL_ERR_ARG;
  if (n < 1 || n > (size_t)1 << 40 || capacity > (size_t)1 << 40 || K < 1 || K > KL_RATE_ALTS_MAX) return KL_ERR_ARG;
  if (min_rank < 0 || max_prob != max_prob) return KL_ERR_ARG;
  if (capacity > 0 && (!sel_pos || !sel_prob || !sel_rank || !sel_alt_id || !sel_alt_p)) return KL_ERR_ARG;
  const void* words[] = {probs, rank, alt_id, alt_p, sel_prob, sel_rank, sel_alt_id, sel_alt_p};
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(sel_pos) & 7) || (reinterpret_cast<uintptr_t>(count) & 7) ||
      (reinterpret_cast<uintptr_t>(ws) & 7))
    return KL_ERR_ARG;
  if (ws_bytes < kl_rate_select_workspace_bytes(n)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n_blocks = select_blocks(n);
  long long* counts = reinterpret_cast<long long*>(ws);
  hipLaunchKernelGGL(rate_select_count_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, s, probs, rank, (long long)n,
                     max_prob, min_rank, counts);
  hipLaunchKernelGGL(rate_select_offsets_kernel, dim3(1), dim3(KL_RATE_SELECT_SCAN_THREADS), 0, s, counts, n_blocks,
                     reinterpret_cast<long long*>(count));
  if (capacity > 0)      // (the counting call ends here: nothing to place)
    hipLaunchKernelGGL(rate_select_place_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, s, probs, rank,
                       reinterpret_cast<const uint32_t*>(alt_id), reinterpret_cast<const uint32_t*>(alt_p), (long long)n, K,
                       max_prob, min_rank, (long long)capacity, counts, reinterpret_cast<long long*>(sel_pos),
                       reinterpret_cast<uint32_t*>(sel_prob), sel_rank, reinterpret_cast<uint32_t*>(sel_alt_id),
                       reinterpret_cast<uint32_t*>(sel_alt_p));
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
