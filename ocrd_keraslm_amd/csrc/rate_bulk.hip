// Results of bulk rating in corpus order (kl_rate_scatter, kl_rate_scatter_alts, kl_rate_text_bits).
//
// Bulk rating (Rater.rate_batch, precision "bf16") keeps the ids of all texts in one device vector, as stateful training
// does, and describes a window call by the plan rows kl_assemble_windows reads.  These two kernels are the way back:
// rate_scatter puts the [B][T] target probabilities of one call where their characters stand in that vector -- the
// prediction made at corpus position start + t is about the character at start + t + 1 --, and rate_text_bits sums
// -log2(max(p, 1e-99)) (rating.py:531-576) per text over the finished vector, in f64 and in a fixed order, as rate_bits_kernel
// (rate_pick.hip) does per stream.  rate_scatter_alts is rate_scatter for the four results of a window with alternatives
// (kl_rate_window_alts_bulk).  None depends on a model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"

namespace {

constexpr int KL_SCATTER_MAX_CTX = 8;      // (the plan rows are kl_assemble_windows': 4 + n_ctx words)

// one workgroup per stream: out[start + 1 + t] = tprob[b][t] for the text positions of the row, moved as 32-bit words
__global__ void __launch_bounds__(256) rate_scatter_kernel(const uint32_t* __restrict__ tprob,
                                                           const long long* __restrict__ plan, int T, int n_ctx,
                                                           uint32_t* __restrict__ out, long long n_out) {
  const int b = blockIdx.x;
  const long long* row = plan + (long long)b * (4 + n_ctx);
  const long long start = row[0], vl = row[1];
  const int vlen = vl < 0 ? 0 : (vl > T ? T : (int)vl);
  const uint32_t* p = tprob + (long long)b * T;
  for (int t = threadIdx.x; t < vlen; t += blockDim.x) {
    const long long g = start + 1 + t;
    if (g >= 0 && g < n_out) out[g] = p[t];
  }
}

// one workgroup per stream, all four results of a call: the [B][T] planes as rate_scatter_kernel moves them, the [B][T][K]
// planes element by element -- K words per position, and consecutive positions of a row are consecutive in the corpus, so that
// a row's words stay contiguous on both sides
__global__ void __launch_bounds__(256) rate_scatter_alts_kernel(const uint32_t* __restrict__ tprob,
                                                                const uint32_t* __restrict__ rank,
                                                                const uint32_t* __restrict__ alt_id,
                                                                const uint32_t* __restrict__ alt_p,
                                                                const long long* __restrict__ plan, int T, int K, int n_ctx,
                                                                uint32_t* __restrict__ out_prob, uint32_t* __restrict__ out_rank,
                                                                uint32_t* __restrict__ out_alt_id,
                                                                uint32_t* __restrict__ out_alt_p, long long n_out) {
  const int b = blockIdx.x;
  const long long* row = plan + (long long)b * (4 + n_ctx);
  const long long start = row[0], vl = row[1];
  const int vlen = vl < 0 ? 0 : (vl > T ? T : (int)vl);
  const long long at = (long long)b * T;
  for (int t = threadIdx.x; t < vlen; t += blockDim.x) {
    const long long g = start + 1 + t;
    if (g >= 0 && g < n_out) {
      out_prob[g] = tprob[at + t];
      out_rank[g] = rank[at + t];
    }
  }
  for (int e = threadIdx.x; e < vlen * K; e += blockDim.x) {
    const int t = e / K;
    const long long g = start + 1 + t;
    if (g >= 0 && g < n_out) {
      const long long to = g * K + (e - t * K);
      out_alt_id[to] = alt_id[at * K + e];
      out_alt_p[to] = alt_p[at * K + e];
    }
  }
}

// one wave per text: lane j adds the positions first + j, first + j + 64, ... in index order (first = the text's second
// character), then the 64 partial sums are folded in a fixed butterfly
__global__ void __launch_bounds__(256) rate_text_bits_kernel(const float* __restrict__ probs,
                                                             const long long* __restrict__ offsets, int n_texts,
                                                             double* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= n_texts) return;
  const long long first = offsets[i] + 1, end = offsets[i + 1];
  double acc = 0.0;
  for (long long j = first + lane; j < end; j += 64) acc -= log2(fmax((double)probs[j], 1e-99));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) bits[i] = acc;
}

}  // namespace

extern "C" int kl_rate_scatter(const float* tprob, const int64_t* plan, int B, int T, int n_ctx, float* out, size_t n_out,
                               void* stream) {
  if (!tprob || !plan || !out || B < 1 || T < 1) return KL_ERR_ARG;
  if (n_ctx < 0 || n_ctx > KL_SCATTER_MAX_CTX || n_out > (size_t)1 << 40) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(tprob) & 3) || (reinterpret_cast<uintptr_t>(plan) & 7) ||
      (reinterpret_cast<uintptr_t>(out) & 3))
    return KL_ERR_ARG;
  int threads = (T + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  hipLaunchKernelGGL(rate_scatter_kernel, dim3(B), dim3(threads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint32_t*>(tprob), reinterpret_cast<const long long*>(plan), T, n_ctx,
                     reinterpret_cast<uint32_t*>(out), (long long)n_out);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_rate_scatter_alts(const float* tprob, const int32_t* rank, const int32_t* alt_id, const float* alt_p,
                                    const int64_t* plan, int B, int T, int K, int n_ctx, float* out_prob, int32_t* out_rank,
                                    int32_t* out_alt_id, float* out_alt_p, size_t n_out, void* stream) {
  if (!tprob || !rank || !alt_id || !alt_p || !plan || !out_prob || !out_rank || !out_alt_id || !out_alt_p) return KL_ERR_ARG;
  if (B < 1 || T < 1 || K < 1 || K > KL_RATE_ALTS_MAX) return KL_ERR_ARG;
  if (n_ctx < 0 || n_ctx > KL_SCATTER_MAX_CTX || n_out > (size_t)1 << 40) return KL_ERR_ARG;
  const void* words[] = {tprob, rank, alt_id, alt_p, out_prob, out_rank, out_alt_id, out_alt_p};
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return KL_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(plan) & 7) return KL_ERR_ARG;
  long long threads = ((long long)T * K + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  hipLaunchKernelGGL(rate_scatter_alts_kernel, dim3(B), dim3((unsigned)threads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint32_t*>(tprob), reinterpret_cast<const uint32_t*>(rank),
                     reinterpret_cast<const uint32_t*>(alt_id), reinterpret_cast<const uint32_t*>(alt_p),
                     reinterpret_cast<const long long*>(plan), T, K, n_ctx, reinterpret_cast<uint32_t*>(out_prob),
                     reinterpret_cast<uint32_t*>(out_rank), reinterpret_cast<uint32_t*>(out_alt_id),
                     reinterpret_cast<uint32_t*>(out_alt_p), (long long)n_out);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_rate_text_bits(const float* probs, const int64_t* offsets, int n_texts, double* bits, void* stream) {
  if (!probs || !offsets || !bits || n_texts < 1) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(probs) & 3) || (reinterpret_cast<uintptr_t>(offsets) & 7) ||
      (reinterpret_cast<uintptr_t>(bits) & 7))
    return KL_ERR_ARG;
  hipLaunchKernelGGL(rate_text_bits_kernel, dim3((n_texts + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), probs,
                     reinterpret_cast<const long long*>(offsets), n_texts, bits);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
