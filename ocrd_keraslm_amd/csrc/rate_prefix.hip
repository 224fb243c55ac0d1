// A suspect's left context read once for all its variants (kl_prefix_windows, kl_state_fanout): the two pieces that cut a
// hypothesis window of kl_edit_windows into a window over the characters in front of the suspect -- one row per SUSPECT -- and a
// short window per variant that continues from the state the first one left.
//
// kl_prefix_windows: one workgroup per suspect s, one launch.  With g = sel_pos[s] inside text i (the upper-bound binary search
// of variant_windows_kernel, every thread with the same uniform addresses), the row is valid iff g - offsets[i] >= left; it
// then feeds x[g-left .. g-2] -- all of them inside the text, so inside the corpus -- and predicts nothing.  The ids come in
// as lane-consecutive dwords and are parked in LDS, the rows leave through emit_row (kl_emit_row.h): 16-byte stores between
// the first and the last 16-byte boundary of a row.  Every word of the four outputs is written by exactly one thread of one
// workgroup: no atomics, no workgroup waits for another, nothing depends on scheduling.  No model: no handle.
//
// kl_state_fanout: dst[b] = src[parent[b]], a row of zeros where parent[b] names no row of src.  One thread per 16 bytes of
// dst over a flat index (a row of depth 2 / width 512 is 512 such words, a row of 4 floats is one): a 16-byte load and a
// 16-byte store; rows of dst that share a parent read the same source row.  Bandwidth-bound, no LDS, no atomics.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_emit_row.h"

namespace {

__global__ void __launch_bounds__(256) prefix_windows_kernel(
    const int32_t* __restrict__ corpus, long long n_corpus, const long long* __restrict__ offsets, int n_texts,
    const int32_t* __restrict__ text_ctx, int n_ctx, const long long* __restrict__ sel_pos, int left, int T,
    int32_t* __restrict__ idx, int32_t* __restrict__ ctx, int32_t* __restrict__ tgt, int32_t* __restrict__ valid) {
  __shared__ int32_t s_q[KL_VAR_MAX_Q];
  __shared__ int32_t s_ctx[KL_VAR_MAX_CTX];
  const int s = blockIdx.x;
  const long long g = sel_pos[s];
  // a position at or beyond min(n_corpus, offsets[n_texts]) is in no text, or has no id
  const long long end = offsets[n_texts];
  const long long n_read = end < n_corpus ? end : n_corpus;
  bool ok = g >= 0 && g < n_read;
  int text = 0;
  if (ok) {
    // the first j in [0, n_texts] with offsets[j] > g  (g < offsets[n_texts]: j <= n_texts); the text is j - 1
    int lo = 0, hi = n_texts;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (offsets[mid] > g) hi = mid; else lo = mid + 1;
    }
    ok = lo > 0;
    if (ok) {
      text = lo - 1;
      ok = g - offsets[text] >= left;      // the whole of `left` characters stands in front of g: the shared route
    }
  }
  // x[g-left .. g-2] is fed (left - 1 <= T ids); x[g-1] is the first id of the rows that continue
  const int fed = ok ? left - 1 : 0;
  for (int t = threadIdx.x; t < fed; t += blockDim.x) {
    const long long p = g - left + t;
    s_q[t] = (p >= 0 && p < n_read) ? corpus[p] : 0;
  }
  if ((int)threadIdx.x < n_ctx) s_ctx[threadIdx.x] = ok ? text_ctx[(long long)text * n_ctx + threadIdx.x] : 0;
  __syncthreads();
  const long long at = (long long)s * T;
  emit_row(idx + at, T, [&](int t) { return t < fed ? s_q[t] : 0; });
  emit_row(tgt + at, T, [&](int) { return -1; });
  if (n_ctx > 0) {
    const int live = fed * n_ctx;      // the fed positions come first in the row: [t][c]
    emit_row(ctx + at * n_ctx, T * n_ctx, [&](int r) { return r < live ? s_ctx[r % n_ctx] : 0; });
  }
  if (threadIdx.x == 0) valid[s] = ok ? 1 : 0;
}

// word i of dst, 16 bytes each: row i / q, words i % q of it
__global__ void __launch_bounds__(256) state_fanout_kernel(const float4* __restrict__ src, int n_src,
                                                           const int32_t* __restrict__ parent, unsigned total, unsigned q,
                                                           float4* __restrict__ dst) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned b = i / q, w = i - b * q;
  const int p = parent[b];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p >= 0 && p < n_src) v = src[(size_t)p * q + w];
  dst[i] = v;
}

}  // namespace

extern "C" int kl_prefix_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts,
                                 const int32_t* text_ctx, int n_ctx, const int64_t* sel_pos, int S, int left, int T, int32_t* idx,
                                 int32_t* ctx, int32_t* tgt, int32_t* valid, void* stream) {
  if (!corpus || !offsets || !sel_pos || !idx || !tgt || !valid) return KL_ERR_ARG;
  if (S < 1 || (long long)S > KL_VAR_MAX_ROWS || n_texts < 1) return KL_ERR_ARG;
  // (T <= KL_VAR_MAX_T: the left - 1 <= T fed ids fit the staging array)
  if (left < 2 || T > KL_VAR_MAX_T || T < left - 1) return KL_ERR_ARG;
  if (n_ctx < 0 || n_ctx > KL_VAR_MAX_CTX || (n_ctx > 0 && (!text_ctx || !ctx))) return KL_ERR_ARG;
  if (n_corpus > (size_t)1 << 40) return KL_ERR_ARG;
  const void* words[] = {corpus, text_ctx, idx, ctx, tgt, valid};
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(offsets) & 7) || (reinterpret_cast<uintptr_t>(sel_pos) & 7)) return KL_ERR_ARG;
  // a thread owns four positions: as many waves as the longest row (the contexts') needs, at most four
  const int longest = T * (n_ctx > 1 ? n_ctx : 1);
  int threads = ((longest + 3) / 4 + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  hipLaunchKernelGGL(prefix_windows_kernel, dim3((unsigned)S), dim3(threads), 0, static_cast<hipStream_t>(stream), corpus,
                     (long long)n_corpus, reinterpret_cast<const long long*>(offsets), n_texts, text_ctx, n_ctx,
                     reinterpret_cast<const long long*>(sel_pos), left, T, idx, ctx, tgt, valid);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_state_fanout(const float* src, int n_src, const int32_t* parent, int rows, int row_floats, float* dst,
                               void* stream) {
  if (!src || !parent || !dst || n_src < 1 || rows < 1 || row_floats < 4 || (row_floats & 3)) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(dst) & 15) ||
      (reinterpret_cast<uintptr_t>(parent) & 3))
    return KL_ERR_ARG;
  const unsigned long long q = (unsigned)row_floats / 4u, total = q * (unsigned)rows;
  if (total > 0x7fffffffull) return KL_ERR_ARG;      // (a flat 32-bit index over the 16-byte words of dst)
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (size_t)n_src * q * 16;
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (size_t)total * 16;
  if (s0 < d1 && d0 < s1) return KL_ERR_ARG;
  hipLaunchKernelGGL(state_fanout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(src), n_src, parent, (unsigned)total, (unsigned)q,
                     reinterpret_cast<float4*>(dst));
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
