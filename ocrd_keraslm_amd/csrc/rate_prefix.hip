// A suspect's left context read once for all its variants (kl_prefix_windows, kl_state_fanout): the two pieces that cut a
// hypothesis window of kl_edit_windows into a window over the characters in front of the suspect -- one row per SUSPECT -- and a
// short window per variant that continues from the state the first one left.
//
// kl_prefix_windows: one workgroup per suspect s, one launch.  With g = sel_pos[s] inside text i (text_of), the row is valid
// iff g - offsets[i] >= left; it then feeds x[g-left .. g-2] -- all of them inside the text, so inside the corpus, and the
// only positions read -- and predicts nothing.  The ids come in as lane-consecutive dwords and are parked in LDS, the row
// leaves through emit_hypothesis (kl_emit_row.h) with every fed id in q and no target behind the last.  Every output word
// is written by exactly one thread (who writes what: see emit_hypothesis).  No atomics, no workgroup waits for another,
// nothing depends on scheduling.  No model: no handle.
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
  const long long g = sel_pos[blockIdx.x];
  const CorpusView x(corpus, n_corpus, offsets, n_texts);
  const int text = (g >= 0 && g < x.n_read) ? text_of(offsets, n_texts, g) : -1;
  // the whole of `left` characters stands in front of g: the shared route
  const bool ok = text >= 0 && g - offsets[text] >= left;
  // x[g-left .. g-2] is fed (left - 1 <= T ids); x[g-1] is the first id of the rows that continue
  const int fed = ok ? left - 1 : 0;
  for (int t = threadIdx.x; t < fed; t += blockDim.x) s_q[t] = x.read(g - left + t);
  emit_hypothesis(ok, text, fed, fed, s_q, s_ctx, text_ctx, n_ctx, T, idx, ctx, tgt, valid);
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
  // (with T <= KL_VAR_MAX_T: the left - 1 <= T fed ids fit the staging array)
  if (left < 2 || T < left - 1) return KL_ERR_ARG;
  if (!hypothesis_args_ok(n_ctx, text_ctx, ctx, n_corpus, T, {corpus, text_ctx, idx, ctx, tgt, valid}, {offsets, sel_pos}))
    return KL_ERR_ARG;
  hipLaunchKernelGGL(prefix_windows_kernel, dim3((unsigned)S), dim3(hypothesis_threads(T, n_ctx)), 0,
                     static_cast<hipStream_t>(stream), corpus, (long long)n_corpus, reinterpret_cast<const long long*>(offsets),
                     n_texts, text_ctx, n_ctx, reinterpret_cast<const long long*>(sel_pos), left, T, idx, ctx, tgt, valid);
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
