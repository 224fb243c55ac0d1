// What the builders of hypothesis rows share (rate_variants.hip, rate_prefix.hip, rate_spans.hip): the limits of a row, the
// corpus as they read it, the text of a position, the cut of a hypothesis' two contexts, the way a row leaves -- and, for the
// entry points, the argument checks and the size of a workgroup.  A kernel finds its position g and decides `ok`, fills the
// staging array q in LDS, and calls emit_hypothesis; where the kernels differ, they differ in the values they pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

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

// The ids a builder may read: a position at or beyond n_read = min(n_corpus, offsets[n_texts]) is in no text, or has no id.
// Addresses are 64-bit; read(p) is 0 outside [0, n_read) without touching memory.
struct CorpusView {
  const int32_t* __restrict__ ids;
  long long n_read;
  __device__ __forceinline__ CorpusView(const int32_t* __restrict__ corpus, long long n_corpus,
                                        const long long* __restrict__ offsets, int n_texts)
      : ids(corpus), n_read(offsets[n_texts] < n_corpus ? offsets[n_texts] : n_corpus) {}
  __device__ __forceinline__ int32_t read(long long p) const { return (p >= 0 && p < n_read) ? ids[p] : 0; }
};

// The text i with offsets[i] <= g < offsets[i + 1] for a g < offsets[n_texts] (the caller's word: g < n_read), -1 where g
// lies in front of the first text.  An upper-bound binary search -- the first j in [0, n_texts] with offsets[j] > g, the
// text is j - 1 -- that every thread walks with the same uniform addresses: log2(n_texts) steps, and repeated offsets
// (empty texts) are skipped by it.
__device__ __forceinline__ int text_of(const long long* __restrict__ offsets, int n_texts, long long g) {
  int lo = 0, hi = n_texts;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] > g) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

// L characters of left context and A characters of continuation, of the `before` / `after` (>= 0) that the text has
__device__ __forceinline__ void cut_contexts(long long before, long long after, int left, int ahead, int& L, int& A) {
  L = before < left ? (int)before : left;
  A = after < ahead ? (int)after : ahead;
}

// The row of workgroup blockIdx.x leaves: the caller has written q[0 .. ) into s_q without a barrier; the row feeds
// q[0 .. fed) with the contexts of `text` and targets q[t + 1] at first <= t < fed (first >= fed: no targets), behind them a
// dummy stream (idx 0, ctx 0, tgt -1) -- all of an invalid row, which comes with fed == 0.  ok, text, fed and first are
// uniform over the workgroup.  Every thread owns four consecutive output positions (emit_row); every word of the four
// outputs is written by exactly one thread.
__device__ __forceinline__ void emit_hypothesis(bool ok, int text, int fed, int first, const int32_t* s_q, int32_t* s_ctx,
                                                const int32_t* __restrict__ text_ctx, int n_ctx, int T,
                                                int32_t* __restrict__ idx, int32_t* __restrict__ ctx,
                                                int32_t* __restrict__ tgt, int32_t* __restrict__ valid) {
  if ((int)threadIdx.x < n_ctx) s_ctx[threadIdx.x] = ok ? text_ctx[(long long)text * n_ctx + threadIdx.x] : 0;
  __syncthreads();
  const long long at = (long long)blockIdx.x * T;
  emit_row(idx + at, T, [&](int t) { return t < fed ? s_q[t] : 0; });
  emit_row(tgt + at, T, [&](int t) { return (t < fed && t >= first) ? s_q[t + 1] : -1; });
  if (n_ctx > 0) {
    const int live = fed * n_ctx;      // the fed positions come first in the row: [t][c]
    emit_row(ctx + at * n_ctx, T * n_ctx, [&](int r) { return r < live ? s_ctx[r % n_ctx] : 0; });
  }
  if (threadIdx.x == 0) valid[blockIdx.x] = ok ? 1 : 0;
}

// What the three entry points check alike: the contexts, the corpus within 64-bit reach of a 2^40 limit, a row that fits the
// staging array, and the alignment of every array the kernel reads or writes as 4-byte (`words`) or 8-byte (`longs`) items.
inline bool hypothesis_args_ok(int n_ctx, const void* text_ctx, const void* ctx, size_t n_corpus, int T,
                               std::initializer_list<const void*> words, std::initializer_list<const void*> longs) {
  if (n_ctx < 0 || n_ctx > KL_VAR_MAX_CTX || (n_ctx > 0 && (!text_ctx || !ctx))) return false;
  if (n_corpus > (size_t)1 << 40 || T > KL_VAR_MAX_T) return false;
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return false;
  for (const void* p : longs)
    if (reinterpret_cast<uintptr_t>(p) & 7) return false;
  return true;
}

// a thread owns four positions: as many waves as the longest row (the contexts') needs, at most four
inline int hypothesis_threads(int T, int n_ctx) {
  const int longest = T * (n_ctx > 1 ? n_ctx : 1);
  const int threads = ((longest + 3) / 4 + 63) / 64 * 64;
  return threads < 256 ? threads : 256;
}

}  // namespace
