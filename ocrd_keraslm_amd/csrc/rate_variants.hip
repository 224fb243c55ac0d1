// Hypothesis windows of suspect characters (kl_variant_windows, kl_edit_windows): for every selected position (what
// kl_rate_select wrote) and every variant of it -- the character as written, each of the K alternatives in its place,
// optionally the character dropped, optionally each alternative inserted in front of it -- one row of the three arrays a
// window call reads, so that the text that FOLLOWS the suspect is rated under each variant.
//
// One workgroup per row b = s * R + v (R = K + 1 + deletions + K * insertions), one launch.  With g = sel_pos[s] inside text i
// (offsets[i] <= g < offsets[i + 1], found by an upper-bound binary search every thread walks with the same uniform
// addresses: log2(n_texts) steps, repeated offsets -- empty texts -- are skipped by it), L = min(left, g - offsets[i]) and
// A = min(ahead, offsets[i + 1] - 1 - g), the hypothesis q is L characters of left context, the variant's character if it has
// one, and the A characters after g; the row feeds q[0 .. len-2] and targets q[L .. len-1] (see keraslm_hip.h for the rule
// per word).  An inserted alternative sits in front of the written character: q is one id longer, and T >= left + ahead + 1
// is required.  q (at most left + 1 + insertions + ahead <= T + 1 ids) comes in as lane-consecutive dwords and is parked in
// LDS; every thread then owns four consecutive output positions and stores them as one 16-byte word, single dwords in front of the
// first 16-byte boundary of a row and behind its last whole group (emit_row of kl_emit_row.h, as the rows of assemble.hip).
// An invalid row leaves as a dummy stream (idx 0, ctx 0, tgt -1).  Every word of the four outputs is written by exactly one
// thread of one workgroup: no atomics, no workgroup waits for another, nothing depends on scheduling.  Corpus addresses are
// 64-bit; a position outside [0, min(n_corpus, offsets[n_texts])) reads as 0 without touching memory.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_emit_row.h"

namespace {

__global__ void __launch_bounds__(256) variant_windows_kernel(
    const int32_t* __restrict__ corpus, long long n_corpus, const long long* __restrict__ offsets, int n_texts,
    const int32_t* __restrict__ text_ctx, int n_ctx, const long long* __restrict__ sel_pos,
    const int32_t* __restrict__ sel_alt_id, int K, int deletions, int R, int left, int ahead, int T,
    int32_t* __restrict__ idx, int32_t* __restrict__ ctx, int32_t* __restrict__ tgt, int32_t* __restrict__ valid) {
  __shared__ int32_t s_q[KL_VAR_MAX_Q];
  __shared__ int32_t s_ctx[KL_VAR_MAX_CTX];
  const int b = blockIdx.x;
  const int s = b / R, v = b - s * R;
  const long long g = sel_pos[s];
  // a position at or beyond min(n_corpus, offsets[n_texts]) is in no text, or has no id
  const long long end = offsets[n_texts];
  const long long n_read = end < n_corpus ? end : n_corpus;
  bool ok = g >= 0 && g < n_read;
  int text = 0, L = 0, A = 0;
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
      const long long before = g - offsets[text], after = offsets[text + 1] - 1 - g;
      L = before < left ? (int)before : left;
      A = after < ahead ? (int)after : ahead;
      ok = L >= 1;
    }
  }
  int32_t alt = 0;
  // v: 0 written, 1 .. K substituted, K + 1 dropped (deletions), from K + 1 + deletions on inserted (R says whether)
  const bool written = v == 0, inserted = v > K + deletions, dropped = v > K && !inserted;
  if (ok && !written) {
    if (dropped) {
      ok = A > 0;
    } else if (inserted) {
      alt = sel_alt_id[(long long)s * K + (v - (K + 1 + deletions))];
      ok = alt >= 0;      // (the written character doubled is a hypothesis)
    } else {
      alt = sel_alt_id[(long long)s * K + (v - 1)];
      ok = alt >= 0 && alt != corpus[g];
    }
  }
  // q: L characters in front of g, the variant's character(s), the A characters behind g -- len = L + 0 / 1 / 2 + A
  const int len = ok ? L + (dropped ? 0 : inserted ? 2 : 1) + A : 0;
  // from t = L on the corpus is read one ahead (the character dropped) or one behind (one inserted in front of it)
  const int skip = dropped ? 1 : inserted ? -1 : 0;
  for (int t = threadIdx.x; t < len; t += blockDim.x) {
    const long long p = g - L + t + (t >= L ? skip : 0);
    int32_t id = (p >= 0 && p < n_read) ? corpus[p] : 0;
    if (t == L && !written && !dropped) id = alt;
    s_q[t] = id;
  }
  if ((int)threadIdx.x < n_ctx) s_ctx[threadIdx.x] = ok ? text_ctx[(long long)text * n_ctx + threadIdx.x] : 0;
  __syncthreads();
  const int fed = len > 0 ? len - 1 : 0;      // q[0 .. len-2] is fed, q[L .. len-1] is predicted
  const long long at = (long long)b * T;
  emit_row(idx + at, T, [&](int t) { return t < fed ? s_q[t] : 0; });
  emit_row(tgt + at, T, [&](int t) { return (t < fed && t >= L - 1) ? s_q[t + 1] : -1; });
  if (n_ctx > 0) {
    const int live = fed * n_ctx;      // the fed positions come first in the row: [t][c]
    emit_row(ctx + at * n_ctx, T * n_ctx, [&](int r) { return r < live ? s_ctx[r % n_ctx] : 0; });
  }
  if (threadIdx.x == 0) valid[b] = ok ? 1 : 0;
}

}  // namespace

extern "C" int kl_edit_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts,
                               const int32_t* text_ctx, int n_ctx, const int64_t* sel_pos, const int32_t* sel_alt_id, int S, int K,
                               int left, int ahead, int deletions, int insertions, int T, int32_t* idx, int32_t* ctx, int32_t* tgt,
                               int32_t* valid, void* stream) {
  if (!corpus || !offsets || !sel_pos || !sel_alt_id || !idx || !tgt || !valid) return KL_ERR_ARG;
  if (S < 1 || n_texts < 1 || K < 1 || K > KL_RATE_ALTS_MAX) return KL_ERR_ARG;
  if (left < 1 || ahead < 0 || deletions < 0 || deletions > 1 || insertions < 0 || insertions > 1) return KL_ERR_ARG;
  // (T <= KL_VAR_MAX_T: q, at most left + ahead + 1 + insertions <= T + 1 ids, fits the staging array)
  if (T > KL_VAR_MAX_T || (long long)T < (long long)left + ahead + insertions) return KL_ERR_ARG;
  if (n_ctx < 0 || n_ctx > KL_VAR_MAX_CTX || (n_ctx > 0 && (!text_ctx || !ctx))) return KL_ERR_ARG;
  if (n_corpus > (size_t)1 << 40) return KL_ERR_ARG;
  const int R = K + 1 + deletions + K * insertions;
  if ((long long)S * R > KL_VAR_MAX_ROWS) return KL_ERR_ARG;
  const void* words[] = {corpus, text_ctx, sel_alt_id, idx, ctx, tgt, valid};
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(offsets) & 7) || (reinterpret_cast<uintptr_t>(sel_pos) & 7)) return KL_ERR_ARG;
  // a thread owns four positions: as many waves as the longest row (the contexts') needs, at most four
  const int longest = T * (n_ctx > 1 ? n_ctx : 1);
  int threads = ((longest + 3) / 4 + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  hipLaunchKernelGGL(variant_windows_kernel, dim3((unsigned)(S * R)), dim3(threads), 0, static_cast<hipStream_t>(stream), corpus,
                     (long long)n_corpus, reinterpret_cast<const long long*>(offsets), n_texts, text_ctx, n_ctx,
                     reinterpret_cast<const long long*>(sel_pos), sel_alt_id, K, deletions, R, left, ahead, T, idx, ctx, tgt,
                     valid);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_variant_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts,
                                  const int32_t* text_ctx, int n_ctx, const int64_t* sel_pos, const int32_t* sel_alt_id, int S,
                                  int K, int left, int ahead, int deletions, int T, int32_t* idx, int32_t* ctx, int32_t* tgt,
                                  int32_t* valid, void* stream) {
  return kl_edit_windows(corpus, n_corpus, offsets, n_texts, text_ctx, n_ctx, sel_pos, sel_alt_id, S, K, left, ahead, deletions, 0,
                         T, idx, ctx, tgt, valid, stream);
}
