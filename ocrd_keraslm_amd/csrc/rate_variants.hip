// Hypothesis windows of suspect characters (kl_variant_windows, kl_edit_windows): for every selected position (what
// kl_rate_select wrote) and every variant of it -- the character as written, each of the K alternatives in its place,
// optionally the character dropped, optionally each alternative inserted in front of it -- one row of the three arrays a
// window call reads, so that the text that FOLLOWS the suspect is rated under each variant.
//
// One workgroup per row b = s * R + v (R = K + 1 + deletions + K * insertions), one launch.  With g = sel_pos[s] inside text i
// (text_of), L = min(left, g - offsets[i]) and A = min(ahead, offsets[i + 1] - 1 - g), the hypothesis q is L characters of left
// context, the variant's character if it has one, and the A characters after g; the row feeds q[0 .. len-2] and targets
// q[L .. len-1] (see keraslm_hip.h for the rule per word).  An inserted alternative sits in front of the written character: q
// is one id longer, and T >= left + ahead + 1 is required.  q (at most left + 1 + insertions + ahead <= T + 1 ids) comes in as
// lane-consecutive dwords and is parked in LDS; the row leaves through emit_hypothesis (kl_emit_row.h, where the corpus view,
// the text search and the cut of L and A live too), an invalid one as a dummy stream.  Only the positions g - L .. g + A of
// the corpus are read, through the view.  Every output word is written by exactly one thread (who writes what: see
// emit_hypothesis).  No atomics, no workgroup waits for another, nothing depends on scheduling.  No model: no handle.
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
  const CorpusView x(corpus, n_corpus, offsets, n_texts);
  const int text = (g >= 0 && g < x.n_read) ? text_of(offsets, n_texts, g) : -1;
  int L = 0, A = 0;
  if (text >= 0) cut_contexts(g - offsets[text], offsets[text + 1] - 1 - g, left, ahead, L, A);
  bool ok = L >= 1;
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
      ok = alt >= 0 && alt != x.read(g);
    }
  }
  // q: L characters in front of g, the variant's character(s), the A characters behind g -- len = L + 0 / 1 / 2 + A
  const int len = ok ? L + (dropped ? 0 : inserted ? 2 : 1) + A : 0;
  // from t = L on the corpus is read one ahead (the character dropped) or one behind (one inserted in front of it)
  const int skip = dropped ? 1 : inserted ? -1 : 0;
  for (int t = threadIdx.x; t < len; t += blockDim.x) {
    int32_t id = x.read(g - L + t + (t >= L ? skip : 0));
    if (t == L && !written && !dropped) id = alt;
    s_q[t] = id;
  }
  // q[0 .. len-2] is fed, q[L .. len-1] is predicted
  emit_hypothesis(ok, text, len > 0 ? len - 1 : 0, L - 1, s_q, s_ctx, text_ctx, n_ctx, T, idx, ctx, tgt, valid);
}

}  // namespace

extern "C" int kl_edit_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts,
                               const int32_t* text_ctx, int n_ctx, const int64_t* sel_pos, const int32_t* sel_alt_id, int S, int K,
                               int left, int ahead, int deletions, int insertions, int T, int32_t* idx, int32_t* ctx, int32_t* tgt,
                               int32_t* valid, void* stream) {
  if (!corpus || !offsets || !sel_pos || !sel_alt_id || !idx || !tgt || !valid) return KL_ERR_ARG;
  if (S < 1 || n_texts < 1 || K < 1 || K > KL_RATE_ALTS_MAX) return KL_ERR_ARG;
  if (left < 1 || ahead < 0 || deletions < 0 || deletions > 1 || insertions < 0 || insertions > 1) return KL_ERR_ARG;
  // (with T <= KL_VAR_MAX_T: q, at most left + ahead + 1 + insertions <= T + 1 ids, fits the staging array)
  if ((long long)T < (long long)left + ahead + insertions) return KL_ERR_ARG;
  const int R = K + 1 + deletions + K * insertions;
  if ((long long)S * R > KL_VAR_MAX_ROWS) return KL_ERR_ARG;
  if (!hypothesis_args_ok(n_ctx, text_ctx, ctx, n_corpus, T, {corpus, text_ctx, sel_alt_id, idx, ctx, tgt, valid},
                          {offsets, sel_pos}))
    return KL_ERR_ARG;
  hipLaunchKernelGGL(variant_windows_kernel, dim3((unsigned)(S * R)), dim3(hypothesis_threads(T, n_ctx)), 0,
                     static_cast<hipStream_t>(stream), corpus, (long long)n_corpus, reinterpret_cast<const long long*>(offsets),
                     n_texts, text_ctx, n_ctx, reinterpret_cast<const long long*>(sel_pos), sel_alt_id, K, deletions, R, left,
                     ahead, T, idx, ctx, tgt, valid);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_variant_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts,
                                  const int32_t* text_ctx, int n_ctx, const int64_t* sel_pos, const int32_t* sel_alt_id, int S,
                                  int K, int left, int ahead, int deletions, int T, int32_t* idx, int32_t* ctx, int32_t* tgt,
                                  int32_t* valid, void* stream) {
  return kl_edit_windows(corpus, n_corpus, offsets, n_texts, text_ctx, n_ctx, sel_pos, sel_alt_id, S, K, left, ahead, deletions, 0,
                         T, idx, ctx, tgt, valid, stream);
}
