// Hypothesis windows of spans with caller-supplied replacements (kl_span_windows) and the choice among a span's candidates
// (kl_span_pick): the general form of rate_variants.hip.  A span s replaces D = span_len[s] written characters at corpus
// position g = span_start[s] of text i = span_text[s] by each of its candidates, id strings of any length 0 .. M in one pool
// (candidate c is pool[cand_off[c] .. cand_off[c+1]-1], span s owns candidates span_first[s] .. span_first[s+1]-1).  Rows are
// numbered over all spans, N = S + C of them: span s has rows span_first[s] + s .. span_first[s+1] + s, the first the text as
// written, then its candidates in order; a call builds rows row0 .. row0 + rows - 1.
//
// One workgroup per row, one launch.  The row's span is the last s with span_first[s] + s <= b (an upper-bound binary search
// every thread walks with the same uniform addresses, log2(S) steps; a span without candidates has one row and is found like
// any other; the span names its text, so there is no search for it).  With L = min(left, g - offsets[i]) and
// A = min(ahead, offsets[i+1] - g - D) the hypothesis q is L characters of left context, the row's string r (the written
// characters, or the candidate's ids) and the A characters behind the span; the row feeds q[0 .. len-2] and targets
// q[L .. len-1] (see keraslm_hip.h for the rule per word).  Whether a candidate holds a negative id, and whether it differs
// from what is written, is decided by the first m <= 64 threads and a workgroup-wide OR.  q (at most left + M + ahead <= T + 1
// ids) comes in as lane-consecutive dwords and is parked in LDS; the row leaves through emit_hypothesis (kl_emit_row.h, where
// the corpus view and the cut of L and A live too), an invalid one as a dummy stream.  Only the positions g - L .. g + D + A
// of the corpus are read, through the view; a candidate whose pool range is not inside the pool, and a row whose candidate
// index is not in [0, C), is invalid and reads nothing.  No atomics, no workgroup waits for another, nothing depends on
// scheduling.  No model: no handle.
//
// kl_span_pick: one wave per span.  Lane l walks candidates l, l + 64, .. in ascending order and keeps the least cost (the
// first among equal ones); a butterfly over the wave then takes the minimum under the total order (cost, index) -- the result
// does not depend on the order of the exchanges, so two calls on the same input agree bit for bit.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_emit_row.h"

namespace {

static_assert(KL_SPAN_LEN_MAX <= 64, "the first wave decides about a candidate's ids");

__global__ void __launch_bounds__(256) span_windows_kernel(
    const int32_t* __restrict__ corpus, long long n_corpus, const long long* __restrict__ offsets, int n_texts,
    const int32_t* __restrict__ text_ctx, int n_ctx, const int32_t* __restrict__ span_text,
    const long long* __restrict__ span_start, const int32_t* __restrict__ span_len, const long long* __restrict__ span_first, int S,
    const int32_t* __restrict__ pool, long long n_pool, const long long* __restrict__ cand_off, long long C, long long row0,
    int left, int ahead, int M, int T, int32_t* __restrict__ idx, int32_t* __restrict__ ctx, int32_t* __restrict__ tgt,
    int32_t* __restrict__ valid) {
  __shared__ int32_t s_q[KL_VAR_MAX_Q];
  __shared__ int32_t s_ctx[KL_VAR_MAX_CTX];
  const long long b = row0 + blockIdx.x;
  // the first s in [0, S] with span_first[s] + s > b; the row's span is s - 1  (span_first[0] == 0 <= b: s >= 1)
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (span_first[mid] + mid > b) hi = mid; else lo = mid + 1;
  }
  bool ok = lo > 0;
  const int s = ok ? lo - 1 : 0;
  const long long v = b - (span_first[s] + s);      // 0: the text as written, else candidate v - 1 of the span
  const bool written = v == 0;
  const CorpusView x(corpus, n_corpus, offsets, n_texts);
  const int text = span_text[s], D = span_len[s];
  const long long g = span_start[s];
  int L = 0, A = 0;
  ok = ok && text >= 0 && text < n_texts && D >= 0 && D <= M;
  if (ok) {
    const long long o0 = offsets[text], o1 = offsets[text + 1];
    const long long lim = o1 < x.n_read ? o1 : x.n_read;
    ok = o0 <= g && g <= lim && (long long)D <= lim - g;
    if (ok) {
      cut_contexts(g - o0, o1 - g - D, left, ahead, L, A);      // (after >= 0: g + D <= lim <= o1)
      ok = L >= 1 && D + A >= 1;
    }
  }
  // r: the written characters x[g .. g+D-1], or the candidate's ids pool[r0 .. r0+m-1]
  int m = D;
  long long r0 = 0;
  if (!written) {      // (uniform over the workgroup, as is `ok`)
    if (ok) {
      const long long c = span_first[s] + v - 1;
      ok = c >= 0 && c < C;
      if (ok) {
        const long long from = cand_off[c], to = cand_off[c + 1];
        ok = from >= 0 && to >= from && to - from <= (long long)M && to <= n_pool;
        if (ok) {
          r0 = from;
          m = (int)(to - from);
          ok = m + A >= 1;
        }
      }
    }
    int negative = 0, differs = 0;
    if (ok && (int)threadIdx.x < m) {
      const int32_t id = pool[r0 + threadIdx.x];
      negative = id < 0;
      differs = (int)threadIdx.x >= D || id != x.read(g + threadIdx.x);
    }
    negative = __syncthreads_or(negative);
    differs = __syncthreads_or(differs);
    ok = ok && !negative && (m != D || differs);
  }
  // q: L characters in front of g, r, the A characters behind g + D -- len = L + m + A <= left + M + ahead <= T + 1
  const int len = ok ? L + m + A : 0;
  for (int t = threadIdx.x; t < len; t += blockDim.x) {
    int32_t id;
    if (t < L) id = x.read(g - L + t);
    else if (t < L + m) id = written ? x.read(g + (t - L)) : pool[r0 + (t - L)];
    else id = x.read(g + D + (t - L - m));
    s_q[t] = id;
  }
  // q[0 .. len-2] is fed, q[L .. len-1] is predicted
  emit_hypothesis(ok, text, len > 0 ? len - 1 : 0, L - 1, s_q, s_ctx, text_ctx, n_ctx, T, idx, ctx, tgt, valid);
}

__global__ void __launch_bounds__(KL_WAVE) span_pick_kernel(
    const double* __restrict__ cost, const int32_t* __restrict__ valid, const long long* __restrict__ span_first, long long C,
    double min_gain, int32_t* __restrict__ best, double* __restrict__ gain, double* __restrict__ cost_out) {
  const int s = blockIdx.x;
  // the span's candidates [from, to) inside [0, C): its rows from + s (written) .. to + s stay below S + C
  long long from = span_first[s], to = span_first[s + 1];
  from = from < 0 ? 0 : from > C ? C : from;
  to = to < from ? from : to > C ? C : to;
  const long long w = from + s, n = to - from;
  const double inf = __builtin_huge_val();
  double bc = 0.0;
  long long bj = -1;
  for (long long j = threadIdx.x; j < n; j += KL_WAVE) {
    const double c = cost[w + 1 + j];
    const bool ok = valid[w + 1 + j] != 0;
    if (cost_out) cost_out[w + 1 + j] = ok ? c : inf;
    if (ok && c == c && (bj < 0 || c < bc)) {      // (ascending j: the first of equal costs stays; a NaN never enters)
      bc = c;
      bj = j;
    }
  }
  for (int off = KL_WAVE / 2; off > 0; off >>= 1) {
    const double oc = __shfl_xor(bc, off, KL_WAVE);
    const long long oj = __shfl_xor(bj, off, KL_WAVE);
    if (oj >= 0 && (bj < 0 || oc < bc || (oc == bc && oj < bj))) {
      bc = oc;
      bj = oj;
    }
  }
  if (threadIdx.x == 0) {
    const double cw = cost[w];
    const bool w_ok = valid[w] != 0;
    if (cost_out) cost_out[w] = w_ok ? cw : inf;
    const double saved = cw - bc;
    const bool keep = w_ok && bj >= 0 && saved >= min_gain;      // (a NaN gain or min_gain keeps nothing)
    best[s] = keep ? (int32_t)bj : -1;
    gain[s] = keep ? saved : 0.0;
  }
}

}  // namespace

extern "C" int kl_span_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts,
                               const int32_t* text_ctx, int n_ctx, const int32_t* span_text, const int64_t* span_start,
                               const int32_t* span_len, const int64_t* span_first, int S, const int32_t* pool, size_t n_pool,
                               const int64_t* cand_off, int64_t C, int64_t row0, int rows, int left, int ahead, int max_len, int T,
                               int32_t* idx, int32_t* ctx, int32_t* tgt, int32_t* valid, void* stream) {
  if (!corpus || !offsets || !span_text || !span_start || !span_len || !span_first || !cand_off || !idx || !tgt || !valid)
    return KL_ERR_ARG;
  if (!pool && n_pool > 0) return KL_ERR_ARG;
  if (S < 1 || n_texts < 1 || rows < 1 || (long long)rows > KL_VAR_MAX_ROWS) return KL_ERR_ARG;
  if (C < 0 || C > ((int64_t)1 << 40) || row0 < 0 || row0 + (int64_t)rows > (int64_t)S + C) return KL_ERR_ARG;
  if (left < 1 || ahead < 0 || max_len < 1 || max_len > KL_SPAN_LEN_MAX) return KL_ERR_ARG;
  // (with T <= KL_VAR_MAX_T: q, at most left + max_len + ahead <= T + 1 ids, fits the staging array)
  if ((long long)T < (long long)left + ahead + max_len - 1 || n_pool > (size_t)1 << 40) return KL_ERR_ARG;
  if (!hypothesis_args_ok(n_ctx, text_ctx, ctx, n_corpus, T, {corpus, text_ctx, span_text, span_len, pool, idx, ctx, tgt, valid},
                          {offsets, span_start, span_first, cand_off}))
    return KL_ERR_ARG;
  hipLaunchKernelGGL(span_windows_kernel, dim3((unsigned)rows), dim3(hypothesis_threads(T, n_ctx)), 0,
                     static_cast<hipStream_t>(stream), corpus, (long long)n_corpus, reinterpret_cast<const long long*>(offsets),
                     n_texts, text_ctx, n_ctx, span_text, reinterpret_cast<const long long*>(span_start), span_len,
                     reinterpret_cast<const long long*>(span_first), S, pool, (long long)n_pool,
                     reinterpret_cast<const long long*>(cand_off), (long long)C, (long long)row0, left, ahead, max_len, T, idx, ctx,
                     tgt, valid);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_span_pick(const double* cost, const int32_t* valid, const int64_t* span_first, int S, int64_t C, double min_gain,
                            int32_t* best, double* gain, double* cost_out, void* stream) {
  if (!cost || !valid || !span_first || !best || !gain) return KL_ERR_ARG;
  if (S < 1 || C < 0 || C > ((int64_t)1 << 40)) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(valid) & 3) || (reinterpret_cast<uintptr_t>(best) & 3)) return KL_ERR_ARG;
  const void* longs[] = {cost, span_first, gain, cost_out};
  for (const void* p : longs)
    if (reinterpret_cast<uintptr_t>(p) & 7) return KL_ERR_ARG;
  hipLaunchKernelGGL(span_pick_kernel, dim3((unsigned)S), dim3(KL_WAVE), 0, static_cast<hipStream_t>(stream), cost, valid,
                     reinterpret_cast<const long long*>(span_first), (long long)C, min_gain, best, gain, cost_out);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
