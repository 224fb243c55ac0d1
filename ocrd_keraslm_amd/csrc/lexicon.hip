// Lexicon look-up (kl_lexicon_neighbours): which entries of a lexicon lie within max_dist edits of each query word?
//
// The length classes of the lexicon are checked on the host and put into the workspace by a launch of one workgroup; then one
// workgroup per query.  The query is the PATTERN of Myers' bit-parallel edit distance in Hyyro's form for the global
// (Levenshtein) distance: bit i of Peq[id] says that pattern position i holds `id`, the vertical deltas of a DP column live in two
// 64-bit words, and one lexicon character advances the column in about twenty 64-bit operations -- which is why a query holds at
// most 64 ids; a query of at most 32 runs the same steps on 32-bit words (the VALU has no 64-bit add or shift: 10.7 against
// 12.1 ms for 20 000 words against 228 576 entries; KL_LEXICON_NARROW=0 switches it off).  Peq[V] lies in LDS (V * 8 bytes,
// only the query's own ids are non-zero); an id outside [0, V) on either side never reaches the table: it has no bit and
// matches nothing.  (The step is kl_lexicon_myers.h's; the class table, the query's bounds and Peq are the frame's,
// kl_lexicon_frame.h, which all four look-ups share.)
//
// Every lane then walks whole entries of the length classes max(1, m - max_dist) .. min(64, m + max_dist) -- other lengths
// cannot be within max_dist --, one character per step from the column-major layout (consecutive lanes read consecutive
// addresses), and keeps its own KL_LEXICON_K_MAX smallest keys (distance << 32 | original index) sorted in registers.  The
// workgroup then takes the K smallest heads one after the other: a minimum over the waves, the winner (the lowest thread among
// equal keys) drops its head.  `found` is an integer sum and `exact` a minimum, both folded in a fixed order (the lists and the
// fold are kl_lexicon_topk.h's, shared with kl_lexicon_channel).  No atomics, no
// workgroup waits for another, the output depends on the inputs only.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_lexicon_myers.h"
#include "kl_lexicon_topk.h"

namespace {

// a lane's walk over the entries e = tid, tid + LEX_THREADS, .. of every length class that can hold a neighbour of a query of m
// ids: its KL_LEXICON_K_MAX smallest keys (sorted), the least index at distance 0 and the number within 1 .. max_dist
template <typename W>
__device__ __forceinline__ void walk_classes(const int* __restrict__ chars, const int* __restrict__ order,
                                             const long long* __restrict__ table, const unsigned long long* peq, int V, int m,
                                             int max_dist, int tid, unsigned long long (&best)[KL_LEXICON_K_MAX],
                                             unsigned int& least_exact, int& n_found) {
  const W top = (W)1 << (m - 1);
  const int lo = m - max_dist > 1 ? m - max_dist : 1;
  const int hi = m + max_dist < LEX_LEN_MAX ? m + max_dist : LEX_LEN_MAX;
  for (int L = lo; L <= hi; ++L) {
    const long long at = table[L], n_L = table[L + 1] - at, base = table[LEX_CLASSES + L];
    for (long long e = tid; e < n_L; e += LEX_THREADS) {
      const int* __restrict__ col = chars + base + e;      // character j of the entry: col[j * n_L]
      W Pv = ~(W)0, Mv = 0;
      int score = m;
      int c = col[0];
      for (int j = 0; j < L; ++j) {
        const int next = j + 1 < L ? col[(long long)(j + 1) * n_L] : 0;      // (the next character is under way)
        myers_step<W>(match_mask<W>(peq, c, V), top, Pv, Mv, score);
        c = next;
      }
      if (score <= max_dist) {
        const unsigned int index = (unsigned int)order[at + e];
        if (score == 0) {
          least_exact = index < least_exact ? index : least_exact;
        } else {
          ++n_found;
          kl_lex_keep(((unsigned long long)score << 32) | index, best);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(LEX_THREADS) lexicon_neighbours_kernel(
    const int* __restrict__ chars, const int* __restrict__ order, const long long* __restrict__ table, int V,
    const int* __restrict__ q_pool, long long n_q, const long long* __restrict__ q_off, int max_dist, int K, int narrow,
    int* __restrict__ exact, int* __restrict__ found, int* __restrict__ cand, int* __restrict__ dist) {
  __shared__ unsigned long long peq[KL_LEXICON_V_MAX];
  __shared__ int s_query[LEX_LEN_MAX];
  __shared__ kl_lex_fold<LEX_WAVES> s_fold;
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  long long qa;
  int m;
  if (lex_query_bounds(q_off, q, n_q, 1, qa, m)) {      // a neighbour of nothing (uniform: the whole workgroup leaves)
    if (tid == 0) {
      exact[q] = -1;
      found[q] = 0;
    }
    if (tid < K) {
      cand[q * K + tid] = -1;
      dist[q * K + tid] = -1;
    }
    return;
  }
  lex_query_peq<false>(peq, s_query, q_pool, qa, m, V, tid);
  __syncthreads();

  unsigned long long best[KL_LEXICON_K_MAX];
#pragma unroll
  for (int i = 0; i < KL_LEXICON_K_MAX; ++i) best[i] = KL_LEX_NO_KEY;
  unsigned int least_exact = KL_LEX_NO_EXACT;
  int n_found = 0;
  if (narrow && m <= 32)      // (uniform: a workgroup is one query)
    walk_classes<unsigned int>(chars, order, table, peq, V, m, max_dist, tid, best, least_exact, n_found);
  else
    walk_classes<unsigned long long>(chars, order, table, peq, V, m, max_dist, tid, best, least_exact, n_found);

  kl_lex_fold_out<LEX_WAVES>(s_fold, best, least_exact, n_found, K, q, exact, found, cand, dist);
}

}  // namespace

extern "C" size_t kl_lexicon_neighbours_workspace_bytes(size_t Q, int K) {
  (void)Q;
  (void)K;
  return sizeof(lex_classes);      // (the class table, whatever Q and K are)
}

extern "C" int kl_lexicon_neighbours(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                                     const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, int max_dist, int K,
                                     int32_t* exact, int32_t* found, int32_t* cand, int32_t* dist, void* ws, size_t ws_bytes,
                                     void* stream) {
  if (!exact || !found || !cand || !dist) return KL_ERR_ARG;
  if (max_dist < 0 || max_dist > KL_LEXICON_DIST_MAX || K < 1 || K > KL_LEXICON_K_MAX) return KL_ERR_ARG;
  const void* words[] = {chars, order, q_pool, exact, found, cand, dist};
  for (const void* p : words)
    if (lex_misaligned(p, 3)) return KL_ERR_ARG;
  lex_classes cls;
  if (lex_arguments_checked(chars, n_chars, order, class_first, V, q_pool, n_q, q_off, Q, ws, cls) != KL_OK) return KL_ERR_ARG;
  if (ws_bytes < kl_lexicon_neighbours_workspace_bytes(Q, K)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  long long* table = reinterpret_cast<long long*>(ws);
  hipLaunchKernelGGL(lexicon_classes_kernel, dim3(1), dim3(2 * KL_WAVE), 0, s, cls, table);
  hipLaunchKernelGGL(lexicon_neighbours_kernel, dim3((unsigned)Q), dim3(LEX_THREADS), 0, s, chars, order, table, V, q_pool,
                     (long long)n_q, reinterpret_cast<const long long*>(q_off), max_dist, K, lex_narrow(), exact, found, cand, dist);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
