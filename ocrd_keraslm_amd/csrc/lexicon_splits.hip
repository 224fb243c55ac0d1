// Lexicon look-up across a lost space (kl_lexicon_splits): at which places does a query word fall into two lexicon entries?
//
// The missing delimiter costs one edit, so each half may lie d = max_dist - 1 edits from its entry.  Pairs of entries are never
// formed: after Myers' column (kl_lexicon_myers.h) has consumed an entry e of L ids, its vertical deltas hold lev(q[:i], e) for
// EVERY prefix length i -- D[i] = L + popc(Pv & low(i)) - popc(Mv & low(i)) --, and the same walk with the reversed query over the
// entry read back to front holds every suffix.  So one workgroup per query in the frame all four look-ups share
// (kl_lexicon_frame.h: the class table through the workspace, the query's bounds, Peq, the minimum in LDS), and two passes
// over the length classes max(1, min_part - d) .. min(64, m - min_part + d):
//
//   forward   Peq of the query in LDS; every lane walks whole entries and, after an entry's last character, reads D[i] for the
//             split points i in [max(min_part, L - d), min(m - min_part, L + d)] -- at most 2d + 1 pairs of popcounts; where
//             D[i] <= d it lowers s_left[i] to (lev << 32 | original index) with a 64-bit unsigned minimum in LDS;
//   backward  Peq rebuilt for the reversed query, the entries walked from their last character to the first (the column-major
//             layout serves that equally): D[i] is the suffix of i ids, which lowers s_right[m - i];
//   select    thread s forms total << 37 | max(left index, right index) << 6 | s; the keys are distinct, so a key's rank is the
//             number of smaller keys, and the ranks below K write the outputs.
//
// A minimum does not depend on the order of arrival: two calls agree bit for bit (the argument confusions.hip makes for its
// integer atomics).  The atomics are on LDS only; no workgroup waits for another.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_lexicon_myers.h"

namespace {

constexpr unsigned long long NO_KEY = ~0ull;
constexpr int MIN_PART_MAX = LEX_LEN_MAX / 2;      // a larger one leaves no query a split point

// a lane's walk over the entries e = tid, tid + LEX_THREADS, .. of every length class that can hold a half of a query of m
// ids: where the first i ids of the pattern (the query, or with BACK the reversed query against the entry read back to
// front) lie within d edits of an entry, the key of that entry lowers s_best[i] (with BACK: s_best[m - i])
template <typename W, bool BACK>
__device__ __forceinline__ void walk_halves(const int* __restrict__ chars, const int* __restrict__ order,
                                            const long long* __restrict__ table, const unsigned long long* peq, int V, int m,
                                            int d, int min_part, int tid, unsigned long long* s_best) {
  const int lo = min_part - d > 1 ? min_part - d : 1;
  const int hi = m - min_part + d < LEX_LEN_MAX ? m - min_part + d : LEX_LEN_MAX;
  for (int L = lo; L <= hi; ++L) {
    const long long at = table[L], n_L = table[L + 1] - at, base = table[LEX_CLASSES + L];
    const int i_lo = L - d > min_part ? L - d : min_part;
    const int i_hi = L + d < m - min_part ? L + d : m - min_part;      // (i_lo <= i_hi for every L of lo .. hi)
    for (long long e = tid; e < n_L; e += LEX_THREADS) {
      const int* __restrict__ col = chars + base + e;      // character j of the entry: col[j * n_L]
      W Pv = ~(W)0, Mv = 0;
      int unused = 0;      // (no top bit: the distance to the whole pattern is not wanted)
      int c = col[BACK ? (long long)(L - 1) * n_L : 0];
      for (int j = 0; j < L; ++j) {
        const int at_next = BACK ? L - 2 - j : j + 1;
        const int next = j + 1 < L ? col[(long long)at_next * n_L] : 0;      // (the next character is under way)
        myers_step<W>(match_mask<W>(peq, c, V), (W)0, Pv, Mv, unused);
        c = next;
      }
      unsigned int index = 0;
      bool have = false;
      for (int i = i_lo; i <= i_hi; ++i) {
        const W low = ((W)1 << i) - 1;      // (i <= m - 1: below the width of W)
        const int D = L + ones(Pv & low) - ones(Mv & low);
        if (D <= d) {
          if (!have) {
            index = (unsigned int)order[at + e];
            have = true;
          }
          lex_lower(&s_best[BACK ? m - i : i], ((unsigned long long)D << 32) | index);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(LEX_THREADS) lexicon_splits_kernel(
    const int* __restrict__ chars, const int* __restrict__ order, const long long* __restrict__ table, int V,
    const int* __restrict__ q_pool, long long n_q, const long long* __restrict__ q_off, int max_dist, int min_part, int K,
    int narrow, int* __restrict__ found, int* __restrict__ split, int* __restrict__ left, int* __restrict__ right,
    int* __restrict__ dist) {
  __shared__ unsigned long long peq[KL_LEXICON_V_MAX];
  __shared__ int s_query[LEX_LEN_MAX];
  __shared__ unsigned long long s_left[LEX_LEN_MAX], s_right[LEX_LEN_MAX];      // by split point s (1 .. 63)
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  long long qa;
  int m;
  // a query that is none, or too short for two halves, has no split point: nothing of the lexicon is read for it
  if (lex_query_bounds(q_off, q, n_q, 2 * min_part, qa, m)) {      // (uniform: the whole workgroup leaves)
    if (tid == 0) found[q] = 0;
    if (tid < K) {
      split[q * K + tid] = -1;
      left[q * K + tid] = -1;
      right[q * K + tid] = -1;
      dist[q * K + tid] = -1;
    }
    return;
  }
  const int d = max_dist - 1;
  if (tid < LEX_LEN_MAX) {
    s_left[tid] = NO_KEY;
    s_right[tid] = NO_KEY;
  }
  lex_query_peq<false>(peq, s_query, q_pool, qa, m, V, tid);
  __syncthreads();
  const bool w32 = narrow && m <= 32;      // (uniform: a workgroup is one query)
  if (w32)
    walk_halves<unsigned int, false>(chars, order, table, peq, V, m, d, min_part, tid, s_left);
  else
    walk_halves<unsigned long long, false>(chars, order, table, peq, V, m, d, min_part, tid, s_left);
  __syncthreads();
  lex_query_peq<true>(peq, s_query, q_pool, qa, m, V, tid);      // the reversed query: the same ids hold bits
  __syncthreads();
  if (w32)
    walk_halves<unsigned int, true>(chars, order, table, peq, V, m, d, min_part, tid, s_right);
  else
    walk_halves<unsigned long long, true>(chars, order, table, peq, V, m, d, min_part, tid, s_right);
  __syncthreads();

  // selection, by the first wave: lane s owns split point s
  if (tid >= KL_WAVE) return;
  unsigned long long key = NO_KEY;
  int l_index = -1, r_index = -1, total = -1;
  if (tid >= min_part && tid <= m - min_part) {
    const unsigned long long l = s_left[tid], r = s_right[tid];
    if (l != NO_KEY && r != NO_KEY) {
      const int t = 1 + (int)(l >> 32) + (int)(r >> 32);
      if (t <= max_dist) {
        l_index = (int)(unsigned int)l;
        r_index = (int)(unsigned int)r;
        total = t;
        const unsigned long long rarer = (unsigned int)(l_index > r_index ? l_index : r_index);
        key = ((unsigned long long)t << 37) | (rarer << 6) | (unsigned long long)tid;
      }
    }
  }
  const int n_valid = __popcll(__ballot(key != NO_KEY));
  int rank = 0;
  for (int s = 0; s < KL_WAVE; ++s) {
    const unsigned long long other = __shfl(key, s, KL_WAVE);
    rank += other < key ? 1 : 0;
  }
  if (tid == 0) found[q] = n_valid;
  if (key != NO_KEY && rank < K) {
    split[q * K + rank] = tid;
    left[q * K + rank] = l_index;
    right[q * K + rank] = r_index;
    dist[q * K + rank] = total;
  }
  if (tid < K && tid >= n_valid) {
    split[q * K + tid] = -1;
    left[q * K + tid] = -1;
    right[q * K + tid] = -1;
    dist[q * K + tid] = -1;
  }
}

}  // namespace

extern "C" size_t kl_lexicon_splits_workspace_bytes(size_t Q, int K) {
  (void)Q;
  (void)K;
  return sizeof(lex_classes);      // (the class table, whatever Q and K are)
}

extern "C" int kl_lexicon_splits(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                                 const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, int max_dist, int min_part,
                                 int K, int32_t* found, int32_t* split, int32_t* left, int32_t* right, int32_t* dist, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!found || !split || !left || !right || !dist) return KL_ERR_ARG;
  if (max_dist < 1 || max_dist > KL_LEXICON_DIST_MAX || K < 1 || K > KL_LEXICON_K_MAX) return KL_ERR_ARG;
  if (min_part < 1 || min_part > MIN_PART_MAX) return KL_ERR_ARG;
  const void* words[] = {chars, order, q_pool, found, split, left, right, dist};
  for (const void* p : words)
    if (lex_misaligned(p, 3)) return KL_ERR_ARG;
  lex_classes cls;
  if (lex_arguments_checked(chars, n_chars, order, class_first, V, q_pool, n_q, q_off, Q, ws, cls) != KL_OK) return KL_ERR_ARG;
  if (ws_bytes < kl_lexicon_splits_workspace_bytes(Q, K)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  long long* table = reinterpret_cast<long long*>(ws);
  hipLaunchKernelGGL(lexicon_classes_kernel, dim3(1), dim3(2 * KL_WAVE), 0, s, cls, table);
  hipLaunchKernelGGL(lexicon_splits_kernel, dim3((unsigned)Q), dim3(LEX_THREADS), 0, s, chars, order, table, V, q_pool,
                     (long long)n_q, reinterpret_cast<const long long*>(q_off), max_dist, min_part, K, lex_narrow(), found, split,
                     left, right, dist);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
