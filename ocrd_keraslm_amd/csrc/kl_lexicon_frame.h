// The frame of the four lexicon look-ups (kl_lexicon_neighbours, kl_lexicon_channel, kl_lexicon_splits, kl_lexicon_chains):
// what is not the walk over the entries.  On the host the checks of the arguments they have in common, the class table with
// every address a walk forms checked, and the one read of KL_LEXICON_NARROW; on the device the class table's way through the
// workspace, the test whether a query is one at all, the query's match masks Peq in LDS, and the minimum in LDS that the walks
// of kl_lexicon_splits and kl_lexicon_chains lower.  The __shared__ arrays are the kernels' own and come in as pointers.
#pragma once
#include "keraslm_hip.h"
#include "kl_common.h"
#include <stdlib.h>

constexpr int LEX_THREADS = 256;
constexpr int LEX_WAVES = LEX_THREADS / KL_WAVE;
constexpr int LEX_LEN_MAX = 64;      // ids of a query and of an entry at most: one pattern word
constexpr size_t LEX_MAX_QUERIES = 0x7FFFFFFF;      // (one workgroup per query in one grid)
constexpr size_t LEX_MAX_POOL = (size_t)1 << 40;
static_assert(KL_LEXICON_V_MAX * 8 <= 32 * 1024, "Peq fits 32 KiB of LDS");

constexpr int LEX_CLASSES = LEX_LEN_MAX + 2;
// the length classes, checked on the host: entries of length L are the sorted positions [first[L], first[L + 1]) and their
// characters begin at chars[base[L]]
struct lex_classes {
  long long first[LEX_CLASSES];
  long long base[LEX_CLASSES];
};

// the class table from a launch's arguments to the workspace, every index into the arguments a constant (an index known at run
// time only would send the table through scratch): table[L] = first[L], table[LEX_CLASSES + L] = base[L]
static __global__ void __launch_bounds__(2 * KL_WAVE) lexicon_classes_kernel(const lex_classes cls, long long* __restrict__ table) {
#pragma unroll
  for (int i = 0; i < LEX_CLASSES; ++i)
    if ((int)threadIdx.x == i) {
      table[i] = cls.first[i];
      table[LEX_CLASSES + i] = cls.base[i];
    }
}

// the class table of class_first (HOST int64 [66]) for a lexicon of n_chars ids: every address a walk forms is checked here;
// false for a table that breaks the rules of the header or disagrees with n_chars
inline bool lex_classes_checked(const int64_t* class_first, size_t n_chars, lex_classes& cls) {
  if (class_first[0] != 0 || class_first[1] != 0) return false;
  for (int L = 1; L <= LEX_LEN_MAX + 1; ++L)
    if (class_first[L] < class_first[L - 1] || class_first[L] > 0x7FFFFFFFll) return false;
  long long total = 0;      // (at most 64 * 2^31)
  for (int L = 0; L <= LEX_LEN_MAX + 1; ++L) {
    cls.first[L] = class_first[L];
    cls.base[L] = total;
    if (L <= LEX_LEN_MAX) total += (long long)L * (class_first[L + 1] - class_first[L]);
  }
  return class_first[LEX_LEN_MAX + 1] >= 1 && (unsigned long long)total == (unsigned long long)n_chars;
}

inline bool lex_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// the arguments every look-up has, checked (an entry point adds its own -- outputs, K, distances, links, rules and the list of
// what is aligned to four bytes -- and only then compares the workspace): KL_OK and the class table in cls, or KL_ERR_ARG
inline int lex_arguments_checked(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                                 const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, const void* ws,
                                 lex_classes& cls) {
  if (!chars || !order || !class_first || !q_off || !ws) return KL_ERR_ARG;
  if (n_q > 0 && !q_pool) return KL_ERR_ARG;
  if (V < 1 || V > KL_LEXICON_V_MAX) return KL_ERR_ARG;
  if (Q < 1 || Q > LEX_MAX_QUERIES || n_q > LEX_MAX_POOL || n_chars > LEX_MAX_POOL) return KL_ERR_ARG;
  if (lex_misaligned(q_off, 7) || lex_misaligned(class_first, 7) || lex_misaligned(ws, 7)) return KL_ERR_ARG;
  return lex_classes_checked(class_first, n_chars, cls) ? KL_OK : KL_ERR_ARG;
}

// KL_LEXICON_NARROW=0: the 64-bit pattern word for every query, also one of at most 32 ids (the A/B switch of
// tools/bench_lexicon.py)
inline int lex_narrow() {
  const char* env = getenv("KL_LEXICON_NARROW");
  return !(env && env[0] == '0');
}

// Is query q none?  One outside the pool, of no ids, of more than 64 or of fewer than min_len is looked up nowhere, and nothing
// of it is read.  Otherwise qa is where it begins in the pool and m its number of ids.  (Uniform over a workgroup.)
__device__ __forceinline__ bool lex_query_bounds(const long long* __restrict__ q_off, long long q, long long n_q, int min_len,
                                                 long long& qa, int& m) {
  qa = q_off[q];
  const long long qb = q_off[q + 1];
  m = (int)(qb - qa);
  return qa < 0 || qb <= qa || qb > n_q || qb - qa > LEX_LEN_MAX || qb - qa < (long long)min_len;
}

// The match masks of a query of m ids in LDS: bit i of peq[id] says that position i (REVERSED: position m - 1 - i) holds `id`;
// only the query's own ids in [0, V) have a word that is not zero.  Forward it zeroes peq[0 .. V) and loads the query into
// s_query, and a barrier stands between that and the words; REVERSED it follows the forward build of the same query and only
// rewrites the words of the ids the query holds.  No barrier behind the words: the caller has one before it reads them.
template <bool REVERSED>
__device__ __forceinline__ void lex_query_peq(unsigned long long* peq, int* s_query, const int* __restrict__ q_pool, long long qa,
                                              int m, int V, int tid) {
  if (!REVERSED) {
    for (int v = tid; v < V; v += LEX_THREADS) peq[v] = 0ull;
    if (tid < m) s_query[tid] = q_pool[qa + tid];
    __syncthreads();
  }
  if (tid < m) {
    // all positions that hold this id write the same word: no atomics
    const int id = s_query[tid];
    if (id >= 0 && id < V) {
      unsigned long long bits = 0ull;
      for (int j = 0; j < m; ++j) bits |= s_query[REVERSED ? m - 1 - j : j] == id ? 1ull << j : 0ull;
      peq[id] = bits;
    }
  }
}

__device__ __forceinline__ int ones(unsigned int w) { return __popc(w); }
__device__ __forceinline__ int ones(unsigned long long w) { return __popcll(w); }
__device__ __forceinline__ int lowest(unsigned int w) { return __ffs(w) - 1; }
__device__ __forceinline__ int lowest(unsigned long long w) { return __ffsll(w) - 1; }

// the least key of a place in LDS so far, lowered (relaxed, workgroup scope: the barrier behind a pass orders it); a key that is
// not below what the place already shows is dropped without the atomic -- what it shows can only have gone down since
__device__ __forceinline__ void lex_lower(unsigned long long* place, unsigned long long key) {
  if (key < __hip_atomic_load(place, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
    __hip_atomic_fetch_min(place, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lex_lower(unsigned int* place, unsigned int key) {
  if (key < __hip_atomic_load(place, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
    __hip_atomic_fetch_min(place, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
