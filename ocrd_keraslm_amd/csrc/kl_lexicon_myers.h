// What the bit-parallel lexicon look-ups (kl_lexicon_neighbours, kl_lexicon_splits) share in front of their folds: the class
// table and its way through the workspace, and one step of Myers' bit-parallel edit distance in Hyyro's form for the global
// (Levenshtein) distance with the match mask it takes.
#pragma once
#include "keraslm_hip.h"
#include "kl_common.h"

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

// one text character against the pattern column (Pv, Mv: vertical deltas +1 / -1; score: the distance to the whole pattern); the
// pattern word W is 64 bits, or 32 for a query of at most 32 ids (half the instructions: the VALU has no 64-bit add or shift)
template <typename W>
__device__ __forceinline__ void myers_step(W Eq, W top, W& Pv, W& Mv, int& score) {
  const W Xv = Eq | Mv;
  const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  W Ph = Mv | ~(Xh | Pv);
  W Mh = Pv & Xh;
  score += (Ph & top) ? 1 : 0;
  score -= (Mh & top) ? 1 : 0;
  Ph = (Ph << 1) | (W)1;      // (row 0 of the global distance grows by one per text character)
  Mh <<= 1;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
}

// the match mask of id c for the pattern word: the whole word of Peq, or its low half
template <typename W>
__device__ __forceinline__ W match_mask(const unsigned long long* peq, int c, int V);
template <>
__device__ __forceinline__ unsigned long long match_mask<unsigned long long>(const unsigned long long* peq, int c, int V) {
  return (c >= 0 && c < V) ? peq[c] : 0ull;
}
template <>
__device__ __forceinline__ unsigned int match_mask<unsigned int>(const unsigned long long* peq, int c, int V) {
  return (c >= 0 && c < V) ? reinterpret_cast<const unsigned int*>(peq)[2 * c] : 0u;
}
