// What the bit-parallel lexicon look-ups (kl_lexicon_neighbours, kl_lexicon_splits, kl_lexicon_chains) take on top of the frame
// (kl_lexicon_frame.h): one step of Myers' bit-parallel edit distance in Hyyro's form for the global (Levenshtein) distance,
// and the match mask it takes from Peq -- which kl_lexicon_chains' exact match takes too.
#pragma once
#include "kl_lexicon_frame.h"

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
