// What the two lexicon look-ups (kl_lexicon_neighbours, kl_lexicon_channel) share behind their walks: a lane's
// KL_LEXICON_K_MAX smallest keys (distance << 32 | original index) sorted in registers, and the workgroup's fold of them -- `exact`
// a minimum and `found` an integer sum, folded in a fixed order, then the K smallest heads one after the other: a minimum over
// the waves, the winner (the lowest thread among equal keys) drops its head.  No atomics: the output depends on the keys only.
#pragma once
#include "keraslm_hip.h"
#include "kl_common.h"

static_assert(KL_LEXICON_K_MAX == 16, "the lanes' key lists are written out for 16 keys");

constexpr unsigned long long KL_LEX_NO_KEY = ~0ull;
constexpr unsigned int KL_LEX_NO_EXACT = 0xFFFFFFFFu;

// the LDS the fold needs, for a workgroup of WAVES waves
template <int WAVES>
struct kl_lex_fold {
  unsigned long long key[WAVES], mask[WAVES];
  unsigned int exact[WAVES];
  int found[WAVES];
};

__device__ __forceinline__ unsigned long long kl_lex_wave_min(unsigned long long v) {
#pragma unroll
  for (int off = KL_WAVE / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, KL_WAVE);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int kl_lex_wave_sum(int v) {
#pragma unroll
  for (int off = KL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, KL_WAVE);
  return v;
}

// a key into a lane's sorted list (every index a constant: registers)
__device__ __forceinline__ void kl_lex_keep(unsigned long long key, unsigned long long (&best)[KL_LEXICON_K_MAX]) {
  if (key < best[KL_LEXICON_K_MAX - 1]) {
#pragma unroll
    for (int i = 0; i < KL_LEXICON_K_MAX; ++i) {
      const unsigned long long b = best[i];
      const bool less = key < b;
      best[i] = less ? key : b;
      key = less ? b : key;
    }
  }
}

// exact[q], found[q], cand[q][0..K) and dist[q][0..K) from every lane's list, least exact index and count; all threads of the
// workgroup call it
template <int WAVES>
__device__ __forceinline__ void kl_lex_fold_out(kl_lex_fold<WAVES>& s, unsigned long long (&best)[KL_LEXICON_K_MAX],
                                                unsigned int least_exact, int n_found, int K, long long q,
                                                int* __restrict__ exact, int* __restrict__ found, int* __restrict__ cand,
                                                int* __restrict__ dist) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // exact and found
  {
    unsigned int x = least_exact;
#pragma unroll
    for (int off = KL_WAVE / 2; off > 0; off >>= 1) {
      const unsigned int o = __shfl_xor(x, off, KL_WAVE);
      x = o < x ? o : x;
    }
    const int f = kl_lex_wave_sum(n_found);
    if (lane == 0) {
      s.exact[wave] = x;
      s.found[wave] = f;
    }
  }
  __syncthreads();
  if (tid == 0) {
    unsigned int x = s.exact[0];
    int f = s.found[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      x = s.exact[w] < x ? s.exact[w] : x;
      f += s.found[w];
    }
    exact[q] = x == KL_LEX_NO_EXACT ? -1 : (int)x;
    found[q] = f;
  }
  // the K smallest keys of the workgroup, one per round
  for (int r = 0; r < K; ++r) {
    const unsigned long long head = best[0];
    const unsigned long long wmin = kl_lex_wave_min(head);
    if (lane == 0) s.key[wave] = wmin;
    __syncthreads();
    unsigned long long gmin = s.key[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) gmin = s.key[w] < gmin ? s.key[w] : gmin;
    const unsigned long long mask = __ballot(head == gmin && gmin != KL_LEX_NO_KEY);
    if (lane == 0) s.mask[wave] = mask;
    __syncthreads();
    int w_first = WAVES;
#pragma unroll
    for (int w = WAVES - 1; w >= 0; --w) w_first = s.mask[w] != 0ull ? w : w_first;
    if (wave == w_first && lane == __ffsll((long long)mask) - 1) {      // the lowest thread among equal keys drops its head
#pragma unroll
      for (int i = 0; i + 1 < KL_LEXICON_K_MAX; ++i) best[i] = best[i + 1];
      best[KL_LEXICON_K_MAX - 1] = KL_LEX_NO_KEY;
    }
    if (tid == 0) {
      cand[q * K + r] = gmin == KL_LEX_NO_KEY ? -1 : (int)(unsigned int)(gmin & 0xFFFFFFFFull);
      dist[q * K + r] = gmin == KL_LEX_NO_KEY ? -1 : (int)(gmin >> 32);
    }
  }
}
