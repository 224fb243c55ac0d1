// Witness consensus (kl_witness_clusters, kl_witness_pool): from the differing spans kl_align_pairs left on the device for ALL
// witnesses of a text to kl_span_windows' own span and candidate arrays -- the spans clustered across witnesses, every witness
// read over a whole cluster, equal readings made one and counted.
//
// One WAVE per text, lane w its witness w (KL_WITNESS_MAX is the wave's width), a grid-stride loop over the texts.  A lane
// checks its pair (every slot inside both texts, ascending) and keeps a cursor into its span slots, which ascend: the sweep of
// the statement over the spans in order of (a0, a1, witness, slot) is a 64-way merge.  The least a0 under a cursor (a minimum
// over the wave) opens a cluster with the running end E = u0; every lane takes its slots with a0 <= E + join and raises its E,
// the wave takes the maximum, until a round leaves E as it was -- the closure the sweep computes, whatever the order within it.
// The slots a lane took are its run f .. l: the reading's range in the witness is arithmetic on two slots.  Equal readings: the
// lowest lane not yet settled is a leader, its position and length go round by shuffle, every unsettled lane compares its
// code points with the leader's (at most KL_SPAN_LEN_MAX, read from b_pool), a ballot is the candidate's votes and settles
// them; leaders come in order of the first witness.  Everything is in registers: no LDS, no barrier.
//
// Four plain launches on the stream:
//   0. witness_init_kernel     every output to its fill over its whole room, the call's counters 0
//   1. witness_sweep_kernel<false>   per text the kept clusters, their candidates and the candidates' symbols (counts [3][n_texts]);
//                              `different`, `first`, `long`, bad texts and the longest kept span or reading through ONE integer
//                              atomic per wave and reason at the end of the wave's loop (sums and a maximum)
//   2. witness_offsets_kernel  kl_compact.h's one workgroup: the three rows of counts to exclusive offsets, the totals to stats,
//                              span_first[S] = C and cand_off[C] = n_pool
//   3. witness_sweep_kernel<true>    the same sweep, recomputed, writes every kept cluster at its text's offsets: the order by text
//                              and u0 whatever the order of arrival
// and one for kl_witness_pool: a lane per position of the pool finds its candidate by bisection of cand_off.
// No float atomics, no workgroup waits for another, every loop is bounded by the arguments; the outputs depend on the inputs
// only.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_compact.h"

namespace {

typedef unsigned long long u64;

constexpr int WIT_THREADS = 256;
constexpr int WIT_WAVES = WIT_THREADS / KL_WAVE;
constexpr long long WIT_GRID_MAX = 1024;      // workgroups of a launch at most
constexpr size_t MAX_PAIRS = 0x7FFFFFFF;
constexpr long long NO_SPAN = 1ll << 32;      // above every a0
enum { DIFFERENT = 0, FIRST = 1, LONG = 2, BAD = 3, LONGEST = 4, TOTALS = 5, N_COUNTERS = 8 };
static_assert(KL_WITNESS_MAX == KL_WAVE, "a lane per witness");

// the workspace: everything 256-byte aligned
struct wit_layout {
  size_t counters, counts, bytes;      // u64 [N_COUNTERS]; long long [3][n_texts]: clusters, candidates, symbols
};

inline size_t padded(size_t bytes) { return (bytes + 255) / 256 * 256; }

inline wit_layout layout_of(size_t n_texts) {
  wit_layout l;
  size_t at = 0;
  l.counters = at, at += padded(N_COUNTERS * 8);
  l.counts = at, at += padded(3 * n_texts * 8);
  l.bytes = at;
  return l;
}

inline unsigned grid_for(long long items, long long per_block) {
  const long long blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : blocks < WIT_GRID_MAX ? blocks : WIT_GRID_MAX);
}

__device__ __forceinline__ long long wave_least(long long v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const long long u = __shfl_xor(v, off);
    v = u < v ? u : v;
  }
  return v;
}

__device__ __forceinline__ long long wave_greatest(long long v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const long long u = __shfl_xor(v, off);
    v = u > v ? u : v;
  }
  return v;
}

// what a wave has seen in its texts (wave-uniform)
struct wit_sums {
  long long different, first, too_long, bad;
  int longest;
};

// where a text's kept clusters, candidates and symbols go, and the outputs (PLACE only)
struct wit_out {
  int* __restrict__ span_text;
  long long* __restrict__ span_start;
  int* __restrict__ span_len;
  long long* __restrict__ span_first;
  long long* __restrict__ cand_src;
  long long* __restrict__ cand_off;
  int* __restrict__ votes;
};

// Text i on one wave.  Returns its kept clusters, candidates and symbols in n_s, n_c, n_p; with PLACE writes them from
// (s_at, c_at, p_at) on.
template <bool PLACE>
__device__ __forceinline__ void sweep_text(const int* __restrict__ b_pool, long long n_b, const long long* __restrict__ b_off,
                                           long long P, int K, const int* __restrict__ dist, const int* __restrict__ n_spans,
                                           const int* __restrict__ spans, const long long* __restrict__ pair_first,
                                           const long long* __restrict__ text_off, int join, long long i, long long s_at,
                                           long long c_at, long long p_at, const wit_out& out, long long& n_s, long long& n_c,
                                           long long& n_p, wit_sums& sums) {
  const int lane = threadIdx.x & 63;
  n_s = n_c = n_p = 0;
  const long long q0 = pair_first[i], q1 = pair_first[i + 1];
  if (q0 < 0 || q1 < q0 || q1 > P || q1 - q0 > KL_WITNESS_MAX) {      // (the wave's text: uniform)
    ++sums.bad;
    return;
  }
  const long long t_lo = text_off[i], n = text_off[i + 1] - t_lo;
  const bool mine = lane < q1 - q0;
  const int* __restrict__ my = nullptr;      // the lane's span slots; read below `count` only
  long long b_lo = 0, m = 0;
  int count = 0;
  bool ok = false;
  if (mine) {
    const long long q = q0 + lane;
    const long long b_hi = b_off[q + 1];
    b_lo = b_off[q];
    m = b_hi - b_lo;
    count = n_spans[q];
    my = spans + q * K * 4;
    ok = dist[q] >= 0 && b_lo >= 0 && b_hi >= b_lo && b_hi <= n_b && count >= 0 && count <= K;
    int end_a = 0, end_b = 0;
    for (int s = 0; ok && s < count; ++s) {
      const int a0 = my[4 * s], a1 = my[4 * s + 1], b0 = my[4 * s + 2], b1 = my[4 * s + 3];
      ok = a0 >= end_a && a1 >= a0 && a1 <= n && b0 >= end_b && b1 >= b0 && b1 <= m;
      end_a = a1;
      end_b = b1;
    }
    if (!ok) count = 0;
  }
  sums.different += __popcll(__ballot(mine && !ok));
  int cur = 0;
  for (;;) {      // (every round takes at least one of the text's at most 64 K slots)
    const long long u0 = wave_least(cur < count ? (long long)my[4 * cur] : NO_SPAN);
    if (u0 == NO_SPAN) break;
    const int f = cur;
    long long E = u0;
    for (;;) {
      long long e = E;
      while (cur < count && my[4 * cur] <= e + join) {
        const long long a1 = my[4 * cur + 1];
        e = a1 > e ? a1 : e;
        ++cur;
      }
      e = wave_greatest(e);
      if (e == E) break;      // no lane saw further: none has a slot left below E + join
      E = e;
    }
    const long long u1 = E;
    const bool has = cur > f;
    long long bs = 0, be = 0;
    if (has) {
      bs = (long long)my[4 * f + 2] - (my[4 * f] - u0);
      be = (long long)my[4 * (cur - 1) + 3] + (u1 - my[4 * (cur - 1) + 1]);
    }
    const int len = (int)(be - bs < KL_SPAN_LEN_MAX + 1 ? be - bs : KL_SPAN_LEN_MAX + 1);
    const bool outside = has && (bs < 0 || be > m || len > KL_SPAN_LEN_MAX);
    const bool too_long = __ballot(outside) != 0ull || u1 - u0 > KL_SPAN_LEN_MAX;
    if (u0 == 0) {
      ++sums.first;
      continue;
    }
    if (too_long) {
      ++sums.too_long;
      continue;
    }
    const long long at = b_lo + bs;      // (inside [b_lo, b_lo + m - len], and that inside the pool)
    const int agree = __popcll(__ballot(ok && !has));
    if (PLACE && lane == 0) {
      out.span_text[s_at + n_s] = (int)i;
      out.span_start[s_at + n_s] = t_lo + u0;
      out.span_len[s_at + n_s] = (int)(u1 - u0);
      out.span_first[s_at + n_s] = c_at + n_c;
      out.votes[c_at + n_c + s_at + n_s] = 1 + agree;      // the text as written, and who reads it so
    }
    int longest = (int)(u1 - u0);
    u64 todo = __ballot(has);
    while (todo) {      // (a leader settles itself: at most 64 rounds)
      const int leader = __ffsll((long long)todo) - 1;
      const long long its = __shfl(at, leader);
      const int its_len = __shfl(len, leader);
      bool same = ((todo >> lane) & 1ull) != 0ull && len == its_len;
      for (int k = 0; same && k < its_len; ++k) same = b_pool[at + k] == b_pool[its + k];
      const u64 equal = __ballot(same);
      if (PLACE && lane == leader) {
        out.cand_src[c_at + n_c] = at;
        out.cand_off[c_at + n_c] = p_at + n_p;
        out.votes[c_at + n_c + s_at + n_s + 1] = __popcll(equal);
      }
      ++n_c;
      n_p += its_len;
      longest = its_len > longest ? its_len : longest;
      todo &= ~equal;
    }
    ++n_s;
    sums.longest = longest > sums.longest ? longest : sums.longest;
  }
}

__global__ void __launch_bounds__(WIT_THREADS) witness_init_kernel(long long R, wit_out out, u64* __restrict__ counters) {
  const long long first = (long long)blockIdx.x * WIT_THREADS + threadIdx.x;
  if (first < N_COUNTERS) counters[first] = 0;
  for (long long g = first; g <= R; g += (long long)gridDim.x * WIT_THREADS) {
    out.span_first[g] = 0;
    out.cand_off[g] = 0;
    if (g < R) {
      out.span_text[g] = -1;
      out.span_start[g] = -1;
      out.span_len[g] = -1;
      out.cand_src[g] = -1;
      out.votes[g] = 0;
      out.votes[R + g] = 0;
    }
  }
}

template <bool PLACE>
__global__ void __launch_bounds__(WIT_THREADS) witness_sweep_kernel(
    const int* __restrict__ b_pool, long long n_b, const long long* __restrict__ b_off, long long P, int K,
    const int* __restrict__ dist, const int* __restrict__ n_spans, const int* __restrict__ spans,
    const long long* __restrict__ pair_first, const long long* __restrict__ text_off, long long n_texts, int join,
    long long* __restrict__ counts, wit_out out, u64* __restrict__ counters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wit_sums sums = {0, 0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * WIT_WAVES + wave; i < n_texts; i += (long long)gridDim.x * WIT_WAVES) {
    long long n_s, n_c, n_p;
    if (PLACE) {      // (counts hold the exclusive offsets now)
      sweep_text<true>(b_pool, n_b, b_off, P, K, dist, n_spans, spans, pair_first, text_off, join, i, counts[i],
                       counts[n_texts + i], counts[2 * n_texts + i], out, n_s, n_c, n_p, sums);
    } else {
      sweep_text<false>(b_pool, n_b, b_off, P, K, dist, n_spans, spans, pair_first, text_off, join, i, 0, 0, 0, out, n_s, n_c, n_p,
                        sums);
      if (lane == 0) {
        counts[i] = n_s;
        counts[n_texts + i] = n_c;
        counts[2 * n_texts + i] = n_p;
      }
    }
  }
  if (!PLACE && lane == 0) {
    if (sums.different) atomicAdd(&counters[DIFFERENT], (u64)sums.different);
    if (sums.first) atomicAdd(&counters[FIRST], (u64)sums.first);
    if (sums.too_long) atomicAdd(&counters[LONG], (u64)sums.too_long);
    if (sums.bad) atomicAdd(&counters[BAD], (u64)sums.bad);
    if (sums.longest) atomicMax(&counters[LONGEST], (u64)sums.longest);
  }
}

__global__ void __launch_bounds__(KL_RATE_SELECT_SCAN_THREADS) witness_offsets_kernel(long long* __restrict__ counts,
                                                                                      long long n_texts, u64* __restrict__ counters,
                                                                                      long long* __restrict__ span_first,
                                                                                      long long* __restrict__ cand_off,
                                                                                      long long* __restrict__ stats) {
  long long* __restrict__ total = reinterpret_cast<long long*>(counters + TOTALS);
  kl_counts_to_offsets(counts, n_texts, total);
  kl_counts_to_offsets(counts + n_texts, n_texts, total + 1);
  kl_counts_to_offsets(counts + 2 * n_texts, n_texts, total + 2);
  if (threadIdx.x == 0) {      // (the thread that wrote the totals)
    const long long S = total[0], C = total[1], n_pool = total[2];
    span_first[S] = C;
    cand_off[C] = n_pool;
    stats[0] = S;
    stats[1] = C;
    stats[2] = n_pool;
    stats[3] = (long long)counters[LONGEST];
    stats[4] = (long long)counters[DIFFERENT];
    stats[5] = (long long)counters[FIRST];
    stats[6] = (long long)counters[LONG];
    stats[7] = (long long)counters[BAD];
  }
}

__global__ void __launch_bounds__(WIT_THREADS) witness_pool_kernel(const int* __restrict__ b_ids, long long n_b,
                                                                   const long long* __restrict__ cand_src,
                                                                   const long long* __restrict__ cand_off, long long C,
                                                                   int* __restrict__ pool, long long n_pool) {
  for (long long g = (long long)blockIdx.x * WIT_THREADS + threadIdx.x; g < n_pool; g += (long long)gridDim.x * WIT_THREADS) {
    long long lo = 0, hi = C;      // the last c in [0, C) with cand_off[c] <= g (c = 0 if there is none)
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (cand_off[mid] <= g) lo = mid; else hi = mid;
    }
    const u64 at = (u64)cand_src[lo] + ((u64)g - (u64)cand_off[lo]);      // (modulo 2^64, as the statement's int64)
    pool[g] = at < (u64)n_b ? b_ids[at] : 0;
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

inline bool bad_shape(size_t P, int max_dist, size_t n_texts) {
  return P < 1 || P > MAX_PAIRS || max_dist < 1 || max_dist > KL_ALIGN_DIST_MAX || n_texts < 1 || n_texts > MAX_PAIRS;
}

}  // namespace

extern "C" size_t kl_witness_clusters_workspace_bytes(size_t P, int max_dist, size_t n_texts) {
  if (bad_shape(P, max_dist, n_texts)) return 0;
  return layout_of(n_texts).bytes;
}

extern "C" int kl_witness_clusters(const int32_t* b_pool, size_t n_b, const int64_t* b_off, size_t P, int max_dist,
                                   const int32_t* dist, const int32_t* n_spans, const int32_t* spans, const int64_t* pair_first,
                                   const int64_t* text_off, size_t n_texts, int join, int32_t* span_text, int64_t* span_start,
                                   int32_t* span_len, int64_t* span_first, int64_t* cand_src, int64_t* cand_off, int32_t* votes,
                                   int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!b_off || !dist || !n_spans || !spans || !pair_first || !text_off || !span_text || !span_start || !span_len || !span_first ||
      !cand_src || !cand_off || !votes || !stats || !ws || (n_b > 0 && !b_pool))
    return KL_ERR_ARG;
  if (bad_shape(P, max_dist, n_texts) || join < 0 || n_b > (size_t)1 << 40) return KL_ERR_ARG;
  const void* words[] = {b_pool, dist, n_spans, spans, span_text, span_len, votes};
  for (const void* p : words)
    if (misaligned(p, 3)) return KL_ERR_ARG;
  const void* longs[] = {b_off, pair_first, text_off, span_start, span_first, cand_src, cand_off, stats};
  for (const void* p : longs)
    if (misaligned(p, 7)) return KL_ERR_ARG;
  const wit_layout l = layout_of(n_texts);
  if (misaligned(ws, 7) || ws_bytes < l.bytes) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  u64* counters = reinterpret_cast<u64*>(base + l.counters);
  long long* counts = reinterpret_cast<long long*>(base + l.counts);
  const long long R = (long long)P * max_dist;
  const wit_out out = {span_text, reinterpret_cast<long long*>(span_start), span_len, reinterpret_cast<long long*>(span_first),
                       reinterpret_cast<long long*>(cand_src), reinterpret_cast<long long*>(cand_off), votes};
  const long long* b_offsets = reinterpret_cast<const long long*>(b_off);
  const long long* firsts = reinterpret_cast<const long long*>(pair_first);
  const long long* t_offsets = reinterpret_cast<const long long*>(text_off);
  const dim3 threads(WIT_THREADS), per_text(grid_for((long long)n_texts, WIT_WAVES));
  hipLaunchKernelGGL(witness_init_kernel, dim3(grid_for(R + 1, WIT_THREADS)), threads, 0, s, R, out, counters);
  hipLaunchKernelGGL(witness_sweep_kernel<false>, per_text, threads, 0, s, b_pool, (long long)n_b, b_offsets, (long long)P, max_dist,
                     dist, n_spans, spans, firsts, t_offsets, (long long)n_texts, join, counts, out, counters);
  hipLaunchKernelGGL(witness_offsets_kernel, dim3(1), dim3(KL_RATE_SELECT_SCAN_THREADS), 0, s, counts, (long long)n_texts, counters,
                     out.span_first, out.cand_off, reinterpret_cast<long long*>(stats));
  hipLaunchKernelGGL(witness_sweep_kernel<true>, per_text, threads, 0, s, b_pool, (long long)n_b, b_offsets, (long long)P, max_dist,
                     dist, n_spans, spans, firsts, t_offsets, (long long)n_texts, join, counts, out, counters);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_witness_pool(const int32_t* b_ids, size_t n_b, const int64_t* cand_src, const int64_t* cand_off, size_t C,
                               int32_t* pool, size_t n_pool, void* stream) {
  if (!cand_src || !cand_off || (n_b > 0 && !b_ids) || (n_pool > 0 && !pool)) return KL_ERR_ARG;
  if (C < 1 || C > (size_t)1 << 40 || n_b > (size_t)1 << 40 || n_pool > (size_t)1 << 40) return KL_ERR_ARG;
  if (misaligned(b_ids, 3) || misaligned(pool, 3) || misaligned(cand_src, 7) || misaligned(cand_off, 7)) return KL_ERR_ARG;
  if (n_pool == 0) return KL_OK;
  hipLaunchKernelGGL(witness_pool_kernel, dim3(grid_for((long long)n_pool, WIT_THREADS)), dim3(WIT_THREADS), 0,
                     static_cast<hipStream_t>(stream), b_ids, (long long)n_b, reinterpret_cast<const long long*>(cand_src),
                     reinterpret_cast<const long long*>(cand_off), (long long)C, pool, (long long)n_pool);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
