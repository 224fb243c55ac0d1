// Confusion counts (kl_confusion_counts): from the differing spans kl_align_pairs left on the device to the table of distinct
// (source, target) records with how often each was read and how often its source stands in the OCR texts at all.
//
// N = P * max_dist span slots, g = p * max_dist + s.  Eight plain launches on the stream, every loop grid-stride:
//   0. confusion_init_kernel      the two tables EMPTY, their counts and the call's counters 0
//   1. confusion_records_kernel   one lane per span slot: the 40-byte record (src_len, tgt_len, src[4], tgt[4]) after anchoring
//                                 at rec[10 g ..], or 0 in its first word for none; counted / long / empty through ballots per
//                                 wave, LDS per workgroup and ONE integer atomic per workgroup and reason
//   2. confusion_insert_kernel    one lane per record: open addressing, linear probing, a slot holds the span id of a
//                                 representative.  atomicCAS claims an empty slot; otherwise the lane compares ITS record with
//                                 the representative's -- both written by launch 1 -- and lowers the representative with
//                                 atomicMin and adds to the slot's count, or probes on.  A slot once claimed keeps its record
//                                 (only equal records replace each other), so the first slot of a record's probe sequence that
//                                 is empty or its own is the same for all of its lanes whenever they arrive; nothing is
//                                 published and read within the kernel, no lane waits for another.  slot_of[g] is the lane's own
//   3. confusion_count_kernel, confusion_offsets_kernel, confusion_place_kernel: kl_compact.h's ordered compaction of the spans
//                                 that ARE their slot's representative (the least span id of a record): the order of first
//                                 occurrence, whatever the order of arrival.  A placed lane below `room` copies record and count,
//                                 puts its source into the second table (same scheme, no count) and leaves the source's slot in
//                                 occ[row]: scratch of the output's own, replaced by launch 5
//   4. confusion_walk_kernel      one wave per accepted pair, one lane per position and length 1 .. max_chars within the text:
//                                 look the source up (read only: the table is complete), lanes of a wave that hit the same slot
//                                 add once (a ballot per distinct slot), one integer atomic each
//   5. confusion_finish_kernel    occ[row] = the count of its source's slot, -1 / 0 / 0 behind the R-th row, stats
// All atomics are integer atomics on global memory: sums and minima do not depend on the order of arrival, so the outputs depend on
// the inputs only (where a record sits in a table does not, and is never shown).  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_compact.h"

namespace {

typedef unsigned long long u64;

constexpr int CONF_THREADS = 256;
constexpr int CONF_WAVES = CONF_THREADS / KL_WAVE;
constexpr int CONF_ROUNDS = KL_RATE_SELECT_BLOCK / CONF_THREADS;
constexpr long long CONF_GRID_MAX = 1024;       // workgroups of a launch with one item per lane at most
constexpr long long CONF_BLOCK_GRID_MAX = 256;  // ... and with KL_RATE_SELECT_BLOCK items per workgroup: as many items per sweep
constexpr int REC_WORDS = 2 + 2 * KL_CONFUSION_CHARS_MAX;
constexpr u64 EMPTY = ~0ull;
constexpr size_t MAX_PAIRS = 0x7FFFFFFF;
enum { COUNTED = 0, LONG = 1, NO_SOURCE = 2, DISTINCT = 3, N_COUNTERS = 8 };
static_assert(CONF_ROUNDS * CONF_THREADS == KL_RATE_SELECT_BLOCK, "a block is a whole number of rounds");
static_assert(CONF_GRID_MAX * CONF_THREADS == CONF_BLOCK_GRID_MAX * KL_RATE_SELECT_BLOCK, "one sweep of either grid");
static_assert(KL_CONFUSION_CHARS_MAX == 4, "the walk keeps a position's four symbols in registers");

// the workspace: everything 256-byte aligned
struct conf_layout {
  long long N, T, n_blocks;      // span slots, slots of a table (a power of two >= 2 N), blocks of the compaction
  size_t counters, counts, rec, slot_of, tab1, cnt1, tab2, cnt2, bytes;
};

inline size_t padded(size_t bytes) { return (bytes + 255) / 256 * 256; }

inline conf_layout layout_of(size_t P, int max_dist) {
  conf_layout l;
  l.N = (long long)P * max_dist;
  l.T = 64;
  while (l.T < 2 * l.N) l.T *= 2;
  l.n_blocks = (l.N + KL_RATE_SELECT_BLOCK - 1) / KL_RATE_SELECT_BLOCK;
  size_t at = 0;
  l.counters = at, at += padded(N_COUNTERS * 8);
  l.counts = at, at += padded((size_t)l.n_blocks * 8);
  l.rec = at, at += padded((size_t)l.N * REC_WORDS * 4);
  l.slot_of = at, at += padded((size_t)l.N * 8);
  l.tab1 = at, at += padded((size_t)l.T * 8);
  l.cnt1 = at, at += padded((size_t)l.T * 8);
  l.tab2 = at, at += padded((size_t)l.T * 8);
  l.cnt2 = at, at += padded((size_t)l.T * 8);
  l.bytes = at;
  return l;
}

inline unsigned grid_for(long long items, long long per_block, long long most) {
  const long long blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : blocks < most ? blocks : most);
}

__device__ __forceinline__ u64 mixed(u64 h, int word) {
  h = (h ^ (unsigned)word) * 0xff51afd7ed558ccdull;
  return h ^ (h >> 29);
}

// where the probing of a source starts: its length and its symbols, the unused places 0
__device__ __forceinline__ u64 source_hash(int len, int s0, int s1, int s2, int s3) {
  return mixed(mixed(mixed(mixed(mixed(0x9e3779b97f4a7c15ull, len), s0), s1), s2), s3);
}

// ... and of a record: all ten words
__device__ __forceinline__ u64 record_hash(const int* __restrict__ r) {
  u64 h = 0xc2b2ae3d27d4eb4full;
#pragma unroll
  for (int w = 0; w < REC_WORDS; ++w) h = mixed(h, r[w]);
  return h;
}

__device__ __forceinline__ bool same_record(const int* __restrict__ x, const int* __restrict__ y) {
  bool same = true;
#pragma unroll
  for (int w = 0; w < REC_WORDS; ++w) same = same && x[w] == y[w];
  return same;
}

__device__ __forceinline__ bool has_source(const int* __restrict__ r, int len, int s0, int s1, int s2, int s3) {
  return r[0] == len && r[2] == s0 && r[3] == s1 && r[4] == s2 && r[5] == s3;
}

// the texts of pair p, if it was aligned and its offsets lie inside the pools in ascending order
__device__ __forceinline__ bool accepted_pair(long long p, const long long* __restrict__ a_off, long long n_a,
                                              const long long* __restrict__ b_off, long long n_b, const int* __restrict__ dist,
                                              long long& a_lo, long long& n, long long& b_lo, long long& m) {
  if (dist[p] < 0) return false;
  const long long a_hi = a_off[p + 1], b_hi = b_off[p + 1];
  a_lo = a_off[p];
  b_lo = b_off[p];
  if (a_lo < 0 || a_hi < a_lo || a_hi > n_a || b_lo < 0 || b_hi < b_lo || b_hi > n_b) return false;
  n = a_hi - a_lo;
  m = b_hi - b_lo;
  return true;
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_init_kernel(u64* __restrict__ counters, u64* __restrict__ tab1,
                                                                       u64* __restrict__ cnt1, u64* __restrict__ tab2,
                                                                       u64* __restrict__ cnt2, long long T) {
  const long long first = (long long)blockIdx.x * CONF_THREADS + threadIdx.x;
  if (first < N_COUNTERS) counters[first] = 0;
  for (long long h = first; h < T; h += (long long)gridDim.x * CONF_THREADS) {
    tab1[h] = EMPTY;
    cnt1[h] = 0;
    tab2[h] = EMPTY;
    cnt2[h] = 0;
  }
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_records_kernel(
    const int* __restrict__ a_pool, long long n_a, const long long* __restrict__ a_off, const int* __restrict__ b_pool,
    long long n_b, const long long* __restrict__ b_off, long long N, int K, const int* __restrict__ dist,
    const int* __restrict__ n_spans, const int* __restrict__ spans, int max_chars, int* __restrict__ rec,
    u64* __restrict__ counters) {
  __shared__ int wave_n[3][CONF_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int seen[3] = {0, 0, 0};      // (wave-uniform: the loop is the workgroup's)
  for (long long g0 = (long long)blockIdx.x * CONF_THREADS; g0 < N; g0 += (long long)gridDim.x * CONF_THREADS) {
    const long long g = g0 + threadIdx.x;
    int kind = -1;
    if (g < N) {
      const long long p = g / K;
      const int s = (int)(g - p * K);
      long long a_lo = 0, n = 0, b_lo = 0, m = 0;
      int src_len = 0;
      if (accepted_pair(p, a_off, n_a, b_off, n_b, dist, a_lo, n, b_lo, m) && s < n_spans[p]) {
        const int a0 = spans[g * 4 + 0], a1 = spans[g * 4 + 1], b0 = spans[g * 4 + 2], b1 = spans[g * 4 + 3];
        long long s0 = a0, s1 = a1, t0 = b0, t1 = b1;
        bool inside = a0 >= 0 && a1 >= a0 && a1 <= n && b0 >= 0 && b1 >= b0 && b1 <= m;
        kind = COUNTED;
        if (inside && a1 == a0) {
          if (a0 > 0) {              // the OCR lost characters: anchored on the character in front
            s0 = a0 - 1, t0 = t0 - 1;
            inside = b0 > 0;
          } else if (n > 0) {        // ... at the text's beginning: on the one behind
            s1 = 1, t0 = 0, t1 = t1 + 1;
            inside = t1 <= m;
          } else {
            kind = NO_SOURCE;
          }
        }
        if (kind == COUNTED && (!inside || s1 - s0 > max_chars || t1 - t0 > max_chars)) kind = LONG;
        if (kind == COUNTED) {
          src_len = (int)(s1 - s0);
          const int tgt_len = (int)(t1 - t0);
          int* __restrict__ mine = rec + g * REC_WORDS;
          mine[1] = tgt_len;
#pragma unroll
          for (int c = 0; c < KL_CONFUSION_CHARS_MAX; ++c) {
            mine[2 + c] = c < src_len ? a_pool[a_lo + s0 + c] : 0;
            mine[2 + KL_CONFUSION_CHARS_MAX + c] = c < tgt_len ? b_pool[b_lo + t0 + c] : 0;
          }
        }
      }
      rec[g * REC_WORDS] = src_len;      // 0: no record
    }
#pragma unroll
    for (int reason = 0; reason < 3; ++reason) seen[reason] += __popcll(__ballot(kind == reason));
  }
  if (lane == 0)
    for (int reason = 0; reason < 3; ++reason) wave_n[reason][wave] = seen[reason];
  __syncthreads();
  if (threadIdx.x < 3) {
    int all = 0;
#pragma unroll
    for (int w = 0; w < CONF_WAVES; ++w) all += wave_n[threadIdx.x][w];
    if (all) atomicAdd(&counters[threadIdx.x], (u64)all);
  }
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_insert_kernel(const int* __restrict__ rec, long long N, long long T,
                                                                         u64* tab1, u64* cnt1, long long* __restrict__ slot_of) {
  const u64 mask = (u64)T - 1;
  for (long long g = (long long)blockIdx.x * CONF_THREADS + threadIdx.x; g < N; g += (long long)gridDim.x * CONF_THREADS) {
    const int* __restrict__ mine = rec + g * REC_WORDS;
    if (mine[0] <= 0) continue;
    u64 h = record_hash(mine) & mask;
    for (;;) {      // (at most N of the T >= 2 N slots are ever taken: an empty one comes)
      const u64 held = atomicCAS(&tab1[h], EMPTY, (u64)g);
      if (held == EMPTY) break;
      if (same_record(mine, rec + held * REC_WORDS)) {
        atomicMin(&tab1[h], (u64)g);
        break;
      }
      h = (h + 1) & mask;
    }
    atomicAdd(&cnt1[h], 1ull);
    slot_of[g] = (long long)h;
  }
}

// is span slot g the representative of its record: the first span that gave it
__device__ __forceinline__ bool is_first(const int* __restrict__ rec, const long long* __restrict__ slot_of,
                                         const u64* __restrict__ tab1, long long g, long long N) {
  return g < N && rec[g * REC_WORDS] > 0 && tab1[slot_of[g]] == (u64)g;
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_count_kernel(const int* __restrict__ rec,
                                                                        const long long* __restrict__ slot_of,
                                                                        const u64* __restrict__ tab1, long long N,
                                                                        long long n_blocks, long long* __restrict__ counts) {
  __shared__ int wave_n[CONF_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long block = blockIdx.x; block < n_blocks; block += gridDim.x) {
    const long long base = block * KL_RATE_SELECT_BLOCK;
    int c = 0;
#pragma unroll
    for (int r = 0; r < CONF_ROUNDS; ++r) c += __popcll(__ballot(is_first(rec, slot_of, tab1, base + r * CONF_THREADS + threadIdx.x, N)));
    if (lane == 0) wave_n[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      int all = 0;
#pragma unroll
      for (int w = 0; w < CONF_WAVES; ++w) all += wave_n[w];
      counts[block] = all;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(KL_RATE_SELECT_SCAN_THREADS) confusion_offsets_kernel(long long* __restrict__ counts,
                                                                                        long long n_blocks,
                                                                                        long long* __restrict__ total) {
  kl_counts_to_offsets(counts, n_blocks, total);
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_place_kernel(
    const int* __restrict__ rec, const long long* __restrict__ slot_of, const u64* __restrict__ tab1,
    const u64* __restrict__ cnt1, long long N, long long n_blocks, long long T, const long long* __restrict__ offsets,
    long long room, u64* tab2, int* __restrict__ rules, long long* __restrict__ count, long long* __restrict__ occ) {
  __shared__ int wave_n[CONF_ROUNDS][CONF_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 mask_T = (u64)T - 1;
  for (long long block = blockIdx.x; block < n_blocks; block += gridDim.x) {
    const long long base = block * KL_RATE_SELECT_BLOCK;
    bool flag[CONF_ROUNDS];
    unsigned long long mask[CONF_ROUNDS];
#pragma unroll
    for (int r = 0; r < CONF_ROUNDS; ++r) {
      flag[r] = is_first(rec, slot_of, tab1, base + r * CONF_THREADS + threadIdx.x, N);
      mask[r] = __ballot(flag[r]);
      if (lane == 0) wave_n[r][wave] = __popcll(mask[r]);
    }
    __syncthreads();
    long long at = offsets[block];
#pragma unroll
    for (int r = 0; r < CONF_ROUNDS; ++r) {
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < CONF_WAVES; ++w) {
        const int c = wave_n[r][w];
        before += w < wave ? c : 0;
        all += c;
      }
      const long long to = at + before + kl_lanes_before(mask[r]);
      if (flag[r] && to < room) {
        const long long g = base + r * CONF_THREADS + threadIdx.x;
        const int* __restrict__ mine = rec + g * REC_WORDS;
#pragma unroll
        for (int w = 0; w < REC_WORDS; ++w) rules[to * REC_WORDS + w] = mine[w];
        count[to] = (long long)cnt1[slot_of[g]];
        u64 h = source_hash(mine[0], mine[2], mine[3], mine[4], mine[5]) & mask_T;
        for (;;) {      // the source's slot: claimed, or found under a span with the same source
          const u64 held = atomicCAS(&tab2[h], EMPTY, (u64)g);
          if (held == EMPTY || has_source(rec + held * REC_WORDS, mine[0], mine[2], mine[3], mine[4], mine[5])) break;
          h = (h + 1) & mask_T;
        }
        occ[to] = (long long)h;      // (until confusion_finish_kernel puts the slot's count here)
      }
      at += all;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_walk_kernel(
    const int* __restrict__ a_pool, long long n_a, const long long* __restrict__ a_off, long long n_b,
    const long long* __restrict__ b_off, long long P, const int* __restrict__ dist, int max_chars, const int* __restrict__ rec,
    const u64* __restrict__ tab2, u64* cnt2, long long T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 mask_T = (u64)T - 1;
  for (long long p = (long long)blockIdx.x * CONF_WAVES + wave; p < P; p += (long long)gridDim.x * CONF_WAVES) {
    long long a_lo = 0, n = 0, b_lo = 0, m = 0;
    if (!accepted_pair(p, a_off, n_a, b_off, n_b, dist, a_lo, n, b_lo, m)) continue;      // (the wave's pair: uniform)
    for (long long x0 = 0; x0 < n; x0 += KL_WAVE) {
      const long long i = x0 + lane;
      int s[KL_CONFUSION_CHARS_MAX] = {0, 0, 0, 0};
#pragma unroll
      for (int len = 1; len <= KL_CONFUSION_CHARS_MAX; ++len) {
        if (len > max_chars) break;
        long long slot = -1;
        if (i + len <= n) {      // a source never reaches across the text's end
          s[len - 1] = a_pool[a_lo + i + len - 1];
          u64 h = source_hash(len, s[0], s[1], s[2], s[3]) & mask_T;
          for (;;) {
            const u64 held = tab2[h];
            if (held == EMPTY) break;
            if (has_source(rec + held * REC_WORDS, len, s[0], s[1], s[2], s[3])) {
              slot = (long long)h;
              break;
            }
            h = (h + 1) & mask_T;
          }
        }
        unsigned long long todo = __ballot(slot >= 0);
        while (todo) {      // one add per distinct slot of the wave
          const int leader = __ffsll(todo) - 1;
          const long long its = __shfl(slot, leader);
          const unsigned long long same = __ballot(slot == its);
          if (lane == leader) atomicAdd(&cnt2[its], (u64)__popcll(same));
          todo &= ~same;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(CONF_THREADS) confusion_finish_kernel(const u64* __restrict__ counters,
                                                                         const long long* __restrict__ total,
                                                                         const u64* __restrict__ cnt2, long long room,
                                                                         int* __restrict__ rules, long long* __restrict__ count,
                                                                         long long* __restrict__ occ, long long* __restrict__ stats) {
  const long long R = total[0];
  const long long first = (long long)blockIdx.x * CONF_THREADS + threadIdx.x;
  if (first == 0) {
    stats[0] = R;
    stats[1] = (long long)counters[COUNTED];
    stats[2] = (long long)counters[LONG];
    stats[3] = (long long)counters[NO_SOURCE];
  }
  for (long long row = first; row < room; row += (long long)gridDim.x * CONF_THREADS) {
    if (row < R) {
      occ[row] = (long long)cnt2[occ[row]];
    } else {
#pragma unroll
      for (int w = 0; w < REC_WORDS; ++w) rules[row * REC_WORDS + w] = -1;
      count[row] = 0;
      occ[row] = 0;
    }
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

inline bool bad_shape(size_t P, int max_dist, size_t n_a) {
  return P < 1 || P > MAX_PAIRS || max_dist < 1 || max_dist > KL_ALIGN_DIST_MAX || n_a > (size_t)1 << 40;
}

}  // namespace

extern "C" size_t kl_confusion_counts_workspace_bytes(size_t P, int max_dist, size_t n_a) {
  if (bad_shape(P, max_dist, n_a)) return 0;
  return layout_of(P, max_dist).bytes;
}

extern "C" int kl_confusion_counts(const int32_t* a_pool, size_t n_a, const int64_t* a_off, const int32_t* b_pool, size_t n_b,
                                   const int64_t* b_off, size_t P, int max_dist, const int32_t* dist, const int32_t* n_spans,
                                   const int32_t* spans, int max_chars, size_t room, int32_t* rules, int64_t* count, int64_t* occ,
                                   int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!a_off || !b_off || !dist || !n_spans || !spans || !rules || !count || !occ || !stats || !ws) return KL_ERR_ARG;
  if ((n_a > 0 && !a_pool) || (n_b > 0 && !b_pool)) return KL_ERR_ARG;
  if (bad_shape(P, max_dist, n_a) || n_b > (size_t)1 << 40 || max_chars < 1 || max_chars > KL_CONFUSION_CHARS_MAX || room < 1 ||
      room > (size_t)1 << 40)
    return KL_ERR_ARG;
  const void* words[] = {a_pool, b_pool, dist, n_spans, spans, rules};
  for (const void* p : words)
    if (misaligned(p, 3)) return KL_ERR_ARG;
  const void* longs[] = {a_off, b_off, count, occ, stats};
  for (const void* p : longs)
    if (misaligned(p, 7)) return KL_ERR_ARG;
  const conf_layout l = layout_of(P, max_dist);
  if (misaligned(ws, 7) || ws_bytes < l.bytes) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  u64* counters = reinterpret_cast<u64*>(base + l.counters);
  long long* counts = reinterpret_cast<long long*>(base + l.counts);
  int* rec = reinterpret_cast<int*>(base + l.rec);
  long long* slot_of = reinterpret_cast<long long*>(base + l.slot_of);
  u64* tab1 = reinterpret_cast<u64*>(base + l.tab1);
  u64* cnt1 = reinterpret_cast<u64*>(base + l.cnt1);
  u64* tab2 = reinterpret_cast<u64*>(base + l.tab2);
  u64* cnt2 = reinterpret_cast<u64*>(base + l.cnt2);
  long long* total = reinterpret_cast<long long*>(counters + DISTINCT);
  const long long* a_offsets = reinterpret_cast<const long long*>(a_off);
  const long long* b_offsets = reinterpret_cast<const long long*>(b_off);
  const dim3 threads(CONF_THREADS), per_slot(grid_for(l.N, CONF_THREADS, CONF_GRID_MAX)),
      per_block(grid_for(l.n_blocks, 1, CONF_BLOCK_GRID_MAX));
  hipLaunchKernelGGL(confusion_init_kernel, dim3(grid_for(l.T, CONF_THREADS, CONF_GRID_MAX)), threads, 0, s, counters, tab1, cnt1,
                     tab2, cnt2, l.T);
  hipLaunchKernelGGL(confusion_records_kernel, per_slot, threads, 0, s, a_pool, (long long)n_a, a_offsets, b_pool, (long long)n_b,
                     b_offsets, l.N, max_dist, dist, n_spans, spans, max_chars, rec, counters);
  hipLaunchKernelGGL(confusion_insert_kernel, per_slot, threads, 0, s, rec, l.N, l.T, tab1, cnt1, slot_of);
  hipLaunchKernelGGL(confusion_count_kernel, per_block, threads, 0, s, rec, slot_of, tab1, l.N, l.n_blocks, counts);
  hipLaunchKernelGGL(confusion_offsets_kernel, dim3(1), dim3(KL_RATE_SELECT_SCAN_THREADS), 0, s, counts, l.n_blocks, total);
  hipLaunchKernelGGL(confusion_place_kernel, per_block, threads, 0, s, rec, slot_of, tab1, cnt1, l.N, l.n_blocks, l.T, counts,
                     (long long)room, tab2, rules, reinterpret_cast<long long*>(count), reinterpret_cast<long long*>(occ));
  hipLaunchKernelGGL(confusion_walk_kernel, dim3(grid_for((long long)P, CONF_WAVES, CONF_GRID_MAX)), threads, 0, s, a_pool,
                     (long long)n_a, a_offsets, (long long)n_b, b_offsets, (long long)P, dist, max_chars, rec, tab2, cnt2, l.T);
  hipLaunchKernelGGL(confusion_finish_kernel, dim3(grid_for((long long)room, CONF_THREADS, CONF_GRID_MAX)), threads, 0, s, counters,
                     total, cnt2, (long long)room, rules, reinterpret_cast<long long*>(count), reinterpret_cast<long long*>(occ),
                     reinterpret_cast<long long*>(stats));
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
