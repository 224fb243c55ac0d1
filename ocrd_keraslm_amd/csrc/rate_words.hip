// Word-level ratings over corpus-order rating results (kl_word_bounds, kl_rate_segments, kl_segment_select): where are the
// words of the texts, how does the model rate each of them, and which of them look wrong?
//
// Bulk rating leaves probs, rank, the id corpus and the text offsets on the device in corpus order.  Three steps on top of them:
//   kl_word_bounds     the tokeniser: an ordered compaction of the positions where a word starts (rate_select.hip's pattern:
//                      count per block, ONE workgroup turns counts into offsets, place).  Starts and ends alternate, so the end
//                      behind position j belongs to the last start at or in front of j: its index is the number of starts up to
//                      and including j, minus one -- one count per block serves both outputs;
//   kl_rate_segments   per segment n, bits, sum of probabilities, least probability and its place, suspect characters: a group
//                      of SEG_LANES lanes per segment (words average a handful of characters), every lane walks the segment in
//                      steps of SEG_LANES, the partial results are folded in a fixed butterfly;
//   kl_segment_select  the ordered compaction once more, over the records.
// No atomics, no workgroup waits for another, every order depends on indices only; 64-bit indices throughout.  No model: no
// handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_compact.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / KL_WAVE;
constexpr int SEL_ROUNDS = KL_RATE_SELECT_BLOCK / SEL_THREADS;
static_assert(SEL_ROUNDS * SEL_THREADS == KL_RATE_SELECT_BLOCK, "a block is a whole number of rounds");
constexpr int SEG_LANES = 16;
constexpr int SEG_PER_BLOCK = SEL_THREADS / SEG_LANES;
constexpr size_t MAX_ITEMS = (size_t)1 << 40;
constexpr size_t MAX_SEGMENTS = (size_t)1 << 32;      // (kl_rate_segments: SEG_PER_BLOCK segments per workgroup of one grid)

// the selected items of a workgroup's round r in the waves below this one, and in all of its waves
__device__ __forceinline__ void round_counts(const int (*wave_n)[SEL_WAVES], int r, int wave, int& before, int& all) {
  before = 0;
  all = 0;
#pragma unroll
  for (int w = 0; w < SEL_WAVES; ++w) {
    const int c = wave_n[r][w];
    before += w < wave ? c : 0;
    all += c;
  }
}

// a workgroup's count of selected items: the waves' counts folded through LDS
__device__ __forceinline__ void store_block_count(int c, long long* __restrict__ counts) {
  __shared__ int wave_n[SEL_WAVES];
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) all += wave_n[w];
    counts[blockIdx.x] = all;
  }
}

__global__ void __launch_bounds__(KL_RATE_SELECT_SCAN_THREADS) words_offsets_kernel(long long* __restrict__ counts,
                                                                                    long long n_blocks,
                                                                                    long long* __restrict__ total) {
  kl_counts_to_offsets(counts, n_blocks, total);
}

// ---------------------------------------------------------------------------------------------------- kl_word_bounds
// the texts of a corpus: lo = max(offsets[0], 0), hi = min(n_corpus, offsets[n_texts]) -- nothing outside [lo, hi) is read
struct corpus_view {
  const int* __restrict__ corpus;
  const long long* __restrict__ offsets;
  const unsigned char* __restrict__ delim;
  long long lo, hi;
  int n_texts, V;
};

__device__ __forceinline__ corpus_view view_of(const int* __restrict__ corpus, long long n_corpus,
                                               const long long* __restrict__ offsets, int n_texts,
                                               const unsigned char* __restrict__ delim, int V) {
  const long long first = offsets[0], last = offsets[n_texts];
  return corpus_view{corpus, offsets, delim, first > 0 ? first : 0, last < n_corpus ? last : n_corpus, n_texts, V};
}

__device__ __forceinline__ bool is_char(const corpus_view& c, long long j) {
  if (j < c.lo || j >= c.hi) return false;
  const int id = c.corpus[j];
  return !(id >= 0 && id < c.V && c.delim[id] != 0);
}

// bit 0: a word starts at j; bit 1: a word ends behind j
__device__ __forceinline__ int word_flags(const corpus_view& c, long long j) {
  if (!is_char(c, j)) return 0;
  // the text of j: the largest i with offsets[i] <= j.  offsets[0] <= lo <= j < hi <= offsets[n_texts], so 0 <= i < n_texts
  int a = 0, b = c.n_texts - 1;
  while (a < b) {
    const int m = a + ((b - a + 1) >> 1);
    if (c.offsets[m] <= j) a = m; else b = m - 1;
  }
  const bool start = c.offsets[a] == j || !is_char(c, j - 1);
  const bool end = j + 1 >= c.hi || c.offsets[a + 1] == j + 1 || !is_char(c, j + 1);
  return (start ? 1 : 0) | (end ? 2 : 0);
}

__global__ void __launch_bounds__(SEL_THREADS) word_count_kernel(const int* __restrict__ corpus, long long n_corpus,
                                                                  const long long* __restrict__ offsets, int n_texts,
                                                                  const unsigned char* __restrict__ delim, int V,
                                                                  long long* __restrict__ counts) {
  const corpus_view c = view_of(corpus, n_corpus, offsets, n_texts, delim, V);
  const long long base = (long long)blockIdx.x * KL_RATE_SELECT_BLOCK;
  int n = 0;
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) n += __popcll(__ballot(word_flags(c, base + r * SEL_THREADS + threadIdx.x) & 1));
  store_block_count(n, counts);
}

__global__ void __launch_bounds__(SEL_THREADS) word_place_kernel(const int* __restrict__ corpus, long long n_corpus,
                                                                  const long long* __restrict__ offsets, int n_texts,
                                                                  const unsigned char* __restrict__ delim, int V,
                                                                  long long capacity, const long long* __restrict__ block_at,
                                                                  long long* __restrict__ seg_start,
                                                                  long long* __restrict__ seg_end) {
  __shared__ int wave_n[SEL_ROUNDS][SEL_WAVES];
  const corpus_view c = view_of(corpus, n_corpus, offsets, n_texts, delim, V);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * KL_RATE_SELECT_BLOCK;
  int flags[SEL_ROUNDS];
  unsigned long long mask[SEL_ROUNDS];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    flags[r] = word_flags(c, base + r * SEL_THREADS + threadIdx.x);
    mask[r] = __ballot(flags[r] & 1);
    if (lane == 0) wave_n[r][wave] = __popcll(mask[r]);
  }
  __syncthreads();
  long long at = block_at[blockIdx.x];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    int before, all;
    round_counts(wave_n, r, wave, before, all);
    const long long j = base + r * SEL_THREADS + threadIdx.x;
    const long long starts = at + before + kl_lanes_before(mask[r]);      // the starts in front of j
    if ((flags[r] & 1) && starts < capacity) seg_start[starts] = j;
    const long long word = starts + (flags[r] & 1) - 1;                    // the word an end behind j closes
    if ((flags[r] & 2) && word >= 0 && word < capacity) seg_end[word] = j + 1;
    at += all;
  }
}

// ---------------------------------------------------------------------------------------------------- kl_rate_segments
__global__ void __launch_bounds__(SEL_THREADS) rate_segments_kernel(
    const float* __restrict__ probs, const int* __restrict__ rank, long long n, const long long* __restrict__ offsets,
    int n_texts, const long long* __restrict__ seg_start, const long long* __restrict__ seg_end, long long S, float max_prob,
    int min_rank, int* __restrict__ seg_n, double* __restrict__ seg_bits, double* __restrict__ seg_psum,
    uint32_t* __restrict__ seg_min, long long* __restrict__ seg_worst, int* __restrict__ seg_bad) {
  const int lane = threadIdx.x & (SEG_LANES - 1);
  const long long s = (long long)blockIdx.x * SEG_PER_BLOCK + threadIdx.x / SEG_LANES;
  long long lo = 0, hi = 0;      // the counted positions [lo, hi): none unless the segment starts inside a text
  if (s < S) {
    const long long a = seg_start[s], b = seg_end[s];
    if (a >= 0 && b >= a && a < n && offsets[0] <= a && a < offsets[n_texts]) {
      int x = 0, y = n_texts - 1;      // the largest i with offsets[i] <= a: offsets[i + 1] > a, empty texts are skipped
      while (x < y) {
        const int m = x + ((y - x + 1) >> 1);
        if (offsets[m] <= a) x = m; else y = m - 1;
      }
      const long long first = offsets[x] + 1, last = offsets[x + 1];
      lo = a > first ? a : first;
      hi = b < last ? b : last;
      hi = hi < n ? hi : n;
    }
  }
  double bits = 0.0, psum = 0.0;
  float least = __builtin_inff();
  long long worst = -1;
  int bad = 0;
  for (long long j = lo + lane; j < hi; j += SEG_LANES) {
    const float p = probs[j];
    bits -= log2(fmax((double)p, 1e-99));
    psum += (double)p;
    if (p < least) {
      least = p;
      worst = j;
    }
    if (rank != nullptr && rank[j] >= min_rank && p <= max_prob) ++bad;
  }
#pragma unroll
  for (int off = SEG_LANES / 2; off > 0; off >>= 1) {
    bits += __shfl_xor(bits, off, SEG_LANES);
    psum += __shfl_xor(psum, off, SEG_LANES);
    bad += __shfl_xor(bad, off, SEG_LANES);
    const float p = __shfl_xor(least, off, SEG_LANES);
    const long long j = __shfl_xor(worst, off, SEG_LANES);
    if (p < least || (p == least && j >= 0 && (worst < 0 || j < worst))) {
      least = p;
      worst = j;
    }
  }
  if (s < S && lane == 0) {
    seg_n[s] = hi > lo ? (int)(hi - lo) : 0;
    seg_bits[s] = bits;
    seg_psum[s] = psum;
    seg_min[s] = __float_as_uint(least);
    seg_worst[s] = worst;
    seg_bad[s] = bad;
  }
}

// ---------------------------------------------------------------------------------------------------- kl_segment_select
// the selection rule; the third comparison in f64: NaN bits compare false
__device__ __forceinline__ bool selected(const int* __restrict__ seg_n, const double* __restrict__ seg_bits,
                                         const int* __restrict__ seg_bad, long long s, long long S, int min_n, int min_bad,
                                         double min_bpc) {
  if (s >= S) return false;
  const int n = seg_n[s];
  return n >= min_n && seg_bad[s] >= min_bad && seg_bits[s] >= min_bpc * (double)n;
}

__global__ void __launch_bounds__(SEL_THREADS) segment_count_kernel(const int* __restrict__ seg_n,
                                                                     const double* __restrict__ seg_bits,
                                                                     const int* __restrict__ seg_bad, long long S, int min_n,
                                                                     int min_bad, double min_bpc,
                                                                     long long* __restrict__ counts) {
  const long long base = (long long)blockIdx.x * KL_RATE_SELECT_BLOCK;
  int c = 0;
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r)
    c += __popcll(__ballot(selected(seg_n, seg_bits, seg_bad, base + r * SEL_THREADS + threadIdx.x, S, min_n, min_bad, min_bpc)));
  store_block_count(c, counts);
}

__global__ void __launch_bounds__(SEL_THREADS) segment_place_kernel(
    const long long* __restrict__ seg_start, const long long* __restrict__ seg_end, const int* __restrict__ seg_n,
    const double* __restrict__ seg_bits, const double* __restrict__ seg_psum, const uint32_t* __restrict__ seg_min,
    const long long* __restrict__ seg_worst, const int* __restrict__ seg_bad, long long S, int min_n, int min_bad,
    double min_bpc, long long capacity, const long long* __restrict__ block_at, long long* __restrict__ sel_index,
    long long* __restrict__ sel_start, long long* __restrict__ sel_end, int* __restrict__ sel_n, double* __restrict__ sel_bits,
    double* __restrict__ sel_psum, uint32_t* __restrict__ sel_min, long long* __restrict__ sel_worst,
    int* __restrict__ sel_bad) {
  __shared__ int wave_n[SEL_ROUNDS][SEL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * KL_RATE_SELECT_BLOCK;
  bool flag[SEL_ROUNDS];
  unsigned long long mask[SEL_ROUNDS];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    flag[r] = selected(seg_n, seg_bits, seg_bad, base + r * SEL_THREADS + threadIdx.x, S, min_n, min_bad, min_bpc);
    mask[r] = __ballot(flag[r]);
    if (lane == 0) wave_n[r][wave] = __popcll(mask[r]);
  }
  __syncthreads();
  long long at = block_at[blockIdx.x];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    int before, all;
    round_counts(wave_n, r, wave, before, all);
    const long long to = at + before + kl_lanes_before(mask[r]);
    if (flag[r] && to < capacity) {
      const long long s = base + r * SEL_THREADS + threadIdx.x;
      sel_index[to] = s;
      sel_start[to] = seg_start[s];
      sel_end[to] = seg_end[s];
      sel_n[to] = seg_n[s];
      sel_bits[to] = seg_bits[s];
      sel_psum[to] = seg_psum[s];
      sel_min[to] = seg_min[s];
      sel_worst[to] = seg_worst[s];
      sel_bad[to] = seg_bad[s];
    }
    at += all;
  }
}

inline long long blocks_of(size_t n) { return (long long)((n + KL_RATE_SELECT_BLOCK - 1) / KL_RATE_SELECT_BLOCK); }
inline size_t counts_bytes(size_t n) { return ((size_t)(n ? blocks_of(n) : 1) * sizeof(long long) + 255) / 256 * 256; }
inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

}  // namespace

extern "C" size_t kl_word_bounds_workspace_bytes(size_t n_corpus, int n_texts) {
  if (n_corpus > MAX_ITEMS || n_texts < 1) return 0;
  return counts_bytes(n_corpus);
}

extern "C" int kl_word_bounds(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts, const uint8_t* delim,
                              int V, size_t capacity, int64_t* seg_start, int64_t* seg_end, int64_t* count, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!corpus || !offsets || !delim || !count || !ws) return KL_ERR_ARG;
  if (n_texts < 1 || V < 1 || n_corpus > MAX_ITEMS || capacity > MAX_ITEMS) return KL_ERR_ARG;
  if (capacity > 0 && (!seg_start || !seg_end)) return KL_ERR_ARG;
  if (misaligned(corpus, 3) || misaligned(offsets, 7) || misaligned(seg_start, 7) || misaligned(seg_end, 7) ||
      misaligned(count, 7) || misaligned(ws, 7))
    return KL_ERR_ARG;
  if (ws_bytes < kl_word_bounds_workspace_bytes(n_corpus, n_texts)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n_blocks = blocks_of(n_corpus);
  long long* counts = reinterpret_cast<long long*>(ws);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  if (n_blocks > 0)
    hipLaunchKernelGGL(word_count_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, s, corpus, (long long)n_corpus, off,
                       n_texts, delim, V, counts);
  hipLaunchKernelGGL(words_offsets_kernel, dim3(1), dim3(KL_RATE_SELECT_SCAN_THREADS), 0, s, counts, n_blocks,
                     reinterpret_cast<long long*>(count));
  if (capacity > 0 && n_blocks > 0)      // (the counting call ends here: nothing to place)
    hipLaunchKernelGGL(word_place_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, s, corpus, (long long)n_corpus, off,
                       n_texts, delim, V, (long long)capacity, counts, reinterpret_cast<long long*>(seg_start),
                       reinterpret_cast<long long*>(seg_end));
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_rate_segments(const float* probs, const int32_t* rank, size_t n, const int64_t* offsets, int n_texts,
                                const int64_t* seg_start, const int64_t* seg_end, size_t S, float max_prob, int min_rank,
                                int32_t* seg_n, double* seg_bits, double* seg_psum, float* seg_min, int64_t* seg_worst,
                                int32_t* seg_bad, void* stream) {
  if (!probs || !offsets || !seg_start || !seg_end || !seg_n || !seg_bits || !seg_psum || !seg_min || !seg_worst || !seg_bad)
    return KL_ERR_ARG;
  if (S < 1 || S > MAX_SEGMENTS || n_texts < 1 || n > MAX_ITEMS) return KL_ERR_ARG;
  if (min_rank < 0 || max_prob != max_prob) return KL_ERR_ARG;
  if (misaligned(probs, 3) || misaligned(rank, 3) || misaligned(seg_n, 3) || misaligned(seg_min, 3) || misaligned(seg_bad, 3) ||
      misaligned(offsets, 7) || misaligned(seg_start, 7) || misaligned(seg_end, 7) || misaligned(seg_bits, 7) ||
      misaligned(seg_psum, 7) || misaligned(seg_worst, 7))
    return KL_ERR_ARG;
  const unsigned n_blocks = (unsigned)((S + SEG_PER_BLOCK - 1) / SEG_PER_BLOCK);
  hipLaunchKernelGGL(rate_segments_kernel, dim3(n_blocks), dim3(SEL_THREADS), 0, static_cast<hipStream_t>(stream), probs, rank,
                     (long long)n, reinterpret_cast<const long long*>(offsets), n_texts,
                     reinterpret_cast<const long long*>(seg_start), reinterpret_cast<const long long*>(seg_end), (long long)S,
                     max_prob, min_rank, seg_n, seg_bits, seg_psum, reinterpret_cast<uint32_t*>(seg_min),
                     reinterpret_cast<long long*>(seg_worst), seg_bad);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" size_t kl_segment_select_workspace_bytes(size_t S) {
  if (S < 1 || S > MAX_ITEMS) return 0;
  return counts_bytes(S);
}

extern "C" int kl_segment_select(const int64_t* seg_start, const int64_t* seg_end, const int32_t* seg_n, const double* seg_bits,
                                 const double* seg_psum, const float* seg_min, const int64_t* seg_worst, const int32_t* seg_bad,
                                 size_t S, int min_n, int min_bad, double min_bpc, size_t capacity, int64_t* sel_index,
                                 int64_t* sel_start, int64_t* sel_end, int32_t* sel_n, double* sel_bits, double* sel_psum,
                                 float* sel_min, int64_t* sel_worst, int32_t* sel_bad, int64_t* count, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (!seg_start || !seg_end || !seg_n || !seg_bits || !seg_psum || !seg_min || !seg_worst || !seg_bad || !count || !ws)
    return KL_ERR_ARG;
  if (S < 1 || S > MAX_ITEMS || capacity > MAX_ITEMS) return KL_ERR_ARG;
  if (min_n < 1 || min_bad < 0 || !(min_bpc >= 0.0)) return KL_ERR_ARG;
  if (capacity > 0 &&
      (!sel_index || !sel_start || !sel_end || !sel_n || !sel_bits || !sel_psum || !sel_min || !sel_worst || !sel_bad))
    return KL_ERR_ARG;
  const void* words[] = {seg_n, seg_min, seg_bad, sel_n, sel_min, sel_bad};
  for (const void* p : words)
    if (misaligned(p, 3)) return KL_ERR_ARG;
  const void* doubles[] = {seg_start, seg_end, seg_bits, seg_psum, seg_worst, sel_index, sel_start, sel_end,
                           sel_bits,  sel_psum, sel_worst, count,   ws};
  for (const void* p : doubles)
    if (misaligned(p, 7)) return KL_ERR_ARG;
  if (ws_bytes < kl_segment_select_workspace_bytes(S)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n_blocks = blocks_of(S);
  long long* counts = reinterpret_cast<long long*>(ws);
  hipLaunchKernelGGL(segment_count_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, s, seg_n, seg_bits, seg_bad,
                     (long long)S, min_n, min_bad, min_bpc, counts);
  hipLaunchKernelGGL(words_offsets_kernel, dim3(1), dim3(KL_RATE_SELECT_SCAN_THREADS), 0, s, counts, n_blocks,
                     reinterpret_cast<long long*>(count));
  if (capacity > 0)      // (the counting call ends here: nothing to place)
    hipLaunchKernelGGL(segment_place_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, s,
                       reinterpret_cast<const long long*>(seg_start), reinterpret_cast<const long long*>(seg_end), seg_n,
                       seg_bits, seg_psum, reinterpret_cast<const uint32_t*>(seg_min),
                       reinterpret_cast<const long long*>(seg_worst), seg_bad, (long long)S, min_n, min_bad, min_bpc,
                       (long long)capacity, counts, reinterpret_cast<long long*>(sel_index),
                       reinterpret_cast<long long*>(sel_start), reinterpret_cast<long long*>(sel_end), sel_n, sel_bits,
                       sel_psum, reinterpret_cast<uint32_t*>(sel_min), reinterpret_cast<long long*>(sel_worst), sel_bad);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
