// Alignment of two readings (kl_align_pairs): where do the texts of a pair differ, within a band of max_dist edits?
//
// One workgroup per pair, a grid-stride loop over the pairs.  The band |i - j| <= K = max_dist has L = 2 K + 1 diagonals and lane
// k owns diagonal j - i = k - K.  The workgroup walks the anti-diagonals t = i + j = 0 .. n + m: on t the lanes with
// t - k + K = 2 i even hold a cell, so neighbouring lanes alternate.  A cell needs D[i-1][j-1] -- the lane's own last value, a
// register --, D[i-1][j] -- lane k + 1 on t - 1 -- and D[i][j-1] -- lane k - 1 on t - 1: one LDS word per lane, written by
// the lanes of one parity while the others read, hence one barrier per anti-diagonal and a single row of values.  Beyond the
// band stands ALIGN_INF.  Both texts lie in LDS before the first anti-diagonal.
//
// What the walk back needs is the rule of the statement that applies at a cell (match, substitution, deletion, insertion): two
// bits.  A lane packs the bits of 16 successive rows of ITS diagonal into a word of its own -- no two lanes share a word, so
// nothing is read back and nothing is atomic -- and stores word r / 16 of lane k at [(r / 16) * L + k]: in LDS while
// (n / 16 + 1) * L words fit the share the launch set aside, else in the workgroup's own slice of the workspace.  Every word the
// walk reads was stored whole by the same pair, so scratch left by an earlier pair never shows.  Lane 0 walks back from (n, m),
// closes the spans in descending order in LDS, and the workgroup writes them out ascending with the -1 fill behind.
//
// No atomics, no workgroup waits for another, the output depends on the inputs only.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"

namespace {

constexpr int ALIGN_THREADS_MAX = 512;      // 2 * KL_ALIGN_DIST_MAX + 1 lanes, in whole waves
constexpr int ALIGN_GRID_MAX = 512;         // workgroups of a launch at most (two per CU): what the workspace is sized by
constexpr int ALIGN_LDS_CELL_WORDS = 6144;  // words of two-bit cells a workgroup keeps in LDS at most (24 KiB)
constexpr int ALIGN_INF = 1 << 20;          // a value beyond the band (a true one is at most 2 * KL_ALIGN_LEN_MAX)
constexpr size_t MAX_PAIRS = 0x7FFFFFFF;
constexpr int OP_MATCH = 0, OP_SUBST = 1, OP_DELETE = 2, OP_INSERT = 3;
static_assert(2 * KL_ALIGN_DIST_MAX + 1 <= ALIGN_THREADS_MAX, "one lane per diagonal");
// the texts, the cells, the row of values with its two sentinels, the spans and two words of results: within 64 KiB
static_assert((2 * KL_ALIGN_LEN_MAX + ALIGN_LDS_CELL_WORDS + ALIGN_THREADS_MAX + 2 + 4 * KL_ALIGN_DIST_MAX + 2) * 4 <= 64 * 1024,
              "LDS of the largest launch");

// words of two-bit cells for a text a of n symbols: rows 0 .. n in groups of 16, one word per group and diagonal
__host__ __device__ inline int cell_words(int n, int L) { return (n / 16 + 1) * L; }

// what a launch sets aside: the cells of the longest text in LDS if they fit, else the LDS share and a slice of workspace
struct align_shape {
  int threads, L;
  int lds_cell_words;      // two-bit cells kept in LDS (words)
  int slice_words;         // ... and in the workspace, per workgroup (0: the longest text fits LDS)
  size_t lds_bytes;
};

inline align_shape shape_of(int max_len, int max_dist) {
  align_shape s;
  s.L = 2 * max_dist + 1;
  s.threads = (s.L + KL_WAVE - 1) / KL_WAVE * KL_WAVE;
  const int need = cell_words(max_len, s.L);
  s.lds_cell_words = need <= ALIGN_LDS_CELL_WORDS ? need : ALIGN_LDS_CELL_WORDS;
  s.slice_words = need <= ALIGN_LDS_CELL_WORDS ? 0 : (need + 1) / 2 * 2;      // (whole 8-byte words)
  s.lds_bytes = (size_t)(2 * max_len + s.lds_cell_words + s.L + 2 + 4 * max_dist + 2) * 4;
  return s;
}

inline unsigned grid_of(size_t P) { return P < (size_t)ALIGN_GRID_MAX ? (unsigned)P : (unsigned)ALIGN_GRID_MAX; }

// Lane k on anti-diagonal t.  a, b: the texts (n, m symbols); row: the lanes' last values, lane k at row[k + 1], ALIGN_INF in
// row[0] and row[L + 1]; own: this lane's last value, D[i-1][j-1] of its next cell; acc: the two-bit rules of its rows since
// the last stored word; cells: where the words go (the caller chose LDS or workspace).  Returns true with `d` set at (n, m).
__host__ __device__ __forceinline__ bool align_cell(int t, int k, int K, int L, const int* a, int n, const int* b, int m, int* row,
                                           int& own, unsigned& acc, unsigned* cells, int& d) {
  const int twice = t - k + K;      // 2 i
  if (twice < 0 || (twice & 1)) return false;
  const int i = twice >> 1, j = t - i;
  if (i > n || j < 0 || j > m) return false;
  int v, op;
  if (i == 0) {
    v = j;
    op = OP_INSERT;
  } else if (j == 0) {
    v = i;
    op = OP_DELETE;
  } else {
    const bool same = a[i - 1] == b[j - 1];
    const int diag = own, up = row[k + 2], left = row[k];
    const int step = up < left ? up : left;
    v = diag + (same ? 0 : 1);
    v = step + 1 < v ? step + 1 : v;
    op = same && diag == v ? OP_MATCH : diag + 1 == v ? OP_SUBST : up + 1 == v ? OP_DELETE : OP_INSERT;
  }
  own = v;
  row[k + 1] = v;
  acc |= (unsigned)op << (2 * (i & 15));
  if ((i & 15) == 15 || i == n || j == m) {      // the word is full, or this is the diagonal's last cell
    cells[(i >> 4) * L + k] = acc;
    acc = 0u;
  }
  if (i == n && j == m) {
    d = v;
    return true;
  }
  return false;
}

// The walk back from (n, m) over the stored rules, on one lane: the differences -- maximal runs of non-matches, two of them with
// at most `join` matches between them made one -- as (a_start, a_end, b_start, b_end), in DESCENDING order in out[4 * s ..].
// Returns their number, at most D[n][m].
__host__ __device__ __forceinline__ int align_walk(int n, int m, int K, int L, int join, const unsigned* cells, int* out) {
  int i = n, j = m, count = 0;
  int a0 = 0, a1 = 0, b0 = 0, b1 = 0;      // the open span
  bool open = false;
  int matches = 0;                         // ... and the matches walked since its first operation
  int held = -1;                           // (a diagonal's word serves up to 16 steps of a run of matches)
  unsigned word = 0u;
  while (i > 0 || j > 0) {
    const int at = (i >> 4) * L + (j - i + K);
    if (at != held) {
      word = cells[at];
      held = at;
    }
    const int op = (int)((word >> (2 * (i & 15))) & 3u);
    if (op == OP_MATCH) {
      --i;
      --j;
      ++matches;
      continue;
    }
    if (!open || matches > join) {
      if (open) {
        out[4 * count + 0] = a0, out[4 * count + 1] = a1, out[4 * count + 2] = b0, out[4 * count + 3] = b1;
        ++count;
      }
      a1 = i;
      b1 = j;
      open = true;
    }
    i -= op != OP_INSERT ? 1 : 0;
    j -= op != OP_DELETE ? 1 : 0;
    a0 = i;
    b0 = j;
    matches = 0;
  }
  if (open) {
    out[4 * count + 0] = a0, out[4 * count + 1] = a1, out[4 * count + 2] = b0, out[4 * count + 3] = b1;
    ++count;
  }
  return count;
}

__global__ void __launch_bounds__(ALIGN_THREADS_MAX) align_pairs_kernel(
    const int* __restrict__ a_pool, long long n_a, const long long* __restrict__ a_off, const int* __restrict__ b_pool,
    long long n_b, const long long* __restrict__ b_off, int P, int max_len, int K, int join, int lds_cell_words, int slice_words,
    int* __restrict__ dist, int* __restrict__ n_spans, int* __restrict__ spans, unsigned* ws) {
  extern __shared__ int lds[];
  const int L = 2 * K + 1;
  int* s_a = lds;                                                        // [max_len]
  int* s_b = s_a + max_len;                                              // [max_len]
  unsigned* s_cells = reinterpret_cast<unsigned*>(s_b + max_len);        // [lds_cell_words]
  int* s_row = reinterpret_cast<int*>(s_cells + lds_cell_words);         // [L + 2]
  int* s_spans = s_row + L + 2;                                          // [4 * K]
  int* s_result = s_spans + 4 * K;                                       // d, the number of spans
  unsigned* g_cells = ws + (size_t)blockIdx.x * slice_words;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_row[0] = ALIGN_INF;
    s_row[L + 1] = ALIGN_INF;
  }
  for (int p = blockIdx.x; p < P; p += gridDim.x) {
    const long long a_lo = a_off[p], a_hi = a_off[p + 1], b_lo = b_off[p], b_hi = b_off[p + 1];
    const bool outside = a_lo < 0 || a_hi < a_lo || a_hi > n_a || b_lo < 0 || b_hi < b_lo || b_hi > n_b;
    int status, count = 0;      // (uniform: a workgroup is one pair)
    if (outside || a_hi - a_lo > max_len || b_hi - b_lo > max_len) {
      status = -2;
    } else if (a_hi - a_lo - (b_hi - b_lo) > K || b_hi - b_lo - (a_hi - a_lo) > K) {
      status = -1;
    } else {
      const int n = (int)(a_hi - a_lo), m = (int)(b_hi - b_lo);
      for (int x = tid; x < n; x += blockDim.x) s_a[x] = a_pool[a_lo + x];
      for (int x = tid; x < m; x += blockDim.x) s_b[x] = b_pool[b_lo + x];
      const bool in_lds = cell_words(n, L) <= lds_cell_words;
      __syncthreads();
      int own = 0, d = 0;
      unsigned acc = 0u;
      for (int t = 0; t <= n + m; ++t) {
        if (tid < L) {
          const bool last = in_lds ? align_cell(t, tid, K, L, s_a, n, s_b, m, s_row, own, acc, s_cells, d)
                                   : align_cell(t, tid, K, L, s_a, n, s_b, m, s_row, own, acc, g_cells, d);
          if (last) s_result[0] = d;
        }
        __syncthreads();
      }
      status = s_result[0];
      if (status > K) {
        status = -1;
      } else {
        if (tid == 0) s_result[1] = in_lds ? align_walk(n, m, K, L, join, s_cells, s_spans) : align_walk(n, m, K, L, join, g_cells, s_spans);
        __syncthreads();
        count = s_result[1];
      }
    }
    if (tid == 0) {
      dist[p] = status;
      n_spans[p] = count;
    }
    int* __restrict__ mine = spans + (size_t)p * K * 4;
    for (int x = tid; x < 4 * K; x += blockDim.x)
      mine[x] = x < 4 * count ? s_spans[4 * (count - 1 - (x >> 2)) + (x & 3)] : -1;      // ascending; -1 behind
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

inline bool bad_shape(size_t P, int max_len, int max_dist) {
  return P < 1 || P > MAX_PAIRS || max_len < 0 || max_len > KL_ALIGN_LEN_MAX || max_dist < 1 || max_dist > KL_ALIGN_DIST_MAX;
}

}  // namespace

extern "C" size_t kl_align_pairs_workspace_bytes(size_t P, int max_len, int max_dist) {
  if (bad_shape(P, max_len, max_dist)) return 0;
  const size_t bytes = (size_t)grid_of(P) * shape_of(max_len, max_dist).slice_words * 4;
  return bytes < 8 ? 8 : bytes;
}

extern "C" int kl_align_pairs(const int32_t* a_pool, size_t n_a, const int64_t* a_off, const int32_t* b_pool, size_t n_b,
                              const int64_t* b_off, size_t P, int max_len, int max_dist, int join, int32_t* dist, int32_t* n_spans,
                              int32_t* spans, void* ws, size_t ws_bytes, void* stream) {
  if (!a_off || !b_off || !dist || !n_spans || !spans || !ws) return KL_ERR_ARG;
  if ((n_a > 0 && !a_pool) || (n_b > 0 && !b_pool)) return KL_ERR_ARG;
  if (bad_shape(P, max_len, max_dist) || join < 0 || n_a > (size_t)1 << 40 || n_b > (size_t)1 << 40) return KL_ERR_ARG;
  const void* words[] = {a_pool, b_pool, dist, n_spans, spans};
  for (const void* p : words)
    if (misaligned(p, 3)) return KL_ERR_ARG;
  if (misaligned(a_off, 7) || misaligned(b_off, 7)) return KL_ERR_ARG;
  if (misaligned(ws, 7) || ws_bytes < kl_align_pairs_workspace_bytes(P, max_len, max_dist)) return KL_ERR_WORKSPACE;
  const align_shape s = shape_of(max_len, max_dist);
  hipLaunchKernelGGL(align_pairs_kernel, dim3(grid_of(P)), dim3(s.threads), s.lds_bytes, static_cast<hipStream_t>(stream), a_pool,
                     (long long)n_a, reinterpret_cast<const long long*>(a_off), b_pool, (long long)n_b,
                     reinterpret_cast<const long long*>(b_off), (int)P, max_len, max_dist, join, s.lds_cell_words, s.slice_words, dist,
                     n_spans, spans, static_cast<unsigned*>(ws));
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
