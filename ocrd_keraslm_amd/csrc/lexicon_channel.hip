// Lexicon look-up under learned confusions (kl_lexicon_channel): which entries of a lexicon are cheap to reach from each query
// word when a plain insertion, deletion or substitution costs `unit` and every rule "src in the query stands for tgt in the
// entry" (up to four ids a side, the records kl_confusion_counts writes) its own cost?
//
// W[0][0] = 0, W[i][j] = min(W[i-1][j-1] + (q[i-1] == e[j-1] ? 0 : unit), W[i-1][j] + unit, W[i][j-1] + unit,
// W[i-s][j-t] + cost_r for every rule r with q[i-s:i] == src_r and e[j-t:j] == tgt_r); the distance is W[m][n].  Myers' bit
// vectors carry neither weights nor rules, so this is the plain DP over every (query, entry) pair of the reachable classes.
//
// The frame all four look-ups share (kl_lexicon_frame.h: the arguments and the class table checked on the host, the query's
// bounds): a preparing launch of one workgroup puts the class table into the workspace, then one workgroup per query, every
// lane walks whole entries of a length class from the column-major layout, the lanes' key lists and the fold are
// kl_lexicon_topk.h's.  No Peq: ids are compared, and the query's ids outside [0, V) are -1 in LDS.  The preparing launch
// also checks the rules (they lie on the device: the entry point cannot), packs the kept ones into 5 words each -- ids in 16
// bits, V <= 4096 --, and reduces them to two prices.
//
// Which classes.  An entry of m + d ids costs at least |d| times the cheapest price per id of lengthening (d > 0: unit, or
// cost / (t - s) of a rule with t > s) or of shortening (d < 0, s > t).  |t - s| is 1 .. 4, so 12 * cost / |t - s| is an
// integer: the prices are kept in twelfths, and d is within the window iff |d| * price12 <= 12 * max_cost; a price of 0 opens
// every class on its side.  A bound, not the definition: the DP decides.
//
// The query side once per workgroup.  Every thread takes up to four rules and marks the rows i at which their source stands
// (q[i-s:i] == src) in a 64-bit word; the rows' counts (LDS atomic adds: a sum) give each row a slice of the active list, into
// which the rules are then put in the order of arrival (LDS atomic adds again: the list is only ever folded by a minimum, its
// order is never observed).  A list entry is the rule's target, lengths and cost: 3 words.  Per cell a lane then compares the
// targets of the rules active at row i with the entry's last four ids, which it holds packed in two registers.  When more than
// CH_ACTIVE (rule, row) pairs match -- one source with 1024 targets on a query of 64 equal ids has 65 536 -- no list is built and
// every cell loops over all rules and checks the source too: slower, the same result.
//
// The cells.  A rule reaches back four columns and four rows, so a lane needs a ring of five columns of m + 1 cells.  In
// registers that is dynamic indexing, hence scratch; the ring lives in LDS.  A value above max_cost is as good as max_cost + 1
// <= 4096, so a cell is 16 bits, saturated; laid out [column][row][lane], a wave's 64 cells of one (column, row) are 128
// consecutive bytes -- 32 banks, two lanes per bank word, no conflict.  That is 10 (m + 1) bytes per lane: 160 at m = 15, 330
// at m = 32, 650 at m = 64.  The ring is CH_RING = 5 * 33 * 128 cells (42 240 bytes) for every query, and the lanes that walk
// are what fits it, in whole waves: 256 at m <= 15, 192 at m <= 21, 128 at m <= 32, 64 beyond -- one kernel, no
// instantiation per length bucket; the waves without a ring have empty lists and only take part in the fold.  With the active
// list (6 KiB) and the small arrays a workgroup holds 49.5 KiB of LDS: three workgroups per CU within 160 KiB, 12 waves, and
// the registers (well below 128) do not bind before that.
//
// No atomics on global memory, no workgroup waits for another, the output depends on the inputs only.  No address is formed
// from an id, a length or a rule field that has not been range-checked: ids are only ever compared.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_lexicon_frame.h"
#include "kl_lexicon_topk.h"

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_WAVES = CH_THREADS / KL_WAVE;
constexpr int CH_LEN_MAX = LEX_LEN_MAX;
constexpr int CH_RING_COLS = 5;                  // a rule reaches back four columns
constexpr int CH_RING = CH_RING_COLS * 33 * 128;      // cells: 128 lanes at m = 32, 64 at m = 64
constexpr int CH_ACTIVE = 512;                   // (rule, row) pairs of the active list
constexpr int CH_RULE_WORDS = 5;                 // a packed rule: src (2 words), tgt (2 words), meta
constexpr int CH_RULES_PER_THREAD = KL_CHANNEL_RULES_MAX / CH_THREADS;
static_assert(CH_RING >= CH_RING_COLS * (CH_LEN_MAX + 1) * KL_WAVE, "one wave walks a query of 64 ids");
static_assert(KL_CHANNEL_RULES_MAX % CH_THREADS == 0, "every thread settles the same number of rules");
static_assert(KL_CHANNEL_COST_MAX < (1 << 12), "a cost is 12 bits of a rule's meta word");
static_assert(KL_LEXICON_V_MAX <= 0xFFF0, "an id is 16 bits of a packed rule, 0xFFFE and 0xFFFF are no ids");

// the workspace: the class table, the two prices, the packed rules
constexpr size_t WS_PRICES = 2 * LEX_CLASSES * sizeof(long long);
constexpr size_t WS_RULES = WS_PRICES + 16;

__device__ __forceinline__ unsigned int meta_s(unsigned int meta) { return (meta >> 12) & 7u; }
__device__ __forceinline__ unsigned int meta_t(unsigned int meta) { return (meta >> 15) & 7u; }
__device__ __forceinline__ int meta_cost(unsigned int meta) { return (int)(meta & 0xFFFu); }

// One workgroup: the class table (every index into the arguments a constant, as in lexicon.hip), every rule checked and packed
// -- an ignored rule has meta 0, that is src_len 0 --, and the cheapest price per id of lengthening and of shortening in
// twelfths of a cost unit.
__global__ void __launch_bounds__(CH_THREADS) channel_prepare_kernel(const lex_classes cls, const int* __restrict__ rules,
                                                                     const int* __restrict__ rule_cost, int R, int V, int unit,
                                                                     long long* __restrict__ table, int* __restrict__ prices,
                                                                     unsigned int* __restrict__ packed) {
  __shared__ int s_up[CH_WAVES], s_down[CH_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < LEX_CLASSES; ++i)
    if (tid == i) {
      table[i] = cls.first[i];
      table[LEX_CLASSES + i] = cls.base[i];
    }
  int up = 12 * unit, down = 12 * unit;
  for (int r = tid; r < R; r += CH_THREADS) {
    const int* __restrict__ rec = rules + (size_t)r * 10;
    const int s = rec[0], t = rec[1], cost = rule_cost[r];
    bool keep = s >= 1 && s <= 4 && t >= 0 && t <= 4 && cost >= 0 && cost <= KL_CHANNEL_COST_MAX;
    unsigned int src[4] = {0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu}, tgt[4] = {0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (keep && k < s) {
        const int id = rec[2 + k];
        keep = id >= 0 && id < V;
        src[k] = (unsigned int)id & 0xFFFFu;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (keep && k < t) {
        const int id = rec[6 + k];
        keep = id >= 0 && id < V;
        tgt[k] = (unsigned int)id & 0xFFFFu;
      }
    }
    unsigned int* __restrict__ out = packed + (size_t)r * CH_RULE_WORDS;
    // the source in the order of the query, the target BACKWARDS: tgt[t-1] is held against the entry's last id
    unsigned int back[4] = {0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (keep && j == t - 1 - k) back[k] = tgt[j];
    out[0] = keep ? src[0] | (src[1] << 16) : 0u;
    out[1] = keep ? src[2] | (src[3] << 16) : 0u;
    out[2] = keep ? back[0] | (back[1] << 16) : 0u;
    out[3] = keep ? back[2] | (back[3] << 16) : 0u;
    out[4] = keep ? (unsigned int)cost | ((unsigned int)s << 12) | ((unsigned int)t << 15) : 0u;
    if (keep && t > s) {
      const int p = 12 * cost / (t - s);
      up = p < up ? p : up;
    }
    if (keep && s > t) {
      const int p = 12 * cost / (s - t);
      down = p < down ? p : down;
    }
  }
#pragma unroll
  for (int off = KL_WAVE / 2; off > 0; off >>= 1) {
    const int u = __shfl_xor(up, off, KL_WAVE), d = __shfl_xor(down, off, KL_WAVE);
    up = u < up ? u : up;
    down = d < down ? d : down;
  }
  if (lane == 0) {
    s_up[wave] = up;
    s_down[wave] = down;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < CH_WAVES; ++w) {
      up = s_up[w] < up ? s_up[w] : up;
      down = s_down[w] < down ? s_down[w] : down;
    }
    prices[0] = up;
    prices[1] = down;
  }
}

// does the source of a packed rule (s ids) stand in front of row i of the query?  (i >= s; ids of the query outside [0, V) are
// -1 in s_query and equal no id of a rule)
__device__ __forceinline__ bool source_stands(const int* s_query, int i, unsigned int s, unsigned int src_lo, unsigned int src_hi) {
  const int at = i - (int)s;
  bool same = s_query[at] == (int)(src_lo & 0xFFFFu);
  if (s > 1) same = same && s_query[at + 1] == (int)(src_lo >> 16);
  if (s > 2) same = same && s_query[at + 2] == (int)(src_hi & 0xFFFFu);
  if (s > 3) same = same && s_query[at + 3] == (int)(src_hi >> 16);
  return same;
}

// a rule whose source stands at row i, held against the entry's last ids (e_lo: the last and the one before, e_hi: the two before
// them; 0xFFFE: no id) in column j >= t: the cell (i - s, j - t) of the ring plus its cost, or `v`
__device__ __forceinline__ int through_rule(const unsigned short* ring, int rows, int lanes, int i, int j, int slot_j,
                                            unsigned int e_lo, unsigned int e_hi, unsigned int tgt_lo, unsigned int tgt_hi,
                                            unsigned int meta, int v) {
  const int s = (int)meta_s(meta), t = (int)meta_t(meta);
  if (j < t) return v;      // (uniform)
  const unsigned int m_lo = t >= 2 ? 0xFFFFFFFFu : t == 1 ? 0xFFFFu : 0u;
  const unsigned int m_hi = t >= 4 ? 0xFFFFFFFFu : t == 3 ? 0xFFFFu : 0u;
  const bool same = (((e_lo ^ tgt_lo) & m_lo) | ((e_hi ^ tgt_hi) & m_hi)) == 0u;
  int slot = slot_j - t;
  slot = slot < 0 ? slot + CH_RING_COLS : slot;
  const int from = (int)ring[(slot * rows + (i - s)) * lanes] + meta_cost(meta);      // (0 <= i - s, 0 <= j - t: inside the ring)
  return same && from < v ? from : v;
}

__global__ void __launch_bounds__(CH_THREADS) lexicon_channel_kernel(
    const int* __restrict__ chars, const int* __restrict__ order, const long long* __restrict__ table,
    const int* __restrict__ prices, const unsigned int* __restrict__ packed, int R, int V, const int* __restrict__ q_pool,
    long long n_q, const long long* __restrict__ q_off, int unit, int max_cost, int K, int* __restrict__ exact,
    int* __restrict__ found, int* __restrict__ cand, int* __restrict__ cost_out) {
  __shared__ unsigned short s_ring[CH_RING];
  __shared__ unsigned int s_list[CH_ACTIVE * 3];
  __shared__ int s_query[CH_LEN_MAX];
  __shared__ int s_count[CH_LEN_MAX + 2], s_start[CH_LEN_MAX + 2];
  __shared__ kl_lex_fold<CH_WAVES> s_fold;
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
      cost_out[q * K + tid] = -1;
    }
    return;
  }
  if (tid < m) {
    const int id = q_pool[qa + tid];
    s_query[tid] = id >= 0 && id < V ? id : -1;      // (equals nothing)
  }
  if (tid < CH_LEN_MAX + 2) s_count[tid] = 0;
  __syncthreads();

  // where each rule's source stands in the query: bit i - 1 of a thread's word for row i
  unsigned long long stands[CH_RULES_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CH_RULES_PER_THREAD; ++k) {
    stands[k] = 0ull;
    const int r = tid + k * CH_THREADS;
    if (r < R) {
      const unsigned int* __restrict__ rule = packed + (size_t)r * CH_RULE_WORDS;
      const unsigned int meta = rule[4], s = meta_s(meta);
      if (s != 0u) {
        const unsigned int src_lo = rule[0], src_hi = rule[1];
        for (int i = (int)s; i <= m; ++i)
          if (source_stands(s_query, i, s, src_lo, src_hi)) {
            stands[k] |= 1ull << (i - 1);
            atomicAdd(&s_count[i], 1);      // (a sum: the order of arrival is not seen)
          }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int i = 0; i <= m; ++i) {
      s_start[i] = total;
      total += s_count[i];
    }
    s_start[m + 1] = total;
  }
  __syncthreads();
  const bool listed = s_start[m + 1] <= CH_ACTIVE;      // (uniform)
  if (listed) {
    if (tid <= m) s_count[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CH_RULES_PER_THREAD; ++k) {
      if (stands[k] != 0ull) {
        const unsigned int* __restrict__ rule = packed + (size_t)(tid + k * CH_THREADS) * CH_RULE_WORDS;
        const unsigned int tgt_lo = rule[2], tgt_hi = rule[3], meta = rule[4];
        for (int i = 1; i <= m; ++i)
          if ((stands[k] >> (i - 1)) & 1ull) {
            // (a place within the row's slice; the slice is folded by a minimum, so its order is never observed)
            const int at = s_start[i] + atomicAdd(&s_count[i], 1);
            s_list[3 * at] = tgt_lo;
            s_list[3 * at + 1] = tgt_hi;
            s_list[3 * at + 2] = meta;
          }
      }
    }
    __syncthreads();
  }

  unsigned long long best[KL_LEXICON_K_MAX];
#pragma unroll
  for (int i = 0; i < KL_LEXICON_K_MAX; ++i) best[i] = KL_LEX_NO_KEY;
  unsigned int least_exact = KL_LEX_NO_EXACT;
  int n_found = 0;

  // the lanes that walk: what the ring holds, in whole waves
  const int rows = m + 1;
  int lanes = CH_RING / (CH_RING_COLS * rows);
  lanes = lanes >= CH_THREADS ? CH_THREADS : lanes & ~(KL_WAVE - 1);
  // the classes a word of m ids can reach within max_cost
  const int up = prices[0], down = prices[1];
  int d_up = up == 0 ? CH_LEN_MAX : 12 * max_cost / up, d_down = down == 0 ? CH_LEN_MAX : 12 * max_cost / down;
  const int hi = d_up > CH_LEN_MAX - m ? CH_LEN_MAX : m + d_up;
  const int lo = d_down > m - 1 ? 1 : m - d_down;
  const int beyond = max_cost + 1;      // every larger value is this one

  if (tid < lanes) {
    const unsigned short* ring_r = s_ring + tid;
    unsigned short* ring_w = s_ring + tid;
    for (int L = lo; L <= hi; ++L) {
      const long long at = table[L], n_L = table[L + 1] - at, base = table[LEX_CLASSES + L];
      for (long long e = tid; e < n_L; e += lanes) {
        const int* __restrict__ col = chars + base + e;      // id j of the entry: col[j * n_L]
        unsigned int e_lo = 0xFFFEFFFEu, e_hi = 0xFFFEFFFEu;
        bool identical = L == m;
        int next = col[0];
        int slot_j = 0, slot_left = CH_RING_COLS - 1;      // j % 5, (j - 1) % 5
        int last = beyond;
        for (int j = 0; j <= L; ++j) {
          int c = -2;      // (column 0 holds no id)
          if (j > 0) {
            c = next >= 0 && next < V ? next : -2;      // (equals nothing, not even a query's -1)
            next = j < L ? col[(long long)j * n_L] : 0;      // (the next id is under way)
            e_hi = (e_hi << 16) | (e_lo >> 16);
            e_lo = (e_lo << 16) | ((unsigned int)c & 0xFFFFu);
            identical = identical && s_query[j - 1] == c;
          }
          int above = beyond, diag = beyond;      // W[i-1][j], W[i-1][j-1]
          for (int i = 0; i <= m; ++i) {
            int v = (i | j) == 0 ? 0 : beyond;
            int left = beyond;
            if (j > 0) {
              left = ring_r[(slot_left * rows + i) * lanes];
              v = left + unit < v ? left + unit : v;
            }
            if (i > 0) {
              v = above + unit < v ? above + unit : v;
              if (j > 0) {
                const int through = diag + (s_query[i - 1] == c ? 0 : unit);
                v = through < v ? through : v;
              }
              if (listed) {
                for (int a = s_start[i]; a < s_start[i + 1]; ++a)
                  v = through_rule(ring_r, rows, lanes, i, j, slot_j, e_lo, e_hi, s_list[3 * a], s_list[3 * a + 1],
                                   s_list[3 * a + 2], v);
              } else {      // more pairs than the list holds: every rule, its source checked here
#pragma unroll 4
                for (int r = 0; r < R; ++r) {      // (four rules' words under way at a time)
                  const unsigned int* __restrict__ rule = packed + (size_t)r * CH_RULE_WORDS;
                  const unsigned int meta = rule[4], s = meta_s(meta);
                  if (s != 0u && (int)s <= i && source_stands(s_query, i, s, rule[0], rule[1]))
                    v = through_rule(ring_r, rows, lanes, i, j, slot_j, e_lo, e_hi, rule[2], rule[3], meta, v);
                }
              }
            }
            v = v < beyond ? v : beyond;
            ring_w[(slot_j * rows + i) * lanes] = (unsigned short)v;
            diag = left;
            above = v;
          }
          last = above;
          slot_left = slot_j;
          slot_j = slot_j + 1 == CH_RING_COLS ? 0 : slot_j + 1;
        }
        if (last <= max_cost) {
          const unsigned int index = (unsigned int)order[at + e];
          if (identical) {
            least_exact = index < least_exact ? index : least_exact;
          } else {
            ++n_found;
            kl_lex_keep(((unsigned long long)last << 32) | index, best);
          }
        }
      }
    }
  }
  kl_lex_fold_out<CH_WAVES>(s_fold, best, least_exact, n_found, K, q, exact, found, cand, cost_out);
}

}  // namespace

extern "C" size_t kl_lexicon_channel_workspace_bytes(size_t Q, int K, int R) {
  (void)Q;
  (void)K;
  const size_t rules = R > 0 ? (size_t)(R < KL_CHANNEL_RULES_MAX ? R : KL_CHANNEL_RULES_MAX) : 0;
  return WS_RULES + rules * CH_RULE_WORDS * sizeof(unsigned int);      // (the class table, the prices, the packed rules)
}

extern "C" int kl_lexicon_channel(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                                  const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, const int32_t* rules,
                                  const int32_t* rule_cost, int R, int unit, int max_cost, int K, int32_t* exact, int32_t* found,
                                  int32_t* cand, int32_t* cost, void* ws, size_t ws_bytes, void* stream) {
  if (!exact || !found || !cand || !cost) return KL_ERR_ARG;
  if (K < 1 || K > KL_LEXICON_K_MAX) return KL_ERR_ARG;
  if (R < 0 || R > KL_CHANNEL_RULES_MAX || unit < 1 || unit > KL_CHANNEL_COST_MAX || max_cost < 0 || max_cost > KL_CHANNEL_COST_MAX)
    return KL_ERR_ARG;
  if (R > 0 && (!rules || !rule_cost)) return KL_ERR_ARG;
  const void* words[] = {chars, order, q_pool, exact, found, cand, cost, rules, rule_cost};
  for (const void* p : words)
    if (lex_misaligned(p, 3)) return KL_ERR_ARG;
  lex_classes cls;
  if (lex_arguments_checked(chars, n_chars, order, class_first, V, q_pool, n_q, q_off, Q, ws, cls) != KL_OK) return KL_ERR_ARG;
  if (ws_bytes < kl_lexicon_channel_workspace_bytes(Q, K, R)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* bytes = reinterpret_cast<char*>(ws);
  long long* table = reinterpret_cast<long long*>(bytes);
  int* prices = reinterpret_cast<int*>(bytes + WS_PRICES);
  unsigned int* packed = reinterpret_cast<unsigned int*>(bytes + WS_RULES);
  hipLaunchKernelGGL(channel_prepare_kernel, dim3(1), dim3(CH_THREADS), 0, s, cls, rules, rule_cost, R, V, unit, table, prices,
                     packed);
  hipLaunchKernelGGL(lexicon_channel_kernel, dim3((unsigned)Q), dim3(CH_THREADS), 0, s, chars, order, table, prices, packed, R, V,
                     q_pool, (long long)n_q, reinterpret_cast<const long long*>(q_off), unit, max_cost, K, exact, found, cand, cost);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
