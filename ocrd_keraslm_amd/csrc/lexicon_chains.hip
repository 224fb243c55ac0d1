// Lexicon chains (kl_lexicon_chains): is a query word a concatenation of up to P exact lexicon entries -- a compound
// (`arbeit|s|amt`, a linking element between the parts) or a word that lost more than one space (`inthehouse`) -- and of which?
//
// That asks for every (start, length) substring of the query against the lexicon.  One walk over the length classes
// min_part .. m gives it: with the query's match masks Peq in LDS (kl_lexicon_myers.h), a lane that walks an entry of L ids
// keeps a word R whose bit a says "the entry could start at a" -- R = low(m - L + 1) at first, R &= Peq[c_j] >> j per entry
// character, an exact bit-parallel match in place of Myers' column -- and every bit left lowers s_piece[a][L] to the entry's
// original index with a 32-bit unsigned minimum in LDS.  One workgroup per query in the frame all four look-ups share
// (kl_lexicon_frame.h: the class table through the workspace, the query's bounds, Peq, the minimum in LDS).  Then a small DP
// in LDS over the piece table:
//
//   links     where each link stands in the query is one 64-bit mask per link (bit a: the link ends in front of a);
//   DP        thread b owns column b: E[1][b] = piece(0, b), E[p][b] = the least of max(E[p-1][b'], piece(a, b)) over a
//             ascending and, per a, b' = a (no link) in front of the links in index order that end at a; the first candidate
//             of least key is kept under a strict <, with its (a, link) packed beside it; one barrier per p;
//   walk back thread p - 1 follows the kept predecessors from E[p][m] and writes its row.
//
// A minimum does not depend on the order of arrival: two calls agree bit for bit.  The atomics are on LDS only; no workgroup
// waits for another.  No address is formed from an id that has not been range-checked.  No model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"
#include "kl_lexicon_myers.h"
#include <string.h>

namespace {

constexpr unsigned int NO_PIECE = ~0u;
constexpr int PARTS_MAX = KL_LEXICON_PARTS_MAX;
constexpr int LINKS_MAX = KL_LEXICON_LINKS_MAX;
constexpr int LINK_LEN_MAX = KL_LEXICON_LINK_LEN_MAX;
constexpr int MIN_PART_MAX = LEX_LEN_MAX / 2;      // (the bound of kl_lexicon_splits)

// the links, checked on the host, to the kernel by value
struct chain_links {
  int n;
  int len[LINKS_MAX];
  int ids[LINKS_MAX][LINK_LEN_MAX];
};

// a lane's walk over the entries e = tid, tid + LEX_THREADS, .. of the length classes min_part .. m: where an entry of L
// ids is identical to q[a : a + L], its original index lowers s_piece[a * LEX_LEN_MAX + L - 1]
template <typename W>
__device__ __forceinline__ void walk_pieces(const int* __restrict__ chars, const int* __restrict__ order,
                                            const long long* __restrict__ table, const unsigned long long* peq, int V, int m,
                                            int min_part, int tid, unsigned int* s_piece) {
  constexpr int BITS = 8 * (int)sizeof(W);
  for (int L = min_part; L <= m; ++L) {
    const long long at = table[L], n_L = table[L + 1] - at, base = table[LEX_CLASSES + L];
    const int places = m - L + 1;      // (1 .. BITS)
    const W all = places >= BITS ? ~(W)0 : ((W)1 << places) - 1;
    for (long long e = tid; e < n_L; e += LEX_THREADS) {
      const int* __restrict__ col = chars + base + e;      // character j of the entry: col[j * n_L]
      W R = all;
      int c = col[0];
      for (int j = 0; j < L; ++j) {
        const int next = j + 1 < L ? col[(long long)(j + 1) * n_L] : 0;      // (the next character is under way)
        R &= match_mask<W>(peq, c, V) >> j;
        if (R == 0) break;
        c = next;
      }
      if (R != 0) {
        const unsigned int index = (unsigned int)order[at + e];
        while (R != 0) {
          const int a = lowest(R);      // (a < places <= m - L + 1: inside the table)
          R &= R - 1;
          lex_lower(&s_piece[a * LEX_LEN_MAX + L - 1], index);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(LEX_THREADS) lexicon_chains_kernel(
    const int* __restrict__ chars, const int* __restrict__ order, const long long* __restrict__ table, int V,
    const int* __restrict__ q_pool, long long n_q, const long long* __restrict__ q_off, const chain_links links, int P,
    int min_part, int narrow, int* __restrict__ found, int* __restrict__ worst, int* __restrict__ entry, int* __restrict__ start,
    int* __restrict__ link) {
  __shared__ unsigned long long peq[KL_LEXICON_V_MAX];
  __shared__ unsigned int s_piece[LEX_LEN_MAX * LEX_LEN_MAX];      // [a][L - 1]: the piece q[a : a + L]
  __shared__ int s_query[LEX_LEN_MAX];
  __shared__ unsigned long long s_link_at[LINKS_MAX];               // bit a: link l is q[a - len : a], a - len >= 1
  __shared__ int s_link_len[LINKS_MAX];
  __shared__ unsigned int s_least[PARTS_MAX + 1][LEX_LEN_MAX + 1];  // E[p][b]
  __shared__ unsigned int s_from[PARTS_MAX + 1][LEX_LEN_MAX + 1];   // its predecessor: a | (link + 1) << 8
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  long long qa;
  int m;
  // a query that is none, or shorter than one piece, is no chain: nothing of the lexicon is read for it
  if (lex_query_bounds(q_off, q, n_q, min_part, qa, m)) {      // (uniform: the whole workgroup leaves)
    if (tid == 0) found[q] = 0;
    if (tid < P) worst[q * P + tid] = -1;
    if (tid < P * P) {
      entry[q * P * P + tid] = -1;
      start[q * P * P + tid] = -1;
      link[q * P * P + tid] = -1;
    }
    return;
  }
  for (int i = tid; i < LEX_LEN_MAX * LEX_LEN_MAX; i += LEX_THREADS) s_piece[i] = NO_PIECE;
  lex_query_peq<false>(peq, s_query, q_pool, qa, m, V, tid);
  if (tid < KL_WAVE) {
    // where the links stand, by the first wave: lane a asks whether link l ends in front of a.  (Every index into the
    // argument is a constant: one known at run time only would send it through scratch.)  The links' ids lie in [0, V), so
    // the same number is the same id.
#pragma unroll
    for (int l = 0; l < LINKS_MAX; ++l) {
      const int len = links.len[l];
      bool here = l < links.n && tid - len >= 1 && tid < m;
#pragma unroll
      for (int j = 0; j < LINK_LEN_MAX; ++j)
        if (j < len) here = here && s_query[tid - len + j > 0 ? tid - len + j : 0] == links.ids[l][j];
      const unsigned long long at = __ballot(here);
      if (tid == 0) {
        s_link_at[l] = at;
        s_link_len[l] = len;
      }
    }
  }
  __syncthreads();
  if (narrow && m <= 32)      // (uniform: a workgroup is one query)
    walk_pieces<unsigned int>(chars, order, table, peq, V, m, min_part, tid, s_piece);
  else
    walk_pieces<unsigned long long>(chars, order, table, peq, V, m, min_part, tid, s_piece);
  __syncthreads();

  // the DP: thread b owns column b
  const int b = tid;
  const bool mine = b >= 1 && b <= m;
  if (mine) {
    s_least[1][b] = b >= min_part ? s_piece[b - 1] : NO_PIECE;      // piece(0, b)
    s_from[1][b] = 0u;
  }
  __syncthreads();
  const int n_links = links.n;
  for (int p = 2; p <= P; ++p) {
    if (mine) {
      unsigned int best = NO_PIECE, from = 0u;
      for (int a = 1; a <= b - min_part; ++a) {
        const unsigned int piece = s_piece[a * LEX_LEN_MAX + b - a - 1];
        if (piece == NO_PIECE) continue;
        const unsigned int direct = s_least[p - 1][a];
        if (direct != NO_PIECE) {
          const unsigned int key = direct > piece ? direct : piece;
          if (key < best) {
            best = key;
            from = (unsigned int)a;
          }
        }
        for (int l = 0; l < n_links; ++l)
          if ((s_link_at[l] >> a) & 1ull) {
            const unsigned int before = s_least[p - 1][a - s_link_len[l]];      // (a - len >= 1: the mask says so)
            if (before != NO_PIECE) {
              const unsigned int key = before > piece ? before : piece;
              if (key < best) {
                best = key;
                from = (unsigned int)a | ((unsigned int)(l + 1) << 8);
              }
            }
          }
      }
      s_least[p][b] = best;
      s_from[p][b] = from;
    }
    __syncthreads();
  }

  // the walk back, by the first wave: thread p - 1 writes the row of p parts
  if (tid >= KL_WAVE) return;
  const int p = tid + 1;
  const bool have = p <= P && s_least[p <= P ? p : 1][m] != NO_PIECE;      // (no row behind P is read)
  const unsigned long long rows = __ballot(have);
  if (tid == 0) found[q] = (int)(unsigned int)rows;
  if (p > P) return;
  const long long row = (q * P + (p - 1)) * P;
  int used = 0;
  if (have) {
    int end = m;
    for (int k = p; k >= 1; --k) {
      const unsigned int from = s_from[k][end];
      const int a = (int)(from & 0xFFu), l = (int)(from >> 8) - 1;
      entry[row + k - 1] = (int)s_piece[a * LEX_LEN_MAX + end - a - 1];
      start[row + k - 1] = a;
      if (k >= 2) link[row + k - 2] = l;
      end = l >= 0 ? a - s_link_len[l] : a;
    }
    used = p;
  }
  worst[q * P + (p - 1)] = have ? (int)s_least[p][m] : -1;
  for (int k = used; k < P; ++k) {
    entry[row + k] = -1;
    start[row + k] = -1;
  }
  for (int k = used > 0 ? used - 1 : 0; k < P; ++k) link[row + k] = -1;
}

}  // namespace

extern "C" size_t kl_lexicon_chains_workspace_bytes(size_t Q, int P) {
  (void)Q;
  (void)P;
  return sizeof(lex_classes);      // (the class table, whatever Q and P are)
}

extern "C" int kl_lexicon_chains(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                                 const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, const int32_t* links,
                                 int n_links, int max_parts, int min_part, int32_t* found, int32_t* worst, int32_t* entry,
                                 int32_t* start, int32_t* link, void* ws, size_t ws_bytes, void* stream) {
  if (!found || !worst || !entry || !start || !link) return KL_ERR_ARG;
  if (max_parts < 2 || max_parts > PARTS_MAX || min_part < 1 || min_part > MIN_PART_MAX) return KL_ERR_ARG;
  if (n_links < 0 || n_links > LINKS_MAX || (n_links > 0 && !links)) return KL_ERR_ARG;
  const void* words[] = {chars, order, q_pool, found, worst, entry, start, link, links};
  for (const void* p : words)
    if (lex_misaligned(p, 3)) return KL_ERR_ARG;
  lex_classes cls;
  if (lex_arguments_checked(chars, n_chars, order, class_first, V, q_pool, n_q, q_off, Q, ws, cls) != KL_OK) return KL_ERR_ARG;
  chain_links by_value;
  memset(&by_value, 0, sizeof(by_value));
  by_value.n = n_links;
  for (int l = 0; l < n_links; ++l) {
    const int len = links[4 * l];
    if (len < 1 || len > LINK_LEN_MAX) return KL_ERR_ARG;
    by_value.len[l] = len;
    for (int j = 0; j < len; ++j) {
      const int id = links[4 * l + 1 + j];
      if (id < 0 || id >= V) return KL_ERR_ARG;
      by_value.ids[l][j] = id;
    }
  }
  if (ws_bytes < kl_lexicon_chains_workspace_bytes(Q, max_parts)) return KL_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  long long* table = reinterpret_cast<long long*>(ws);
  hipLaunchKernelGGL(lexicon_classes_kernel, dim3(1), dim3(2 * KL_WAVE), 0, s, cls, table);
  hipLaunchKernelGGL(lexicon_chains_kernel, dim3((unsigned)Q), dim3(LEX_THREADS), 0, s, chars, order, table, V, q_pool,
                     (long long)n_q, reinterpret_cast<const long long*>(q_off), by_value, max_parts, min_part, lex_narrow(),
                     found, worst, entry, start, link);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
