// Beam expand (kl_beam_expand): one expansion and pruning step of `generate`'s beam search (rating.py:689-707) on the device.
//
// After kl_step_batch the probabilities of all hypotheses lie in HBM as probs [rows][V].  The reference then takes, per
// hypothesis, the 10 most likely characters with p >= 0.004, insorts every continuation into one list ordered by running
// cost and keeps the first 256.  Restated as a total order (so that it can run in parallel):
//   * candidates of a live row: its `fan` largest probabilities, equal values by smaller id first (OUR definition: the
//     reference leaves such ties to an unstable sort); of those the ones with p >= floor whose id is valid -- an invalid id
//     among the `fan` largest still occupies its place;
//   * cost = -logf(p), cum = cum_in[row] + cost (one f32 addition, as the host path's float32 + float32);
//   * insertion sequence = row * fan + k, k counting a row's candidates from the least to the most probable;
//   * survivors = the first `rows` candidates in the order (cum ascending, insertion sequence DESCENDING): insort_left puts
//     a later equal key in front, and truncating the running list after every insertion yields the head of the total order.
// Two launches:
//   beam_topk_kernel    one wave per row, four rows per workgroup (the layout of step_finish_kernel): up to `fan` rounds of a
//                       wave-wide arg-max over the row, each lane striding over V; a round skips what precedes the last pick
//                       in (p descending, id ascending) order and the rounds end at the first pick below `floor` (all later
//                       ones are smaller still).  Writes one 64-bit key per (row, k): high word the bits of cum (a
//                       non-negative f32 -- p <= 1 --, so the raw bits order correctly; +inf = absent), low word the
//                       complemented insertion sequence; and the candidate's id.
//   beam_select_kernel  ONE workgroup: bitonic sort of the rows * fan keys in LDS (padded to a power of two, 4096 keys =
//                       32 KiB), then the first `rows` entries become the next step's inputs and the log's row.
// Plain loads and vector stores only; no workgroup waits for another, nothing is written at system scope: the log is read
// after an ordinary stream synchronisation.
#include "kl_common.h"
#include "kl_kernels.h"

namespace {

typedef unsigned long long u64;
constexpr u64 BEAM_ABSENT = 0x7f800000ffffffffull;      // cum = +inf, sequence 0 complemented
constexpr unsigned BEAM_INF = 0x7f800000u;

__global__ __launch_bounds__(256) void beam_topk_kernel(const KlBeamExpand a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;      // (whole waves leave; there is no barrier in this kernel)
  const int fan = a.fan, V = a.V;
  const float base = a.cum_in[row];
  u64 my_key = BEAM_ABSENT;      // lane j keeps the pick of round j
  int my_id = 0;
  if (base < INFINITY) {      // (+inf: dead row; NaN compares false and is dead too)
    const float* p = a.probs + (long)row * V;
    float last_p = INFINITY;
    int last_id = -1;
    for (int j = 0; j < fan; ++j) {
      float bp = -1.f;
      int bi = 0x7fffffff;
      for (int v = lane; v < V; v += 64) {
        const float x = p[v];
        const bool after = x < last_p || (x == last_p && v > last_id);
        if (after && x > bp) {      // (v ascends within a lane: `>` keeps the smaller id among equal values)
          bp = x;
          bi = v;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float op = __shfl_xor(bp, off);
        const int oi = __shfl_xor(bi, off);
        if (op > bp || (op == bp && oi < bi)) {
          bp = op;
          bi = oi;
        }
      }
      // (every lane now holds the same pick)
      if (bi == 0x7fffffff || !(bp >= a.floor)) break;      // nothing left, or below the floor -- as is every later pick
      const bool ok = a.valid ? a.valid[bi] != 0 : bi != 0;
      if (ok && lane == j) {
        const float cost = -logf(bp);
        const float cum = base + cost;
        const unsigned seq = (unsigned)(row * fan + (fan - 1 - j));
        my_key = ((u64)__float_as_uint(cum) << 32) | (u64)(~seq);
        my_id = bi;
      }
      last_p = bp;
      last_id = bi;
    }
  }
  if (lane < fan) {
    const int at = row * fan + (fan - 1 - lane);
    a.keys[at] = my_key;
    a.cand[at] = my_id;
  }
}

__global__ __launch_bounds__(1024) void beam_select_kernel(const KlBeamExpand a, const int N) {
  __shared__ u64 key[4096];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n = a.rows * a.fan;
  for (int i = tid; i < N; i += nt) key[i] = i < n ? a.keys[i] : ~0ull;
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (N >> 1); t += nt) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // the pair's lower index: t with a zero bit put in at j
        const u64 x = key[i], y = key[i + j];
        const bool up = (i & k) == 0;
        if ((x > y) == up) {
          key[i] = y;
          key[i + j] = x;
        }
      }
      __syncthreads();
    }
  }
  const unsigned fan = (unsigned)a.fan;
  for (int i = tid; i < a.rows; i += nt) {
    const u64 kv = key[i];
    const unsigned hi = (unsigned)(kv >> 32);
    const bool here = hi < BEAM_INF;
    int id = 0, slot = a.zero_slot, parent = -1;
    float cum = INFINITY;
    if (here) {
      const unsigned seq = ~(unsigned)kv;      // < rows * fan: only beam_topk_kernel writes keys with a finite high word
      parent = (int)(seq / fan);
      id = a.cand[seq];
      slot = a.slot_new[parent];
      cum = __uint_as_float(hi);
    }
    a.idx_next[i] = id;
    a.slot_in_next[i] = slot;
    a.cum_next[i] = cum;
    a.parent_log[i] = parent;
    a.idx_log[i] = id;
    a.cum_log[i] = cum;
    // the live count: the present keys form a prefix of the sorted order
    const bool next_here = i + 1 < a.rows && (unsigned)(key[i + 1] >> 32) < BEAM_INF;
    if (here && !next_here) *a.n_live = i + 1;
    if (i == 0 && !here) *a.n_live = 0;
  }
}

}  // namespace

size_t kl_beam_ws_bytes(int rows, int fan) {
  const size_t n = (size_t)rows * fan;
  return (n * sizeof(u64) + 255) / 256 * 256 + (n * sizeof(int) + 255) / 256 * 256;
}

int kl_launch_beam_expand(KlBeamExpand a, void* ws, hipStream_t stream) {
  if (a.rows < 1 || a.rows > KL_BEAM_MAX_ROWS || a.fan < 1 || a.fan > KL_BEAM_MAX_FAN || a.V < 1) return KL_ERR_ARG;
  if (!a.probs || !a.cum_in || !a.slot_new || !a.idx_next || !a.slot_in_next || !a.cum_next || !a.parent_log || !a.idx_log ||
      !a.cum_log || !a.n_live || !ws)
    return KL_ERR_ARG;
  const int n = a.rows * a.fan;
  a.keys = reinterpret_cast<u64*>(ws);
  a.cand = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(ws) + ((size_t)n * sizeof(u64) + 255) / 256 * 256);
  int N = 2;
  while (N < n) N <<= 1;      // <= 4096 = KL_BEAM_MAX_ROWS * KL_BEAM_MAX_FAN: what beam_select_kernel's LDS array holds
  hipLaunchKernelGGL(beam_topk_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, stream, a);
  const int threads = N / 2 < 64 ? 64 : (N / 2 > 1024 ? 1024 : N / 2);
  hipLaunchKernelGGL(beam_select_kernel, dim3(1), dim3(threads), 0, stream, a, N);
  return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH;
}
