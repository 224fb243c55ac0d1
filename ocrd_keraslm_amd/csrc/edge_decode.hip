// Edge decode (kl_edge_costs, kl_edge_decode): the beam bookkeeping of MANY lattice edges in one launch.
//
// What `lattice_beam.decode_edge(table=...)`, `_finish` and the truncation to the beam width do for one edge (rating.py:796-851)
// is a serial algorithm over two ordered lists -- whether a track is re-queued depends on the head of the waiting list as left by
// the tracks re-queued before it, history clustering removes entries while it runs.  Its statement as a function over arrays
// is lib/lattice_batch.py::edge_decode_host; this file runs that statement for E edges at once, ONE WAVE PER EDGE:
//
//   * every decision that depends on order is taken on wave-uniform values (all 64 lanes read the same LDS word), in the
//     statement's order: the finishes of a batch cut from the worst end backwards, the re-queueing of a batch in key order, the
//     probes of bisect_left (the first waiting list is NOT sorted, so the position is whatever that probe sequence finds);
//   * what is bulk work runs across the lanes: cutting a batch off the list (ballot + prefix counts), the stable sort of a batch
//     (rank = number of entries that precede, ties by list order), the advance of a batch by one character, the shifts of a list
//     by one entry, the search for the first entry of a key, the distance sums of history clustering (kl_wave_dist2, the
//     function kl_state_dist2 uses);
//   * the waiting list (track, key), the finished list (reference, key), the tracks' costs / positions / lengths and a batch
//     live in LDS: 46 bytes per track of capacity + 768 (47872 bytes at the limit of 1024 tracks; the launch asks for the
//     capacity its largest edge needs, an edge of 60 tracks takes 3.5 KiB);
//   * no workgroup waits for another, no atomics, nothing is written at system scope.  All arithmetic on costs is IEEE f64 without
//     contraction, in the statement's order: results agree with it bit for bit, two launches agree bit for bit.
//
// An edge the kernel cannot hold (tracks above the launch's capacity, more than 64 entries already at the destination, an
// alternative of more than 65535 characters, a nonsensical descriptor, a NaN among its costs) sets out_status[e] = 1 and count 0;
// its other outputs are not defined (an edge over capacity writes nothing else).
#include "kl_common.h"
#include "kl_kernels.h"
#include "kl_state_dist.h"

namespace {

typedef unsigned long long u64;
typedef unsigned short u16;

struct EdgeLds {
  double* wkey; double* fkey; double* cum; double* bkey;
  int* fref;
  u16* wtrk; u16* pos; u16* len; u16* btrk; u16* sb;
};

// the edge's view of the launch's arrays
struct EdgeIn {
  int n_alt, in_off, alt_off, trk_off, pre_off;
};

__device__ __forceinline__ u64 lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// (one load per branch, no choice between pointers: that would put a table of pointers into scratch)
__device__ __forceinline__ int class_of(const KlEdgeDecode& a, const EdgeIn& e, int ref) {
  int v = 0;
  if (ref >= 0) v = a.alt_class[e.alt_off + ref % e.n_alt];
  if (ref < 0) v = a.pre_class[e.pre_off + (-1 - ref)];
  return v;
}

// (final_slot of a track with an empty alternative is its hypothesis' slot: the caller fills it in)
__device__ __forceinline__ int slot_of(const KlEdgeDecode& a, const EdgeIn& e, int ref) {
  int v = 0;
  if (ref >= 0) v = a.final_slot[e.trk_off + ref];
  if (ref < 0) v = a.pre_slot[e.pre_off + (-1 - ref)];
  return v;
}

// bisect.bisect_left(keys[:n], x): the statement's probes, all lanes together
__device__ __forceinline__ int bisect_left(const double* keys, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// make room at `at` in a list of n entries (key + payload): entries at .. n - 1 move up by one, top chunk first
template <typename T>
__device__ __forceinline__ void shift_up(double* keys, T* items, int at, int n, int lane) {
  for (int hi = n; hi > at; hi -= 64) {
    const int k = hi - 1 - lane;
    double kv = 0.0;
    T iv = 0;
    if (k >= at) { kv = keys[k]; iv = items[k]; }
    __syncthreads();
    if (k >= at) { keys[k + 1] = kv; items[k + 1] = iv; }
    __syncthreads();
  }
}

// drop entry `at` of a list of n entries: entries at + 1 .. n - 1 move down by one, bottom chunk first
template <typename T>
__device__ __forceinline__ void shift_down(double* keys, T* items, int at, int n, int lane) {
  for (int lo = at; lo < n - 1; lo += 64) {
    const int k = lo + lane;
    double kv = 0.0;
    T iv = 0;
    if (k < n - 1) { kv = keys[k + 1]; iv = items[k + 1]; }
    __syncthreads();
    if (k < n - 1) { keys[k] = kv; items[k] = iv; }
    __syncthreads();
  }
}

// whether the states of two pool slots are within the clustering distance in each of the first depth_k vectors
__device__ __forceinline__ bool close_states(const KlEdgeDecode& a, int sa, int sb, int lane) {
  for (int k = 0; k < a.depth_k; ++k) {
    const float d2 = kl_wave_dist2(a.pool + (long)sa * a.slot_stride + (long)k * a.W, a.pool + (long)sb * a.slot_stride + (long)k * a.W,
                                   a.W, lane);
    if (!((double)d2 < a.dist2)) return false;
  }
  return true;
}

// lattice_beam._finish: track i has consumed its alternative.  Returns the new length of the finished list.
__device__ __forceinline__ int finish_track(const KlEdgeDecode& a, const EdgeIn& e, const EdgeLds& s, int i, int nf, int lane) {
  __syncthreads();
  const double ci = s.cum[i];
  if (a.depth_k > 0) {
    const int cls = class_of(a, e, i);
    const int si = slot_of(a, e, i);
    int found = -1;
    for (int base = 0; base < nf && found < 0; base += 64) {
      const int k = base + lane;
      const int oref = k < nf ? s.fref[k] : 0;
      const bool same = k < nf && class_of(a, e, oref) == cls;
      const int oslot = same ? slot_of(a, e, oref) : 0;
      u64 mask = __ballot(same);
      while (mask && found < 0) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        if (close_states(a, si, __shfl(oslot, l), lane)) found = base + l;
      }
    }
    if (found >= 0) {
      const double oc = s.fkey[found];
      if (oc < ci) return nf;                      // redundant: the cheaper twin is already there
      int first = found;                           // list.remove by cost: the FIRST entry of equal cost goes
      for (int base = 0; base < found; base += 64) {
        const int k = base + lane;
        const u64 mask = __ballot(k < found && s.fkey[k] == oc);
        if (mask) { first = base + __builtin_ctzll(mask); break; }
      }
      shift_down(s.fkey, s.fref, first, nf, lane);
      --nf;
    }
  }
  const int at = bisect_left(s.fkey, nf, ci);
  shift_up(s.fkey, s.fref, at, nf, lane);
  s.fkey[at] = ci;
  s.fref[at] = i;
  __syncthreads();
  return nf + 1;
}

__global__ __launch_bounds__(64) void edge_decode_kernel(const KlEdgeDecode a) {
#pragma clang fp contract(off)
  extern __shared__ double lds_raw[];
  const int lane = threadIdx.x;
  const int edge = blockIdx.x;
  const int* d = a.desc + (long)edge * 8;
  const int n_in = d[0], n_alt = d[1], n_pre = d[2], max_batches = d[7];
  EdgeIn e;
  e.n_alt = n_alt; e.in_off = d[3]; e.alt_off = d[4]; e.trk_off = d[5]; e.pre_off = d[6];
  const long n_long = (long)n_in * (long)n_alt;
  const int C = a.cap_tracks, F = C + KL_EDGE_MAX_PRE;
  bool bad = n_in < 1 || n_alt < 1 || n_pre < 0 || n_pre > KL_EDGE_MAX_PRE || max_batches < 1 || max_batches > (1 << 20) || n_long > C ||
             e.in_off < 0 || e.alt_off < 0 || e.trk_off < 0 || e.pre_off < 0;
  if (!bad) {
    for (int base = 0; base < n_alt; base += 64) {      // (n_alt <= C here)
      const int k = base + lane;
      const int len = k < n_alt ? a.alt_len[e.alt_off + k] : 0;
      if (__ballot(len < 0 || len > 65535)) bad = true;
    }
  }
  if (bad) {
    if (lane == 0) { a.out_status[edge] = 1; a.out_count[edge] = 0; }
    return;
  }
  const int n = (int)n_long;
  EdgeLds s;
  s.wkey = lds_raw; s.fkey = s.wkey + C; s.cum = s.fkey + F; s.bkey = s.cum + C;
  s.fref = (int*)(s.bkey + C);
  s.wtrk = (u16*)(s.fref + F); s.pos = s.wtrk + C; s.len = s.pos + C; s.btrk = s.len + C; s.sb = s.btrk + C;

  // ---- the tracks (hypothesis-major, alternative-minor), the first waiting list (creation order, UNSORTED), the destination
  bool nan = false;      // (a NaN cost would leave the sort's ranks unassigned: such an edge goes back to the host, status 1)
  for (int i = lane; i < n; i += 64) {
    const int len = a.alt_len[e.alt_off + i % n_alt];
    const double c = a.cum_in[e.in_off + i / n_alt];
    nan = nan || c != c;
    s.cum[i] = c; s.pos[i] = 0; s.len[i] = (u16)len;
    s.wtrk[i] = (u16)i; s.wkey[i] = c + 0.5 * (double)len;
  }
  for (int j = lane; j < n_pre; j += 64) { s.fkey[j] = a.pre_cost[e.pre_off + j]; s.fref[j] = -1 - j; }
  if (__ballot(nan)) {
    if (lane == 0) { a.out_status[edge] = 1; a.out_count[edge] = 0; }
    return;
  }
  int nw = n, nf = n_pre;
  const long cap = (long)max_batches * (long)a.batch_size;
  __syncthreads();

  for (int number = 0; number < max_batches; ++number) {
    // ---- cut the next batch off the worst end; finished tracks found on the way move to the destination
    int nb = 0, taken = 0;
    bool full = false;
    for (int base = 0; base < nw && !full; base += 64) {
      const int k = base + lane;
      const bool valid = k < nw;
      const int i = valid ? s.wtrk[nw - 1 - k] : 0;
      const bool fin = valid && s.pos[i] == s.len[i];
      const bool going = valid && !fin;
      const u64 mask = __ballot(going);
      const int need = a.batch_size - nb, cnt = __builtin_popcountll(mask);
      int limit = 64;
      if (cnt >= need) {      // the batch fills up in this chunk: at the lane of its need-th track
        const bool last = going && __builtin_popcountll(mask & lanes_below(lane)) + 1 == need;
        limit = __builtin_ctzll(__ballot(last)) + 1;
        full = true;
      }
      const bool within = valid && lane < limit;
      if (going && within) s.btrk[nb + __builtin_popcountll(mask & lanes_below(lane))] = (u16)i;      // (end of the list first)
      nb += cnt < need ? cnt : need;
      const int here = nw - base < limit ? nw - base : limit;
      taken += here;
      u64 fmask = __ballot(fin && within);
      while (fmask) {
        const int l = __builtin_ctzll(fmask);
        fmask &= fmask - 1;
        nf = finish_track(a, e, s, __shfl(i, l), nf, lane);
      }
    }
    nw -= taken;
    if (nb == 0) break;
    __syncthreads();
    // ---- back to list order, then ordered by key: a stable sort.  Entry r of btrk is the r-th from the END of the list, so of
    // two equal keys the one with the larger r comes first.
    for (int r = lane; r < nb; r += 64) {
      const int i = s.btrk[r];
      s.bkey[r] = s.cum[i] + 0.5 * (double)((int)s.len[i] - (int)s.pos[i]);
    }
    __syncthreads();
    for (int r = lane; r < nb; r += 64) {
      const double key = s.bkey[r];
      int rank = 0;
      for (int q = 0; q < nb; ++q) {
        const double other = s.bkey[q];
        rank += (other < key || (other == key && q > r)) ? 1 : 0;
      }
      s.sb[rank] = s.btrk[r];
    }
    __syncthreads();
    if (nf > 0 && s.cum[s.sb[0]] >= s.fkey[0] + 15.0) break;      // hopeless against the best finished entry
    // ---- one character on every track of the batch
    for (int r = lane; r < nb; r += 64) {
      const int i = s.sb[r];
      const int p = s.pos[i];
      const long at = (long)a.step_off[e.trk_off + i] + p;
      a.out_when[at] = number * 1024 + r;
      const double c = s.cum[i] + a.cost[at];
      nan = nan || c != c;
      s.cum[i] = c;
      s.pos[i] = (u16)(p + 1);
    }
    if (__ballot(nan)) {
      if (lane == 0) { a.out_status[edge] = 1; a.out_count[edge] = 0; }
      return;
    }
    __syncthreads();
    // ---- back into the waiting list, unless hopeless against its current head
    for (int r = 0; r < nb; ++r) {
      const int i = s.sb[r];
      const double ci = s.cum[i];
      if (nw > 0 && ci >= s.cum[s.wtrk[0]] + 2.5) continue;
      const double key = ci + 0.5 * (double)((int)s.len[i] - (int)s.pos[i]);
      const int at = bisect_left(s.wkey, nw, key);
      shift_up(s.wkey, s.wtrk, at, nw, lane);
      s.wkey[at] = key;
      s.wtrk[at] = (u16)i;
      ++nw;
      __syncthreads();
    }
    if ((long)nw > cap) nw = (int)cap;
  }
  __syncthreads();
  // ---- what the host needs: the first beam_width finished entries, and how far every track got
  const int count = nf < a.beam_width ? nf : a.beam_width;
  for (int k = lane; k < a.beam_width; k += 64) {
    const long o = (long)edge * a.beam_width + k;
    a.out_ref[o] = k < count ? s.fref[k] : 0;
    a.out_cost[o] = k < count ? s.fkey[k] : 0.0;
  }
  for (int i = lane; i < n; i += 64) a.out_consumed[e.trk_off + i] = s.pos[i];
  if (lane == 0) { a.out_count[edge] = count; a.out_status[edge] = 0; }
}

// cost of a (track, step) pair as the host adds it: -log2(max(p, 1e-99)) * lm_weight + conf, log2 as the quotient of natural
// logarithms (math.log(p, 2)), every operation rounded on its own
__global__ __launch_bounds__(256) void edge_costs_kernel(long n_pairs, const float* __restrict__ probs, const int* __restrict__ pair_alt,
                                                         const double* __restrict__ alt_conf, double lm_weight,
                                                         double* __restrict__ cost) {
#pragma clang fp contract(off)
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_pairs) return;
  const double p = (double)probs[s];
  const double clamped = p > 1e-99 ? p : 1e-99;
  const double bits = -(log(clamped) / 0x1.62e42fefa39efp-1);      // (log(2.0), correctly rounded)
  cost[s] = bits * lm_weight + alt_conf[pair_alt[s]];
}

}  // namespace

size_t kl_edge_decode_lds_bytes(int cap_tracks) {
  const size_t C = (size_t)cap_tracks, F = C + KL_EDGE_MAX_PRE;
  return 8 * (3 * C + F) + 4 * F + 2 * 5 * C;
}

int kl_launch_edge_decode(const KlEdgeDecode& a, hipStream_t stream) {
  if (a.n_edges < 1 || a.batch_size < 1 || a.beam_width < 1 || a.cap_tracks < 1 || a.cap_tracks > KL_EDGE_MAX_TRACKS) return KL_ERR_ARG;
  if (!a.desc || !a.cum_in || !a.alt_len || !a.alt_class || !a.step_off || !a.final_slot || !a.cost) return KL_ERR_ARG;
  if (!a.out_count || !a.out_status || !a.out_ref || !a.out_cost || !a.out_consumed || !a.out_when) return KL_ERR_ARG;
  if (a.depth_k < 0 || (a.depth_k > 0 && (!a.pool || a.W < 1))) return KL_ERR_ARG;
  // (the LDS arrays are laid out for a capacity that is a multiple of 4: every array starts 8-byte aligned)
  KlEdgeDecode b = a;
  b.cap_tracks = (a.cap_tracks + 3) & ~3;
  hipLaunchKernelGGL(edge_decode_kernel, dim3(a.n_edges), dim3(64), kl_edge_decode_lds_bytes(b.cap_tracks), stream, b);
  return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH;
}

int kl_launch_edge_costs(long n_pairs, const float* probs, const int* pair_alt, const double* alt_conf, double lm_weight,
                         double* cost, hipStream_t stream) {
  if (n_pairs < 1 || !probs || !pair_alt || !alt_conf || !cost) return KL_ERR_ARG;
  hipLaunchKernelGGL(edge_costs_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, n_pairs, probs, pair_alt,
                     alt_conf, lm_weight, cost);
  return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH;
}
