// Alternatives for rating windows (kl_rate_window_alts): what the model expected instead, and how far down its list
// the character it got stands.
//
// rate_topk reads a window's logits as rate_pick does -- time-major rows, row = t*B + b -- and writes per row,
// batch-major: the probability of the target (tprob [B][T]), the K most probable characters (alt_id, alt_p [B][T][K])
// and the target's position among all V (rank [B][T], 0 = the model's first choice): 8K + 8 bytes out per row against
// the V * 4 of the whole softmax.
// A row's vocabulary is ordered by (logit descending, id ascending): v stands before u iff x[v] > x[u], or x[v] == x[u]
// and v < u.  That is a strict total order of the ids, so the selection needs no "taken" marks: round j's winner is the
// first id that stands strictly after round j-1's winner, found by a wave-wide arg-max over (value, id) pairs.  Lanes
// with nothing left carry (-inf, INT_MAX): logits are finite, so such a pair never wins against a real one, and a winner
// with an id >= V says that the vocabulary is exhausted (K > V): alt_id -1, alt_p 0 from there on.
// Maximum, sum of exponentials and every probability are computed with rate_pick's operations in rate_pick's order
// (expf(x - mx) * inv), form by form, so tprob is the float kl_rate_window delivers, and where rank < K,
// alt_p[rank] is that float again.
// Where tgt < 0 (padded tail, dummy stream) the row delivers nothing: tprob 0, ids -1, probabilities 0, rank -1.
#include <climits>

#include "kl_common.h"
#include "kl_kernels.h"

namespace {

// does (a, i) stand before (b, j)?
__device__ __forceinline__ bool before(float a, int i, float b, int j) { return a > b || (a == b && i < j); }

// REG: V <= 256 with V and ld multiples of 4 -- a lane keeps its four logits in registers, one 16-byte load (as
// rate_pick_v256_kernel); else any V, the lane's ids lane, lane + 64, ... are read again in every pass (as rate_pick_kernel)
template <bool REG>
__global__ void __launch_bounds__(256) rate_topk_kernel(const float* __restrict__ logits, long ld, int rows, int V,
                                                        const int* __restrict__ tgt, int B, int T, int K,
                                                        float* __restrict__ tprob, int* __restrict__ alt_id,
                                                        float* __restrict__ alt_p, int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = row % B, tt = row / B;
  const long at = (long)b * T + tt;
  const int y = tgt[at];
  if (y < 0) {      // (the whole wave: one row)
    if (lane < K) {
      alt_id[at * K + lane] = -1;
      alt_p[at * K + lane] = 0.f;
    }
    if (lane == 0) {
      if (tprob) tprob[at] = 0.f;
      if (rank) rank[at] = -1;
    }
    return;
  }
  const float* x = logits + (long)row * ld;
  const int v0 = lane * 4;
  const bool in = REG && v0 < V;
  float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
  if (in) {
    const float4 a = *reinterpret_cast<const float4*>(x + v0);
    r0 = a.x; r1 = a.y; r2 = a.z; r3 = a.w;
  }
  // f(id, logit) for every id of this lane, ids ascending
  auto each = [&](auto&& f) {
    if (REG) {
      if (in) {
        f(v0, r0); f(v0 + 1, r1); f(v0 + 2, r2); f(v0 + 3, r3);
      }
    } else {
      for (int v = lane; v < V; v += 64) f(v, x[v]);
    }
  };
  float mx = -INFINITY;
  each([&](int, float a) {
    if (a > mx) mx = a;
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(mx, off);
    if (o > mx) mx = o;
  }
  float sum = 0.f;
  each([&](int, float a) { sum += expf(a - mx); });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  const float inv = 1.f / sum;

  // K rounds; lane j keeps round j's winner for the store
  float pv = INFINITY, keep_p = 0.f;
  int pid = -1, keep_id = -1;
  for (int j = 0; j < K; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    each([&](int v, float a) {
      if (before(pv, pid, a, v) && before(a, v, bv, bi)) {
        bv = a;
        bi = v;
      }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (bi >= V) break;      // (wave-uniform: nothing stands after the last winner)
    if (lane == j) {
      keep_id = bi;
      keep_p = expf(bv - mx) * inv;
    }
    pv = bv;
    pid = bi;
  }
  if (lane < K) {
    alt_id[at * K + lane] = keep_id;
    alt_p[at * K + lane] = keep_p;
  }
  if (y >= V) {      // (no such character: rate_pick's 0, and no rank)
    if (lane == 0) {
      if (tprob) tprob[at] = 0.f;
      if (rank) rank[at] = -1;
    }
    return;
  }
  const float xy = x[y];
  int cnt = 0;
  each([&](int v, float a) { cnt += before(a, v, xy, y) ? 1 : 0; });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) {
    if (tprob) tprob[at] = expf(xy - mx) * inv;
    if (rank) rank[at] = cnt;
  }
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH; }

}  // namespace

int kl_launch_rate_topk(const float* logits, long ld, int rows, int V, const int* tgt, int B, int T, int K, float* tprob,
                        int* alt_id, float* alt_p, int* rank, hipStream_t stream) {
  if (!logits || !tgt || !alt_id || !alt_p || B < 1 || T < 1 || V < 1 || ld < V || (long)B * T != rows) return KL_ERR_ARG;
  if (K < 1 || K > KL_RATE_ALTS_MAX) return KL_ERR_ARG;
  dim3 grid((rows + 3) / 4);
  if (V <= 256 && (V & 3) == 0 && (ld & 3) == 0)
    hipLaunchKernelGGL(rate_topk_kernel<true>, grid, dim3(256), 0, stream, logits, ld, rows, V, tgt, B, T, K, tprob, alt_id,
                       alt_p, rank);
  else
    hipLaunchKernelGGL(rate_topk_kernel<false>, grid, dim3(256), 0, stream, logits, ld, rows, V, tgt, B, T, K, tprob, alt_id,
                       alt_p, rank);
  return ok();
}
