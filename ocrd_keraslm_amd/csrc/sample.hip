// Sampling (kl_sample_pick): draw one character per row where the probabilities are.
//
// After kl_step_batch the probabilities of all chains lie in HBM as probs [rows][V].  sample_pick_kernel reads a row as
// rate_topk does -- one wave per row, four rows per workgroup -- and writes 12 bytes per row: the drawn id, the chain's
// running cost and (for the log) the uniform number it drew with.  The contract is in include/keraslm_hip.h, its numpy
// statement in lib/gensample.py; in short, per row r:
//   u           Philox4x32-10, key = the seed's two halves, counter (step, row0 + r, 0, 0), first output word >> 8, * 2^-24;
//   candidates  the valid ids; with top_k > 0 the first top_k of them by (p descending, id ascending) -- rate_topk's total
//               order, found like there by rounds of a wave-wide arg-max, each round skipping what stands before the last
//               winner --; of those the ones with p >= floor; if none is left, the first valid id of that order alone;
//   weights     p, or expf((logf(p) - logf(p_max)) / temperature); 0 for p == 0 and for every id that is no candidate;
//   pick        temperature 0: the first candidate; else the smallest id of positive weight whose running weight sum
//               (ids ascending) exceeds u * S.
// Ids are dealt to lanes in chunks of 64 (id = 64 k + lane), so ascending ids are ascending (chunk, lane) pairs and the
// running sums are one wave-wide inclusive scan per chunk plus the carry of the chunks before: a fixed order of additions,
// so two calls on the same inputs pick bit-identically.
// REG (V <= 256): the four values of a lane and their weights stay in registers.  Else any V: the values are read again in
// every pass, and the weights lie in the workspace between the pass that sums them and the pass that picks (each lane reads
// back only what it wrote itself, so nothing has to be waited for).
// Plain loads and vector stores only; no wave waits for another.
#include <climits>

#include "kl_common.h"
#include "kl_kernels.h"

namespace {

// does (a, i) stand before (b, j)?
__device__ __forceinline__ bool before(float a, int i, float b, int j) { return a > b || (a == b && i < j); }

// Philox4x32-10 on counter (c0, c1, 0, 0): the first output word as a float in [0, 1), 24 bits (integer arithmetic and one
// exact conversion: gensample.philox_uniform gives the same bits)
__device__ __forceinline__ float philox_u01(unsigned k0, unsigned k1, unsigned c0, unsigned c1) {
  unsigned c2 = 0, c3 = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * 0x1p-24f;
}

// inclusive sums over the lanes 0 .. lane
__device__ __forceinline__ float wave_scan(float x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_up(x, off);
    if (lane >= off) x += o;
  }
  return x;
}

template <bool REG>
__global__ void __launch_bounds__(256) sample_pick_kernel(const KlSamplePick a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;      // (whole waves leave; there is no barrier in this kernel)
  const int V = a.V;
  const float* x = a.probs + (long)row * V;
  const float u = philox_u01(a.key0, a.key1, a.step, a.row0 + (unsigned)row);
  const int chunks = REG ? 4 : (V + 63) >> 6;
  const float T = a.temperature, floor = a.floor;

  float r[4] = {0.f, 0.f, 0.f, 0.f};      // REG: the lane's values; ok: bit k = id 64 k + lane exists and is valid
  unsigned ok = 0;
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = k * 64 + lane;
      if (v < V) {
        r[k] = x[v];
        if (a.valid ? a.valid[v] != 0 : v != 0) ok |= 1u << k;
      }
    }
  }

  // the first candidate, and with top_k the last of the first top_k valid ids that reach the floor
  const int K = T == 0.f || a.top_k < 1 ? 1 : a.top_k;
  float first_p = 0.f, last_p = INFINITY;
  int first_id = INT_MAX, last_id = -1;
  for (int j = 0; j < K; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int k = 0; k < chunks; ++k) {
      const int v = k * 64 + lane;
      if constexpr (REG) {
        if ((ok >> k & 1u) && before(last_p, last_id, r[k], v) && before(r[k], v, bv, bi)) {
          bv = r[k];
          bi = v;
        }
      } else if (v < V) {
        const float p = x[v];
        // (the mask is looked at last: only for a value that would take the lane's lead)
        if (before(last_p, last_id, p, v) && before(p, v, bv, bi) && (a.valid ? a.valid[v] != 0 : v != 0)) {
          bv = p;
          bi = v;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    // (every lane now holds the same winner)
    if (bi == INT_MAX) break;      // no valid id is left
    if (j == 0) {
      first_p = bv;
      first_id = bi;
    }
    if (!(bv >= floor)) break;      // below the floor -- as is every later winner
    last_p = bv;
    last_id = bi;
  }

  int pick = 0;
  if (first_id != INT_MAX) {
    pick = first_id;
    if (T != 0.f) {
      const bool single = !(first_p >= floor);      // nothing reaches the floor: the first valid id alone
      const bool cut = a.top_k > 0;
      const float lmax = logf(first_p);
      auto weight = [&](int v, float p, bool valid) -> float {
        const bool cand = valid && (single ? v == first_id : (p >= floor && !(cut && before(last_p, last_id, p, v))));
        if (!cand || !(p > 0.f)) return 0.f;
        return T == 1.f ? p : expf((logf(p) - lmax) / T);
      };
      float w[4] = {0.f, 0.f, 0.f, 0.f};
      float* wrow = REG ? nullptr : a.w + (long)row * V;
      // S: the running sum after the last id
      float carry = 0.f;
      for (int k = 0; k < chunks; ++k) {
        const int v = k * 64 + lane;
        float wv = 0.f;
        if constexpr (REG) {
          wv = w[k] = weight(v, r[k], ok >> k & 1u);
        } else if (v < V) {
          wv = weight(v, x[v], a.valid ? a.valid[v] != 0 : v != 0);
          wrow[v] = wv;
        }
        carry = __shfl(carry + wave_scan(wv, lane), 63);
      }
      const float target = u * carry;
      // the same sums again: the first id of positive weight beyond the target, and the last id of positive weight
      int hit = INT_MAX, tail = -1;
      carry = 0.f;
      for (int k = 0; k < chunks; ++k) {
        const int v = k * 64 + lane;
        float wv = 0.f;
        if constexpr (REG) {
          wv = w[k];
        } else if (v < V) {
          wv = wrow[v];
        }
        const float run = carry + wave_scan(wv, lane);
        carry = __shfl(run, 63);
        if (wv > 0.f) {
          tail = v;
          if (run > target && hit == INT_MAX) hit = v;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int oh = __shfl_xor(hit, off), ot = __shfl_xor(tail, off);
        hit = oh < hit ? oh : hit;
        tail = ot > tail ? ot : tail;
      }
      if (hit != INT_MAX)
        pick = hit;
      else if (tail >= 0)      // rounding left no sum beyond the target
        pick = tail;
      // (no positive weight at all -- the candidates' probabilities are all 0 --: the first candidate stays)
    }
  }
  if (lane == 0) {
    const float cost = first_id != INT_MAX ? -logf(x[pick]) : INFINITY;
    const float cum = a.cum_in[row] + cost;      // (read before the store: cum_in and cum_next may be one array)
    a.idx_next[row] = pick;
    a.cum_next[row] = cum;
    if (a.u_log) a.u_log[row] = u;
  }
}

}  // namespace

size_t kl_sample_ws_bytes(int rows, int V) { return ((size_t)rows * V * sizeof(float) + 255) / 256 * 256; }

int kl_launch_sample_pick(KlSamplePick a, void* ws, hipStream_t stream) {
  if (a.rows < 1 || a.rows > KL_SAMPLE_MAX_ROWS || a.V < 1 || a.top_k < 0 || a.top_k > KL_SAMPLE_MAX_TOPK) return KL_ERR_ARG;
  if (!(a.temperature >= 0.f) || a.temperature == INFINITY || !(a.floor >= 0.f)) return KL_ERR_ARG;
  if (!a.probs || !a.cum_in || !a.idx_next || !a.cum_next || !ws) return KL_ERR_ARG;
  a.w = reinterpret_cast<float*>(ws);
  const dim3 grid((a.rows + 3) / 4);
  if (a.V <= 256)
    hipLaunchKernelGGL(sample_pick_kernel<true>, grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(sample_pick_kernel<false>, grid, dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH;
}
