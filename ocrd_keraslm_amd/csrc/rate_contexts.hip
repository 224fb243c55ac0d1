// Rating under candidate contexts (kl_rate_scatter_planes, kl_context_mix): which context does a text read like?
//
// Rater.rate_contexts rates every text under each of C caller-supplied context tuples in ONE bulk plan: the plan rows are
// the n * C pairs (text, candidate) over the shared id corpus, so kl_assemble_windows serves unchanged and a job of 64
// documents fills the wide scans as 1280 rows.  The way back differs from kl_rate_scatter in one word per row: the
// candidate a row was rated under names the PLANE of a [C][ld] array its probabilities go to.  kl_context_mix then reads
// the C planes of every text side by side: the bits under each candidate, the posterior over the candidates, the best one
// and its margin, and per character the probability under the sequential Bayesian mixture of the candidates -- the weight of
// candidate c at position j is its prior times the probability it gave to everything in front of j.
//
// Decomposition of the mix: one workgroup of four waves per text, the text in tiles of 64 consecutive positions.  A wave owns
// the candidates c = wave, wave + 4, ...: lane p reads planes[c][j0 + p] -- 64 consecutive floats, one 256-byte line per
// candidate however far the planes lie apart --, takes the f64 log2 (every lane one: this is where the logs run in
// parallel), and a six-step shuffle scan over the lanes gives the exclusive prefix; the sum in front of the tile is a value
// per candidate kept in LDS by the wave that owns it.  With lw = prior + prefix each lane folds its candidates into a
// running (max, sum of weights, sum of weights * q) in ascending c, rescaling when the maximum moves; wave 0 folds the four
// waves' triples in wave order, writes 64 consecutive floats of the mixture and adds its own log.  Every order is fixed by
// indices alone: no atomics, no workgroup waits for another, two calls on the same input agree bit for bit.  The triples are
// double-buffered by tile parity, so a tile costs one barrier.  A line of 30 characters is one tile of one workgroup; a
// document of 100 000 characters is 1563 tiles of one workgroup -- serial, as the recurrence that produced the planes was,
// and a few microseconds per tile against that recurrence's 100 000 steps.  None depends on a model: no handle.
#include "keraslm_hip.h"
#include "kl_common.h"

namespace {

constexpr int KL_SCATTER_MAX_CTX = 8;      // (the plan rows are kl_assemble_windows': 4 + n_ctx words)
constexpr int MIX_WAVES = 4;
constexpr double MIX_FLOOR = 1e-99;        // (rating.py:531-576: the floor under a probability before its log)

// one workgroup per stream: out[plane[b]][start + 1 + t] = tprob[b][t] for the text positions of the row, moved as 32-bit words
__global__ void __launch_bounds__(256) rate_scatter_planes_kernel(const uint32_t* __restrict__ tprob,
                                                                  const long long* __restrict__ plan,
                                                                  const int* __restrict__ plane, int T, int n_ctx, int C,
                                                                  uint32_t* __restrict__ out, long long ld, long long n_out) {
  const int b = blockIdx.x;
  const int c = plane[b];
  if (c < 0 || c >= C) return;
  const long long* row = plan + (long long)b * (4 + n_ctx);
  const long long start = row[0], vl = row[1];
  const int vlen = vl < 0 ? 0 : (vl > T ? T : (int)vl);
  const uint32_t* p = tprob + (long long)b * T;
  uint32_t* to = out + (long long)c * ld;
  for (int t = threadIdx.x; t < vlen; t += blockDim.x) {
    const long long g = start + 1 + t;
    if (g >= 0 && g < n_out) to[g] = p[t];
  }
}

__device__ __forceinline__ double shfl_up_f64(double v, int off) { return __shfl_up(v, off); }

// fold one more weighted term into a running (M, S, N): S = sum 2^(lw - M), N = sum 2^(lw - M) * q, M the largest lw so far
__device__ __forceinline__ void mix_fold(double& M, double& S, double& N, double lw, double s, double n) {
  if (lw == -INFINITY) return;      // (weight 0: a candidate the prior rules out, or a wave without a candidate)
  if (lw > M) {
    const double e = exp2(M - lw);      // (M = -inf: 0, and S = N = 0 anyway)
    S = S * e + s;
    N = N * e + n;
    M = lw;
  } else {
    const double e = exp2(lw - M);
    S += e * s;
    N += e * n;
  }
}

__global__ void __launch_bounds__(64 * MIX_WAVES) context_mix_kernel(const float* __restrict__ planes, long long ld,
                                                                     const long long* __restrict__ offsets, int C,
                                                                     const double* __restrict__ log2prior,
                                                                     float* __restrict__ mix, double* __restrict__ cand_bits,
                                                                     double* __restrict__ mix_bits, double* __restrict__ post,
                                                                     int* __restrict__ best, double* __restrict__ margin) {
  __shared__ double sum_s[KL_CTX_CAND_MAX];             // per candidate: sum of log2 q in front of the tile
  __shared__ double prior_s[KL_CTX_CAND_MAX];           // per candidate: log2 of its prior (0: uniform)
  __shared__ double part_s[2][3][MIX_WAVES][64];        // per tile parity: (M, S, N) of every wave and lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x;
  long long first = offsets[i] + 1, end = offsets[i + 1];
  if (first < 1) first = 1;
  if (end > ld) end = ld;                               // (nothing outside the planes is read)
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    sum_s[c] = 0.0;
    prior_s[c] = log2prior ? log2prior[c] : 0.0;
  }
  __syncthreads();
  double bits_acc = 0.0;                                // (wave 0: -sum log2 r of the lane's positions)
  int parity = 0;
  for (long long j0 = first; j0 < end; j0 += 64, parity ^= 1) {
    const long long j = j0 + lane;
    const bool live = j < end;
    double M = -INFINITY, S = 0.0, N = 0.0;
    float next = (live && wave < C) ? planes[(long long)wave * ld + j] : 1.0f;
    for (int c = wave; c < C; c += MIX_WAVES) {
      const float p = next;
      if (live && c + MIX_WAVES < C) next = planes[(long long)(c + MIX_WAVES) * ld + j];
      const double q = fmax((double)p, MIX_FLOOR);      // (fmax: a NaN counts as the floor)
      const double l = live ? log2(q) : 0.0;
      double incl = l;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double v = shfl_up_f64(incl, off);
        if (lane >= off) incl += v;
      }
      const double before = sum_s[c];                   // (written by this wave alone, by all its lanes alike)
      const double total = __shfl(incl, 63);
      sum_s[c] = before + total;
      double excl = shfl_up_f64(incl, 1);
      if (lane == 0) excl = 0.0;
      const double lw = prior_s[c] + (before + excl);
      mix_fold(M, S, N, lw, 1.0, q);
    }
    part_s[parity][0][wave][lane] = M;
    part_s[parity][1][wave][lane] = S;
    part_s[parity][2][wave][lane] = N;
    __syncthreads();
    if (wave == 0) {
      double Mt = -INFINITY, St = 0.0, Nt = 0.0;
#pragma unroll
      for (int w = 0; w < MIX_WAVES; ++w)
        mix_fold(Mt, St, Nt, part_s[parity][0][w][lane], part_s[parity][1][w][lane], part_s[parity][2][w][lane]);
      if (live) {
        const double r = Nt / St;
        if (mix) mix[j] = (float)r;
        bits_acc -= log2(r);
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  // the text's own results, wave 0: lane l takes the candidates l, l + 64, ... in ascending order, then fixed butterflies
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bits_acc += __shfl_xor(bits_acc, off);
  if (lane == 0) mix_bits[i] = bits_acc;
  double top = -INFINITY;
  int arg = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const double s = sum_s[c];
    cand_bits[(long long)i * C + c] = 0.0 - s;
    const double lw = prior_s[c] + s;
    if (arg == 0x7fffffff || lw > top) { top = lw; arg = c; }      // (ascending c: the smallest of equal ones stays)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(top, off);
    const int a = __shfl_xor(arg, off);
    if (a != 0x7fffffff && (arg == 0x7fffffff || o > top || (o == top && a < arg))) { top = o; arg = a; }
  }
  // (NaN weights -- a +inf and a -inf log in one candidate -- compare false everywhere: the smallest index a lane saw wins)
  double second = -INFINITY, wsum = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double lw = prior_s[c] + sum_s[c];
    if (c != arg && lw > second) second = lw;
    if (lw != -INFINITY) wsum += exp2(lw - top);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    second = fmax(second, __shfl_xor(second, off));
    wsum += __shfl_xor(wsum, off);
  }
  for (int c = lane; c < C; c += 64) {
    const double lw = prior_s[c] + sum_s[c];
    post[(long long)i * C + c] = (lw != -INFINITY ? exp2(lw - top) : 0.0) / wsum;
  }
  if (lane == 0) {
    best[i] = arg;
    margin[i] = second == -INFINITY ? INFINITY : top - second;
  }
}

}  // namespace

extern "C" int kl_rate_scatter_planes(const float* tprob, const int64_t* plan, const int32_t* plane, int B, int T, int n_ctx, int C,
                                      float* out, size_t ld, size_t n_out, void* stream) {
  if (!tprob || !plan || !plane || !out || B < 1 || T < 1 || C < 1 || C > KL_CTX_CAND_MAX) return KL_ERR_ARG;
  if (n_ctx < 0 || n_ctx > KL_SCATTER_MAX_CTX || ld < n_out || ld > (size_t)1 << 40) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(tprob) & 3) || (reinterpret_cast<uintptr_t>(plan) & 7) ||
      (reinterpret_cast<uintptr_t>(plane) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
    return KL_ERR_ARG;
  int threads = (T + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  hipLaunchKernelGGL(rate_scatter_planes_kernel, dim3(B), dim3(threads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint32_t*>(tprob), reinterpret_cast<const long long*>(plan), plane, T, n_ctx, C,
                     reinterpret_cast<uint32_t*>(out), (long long)ld, (long long)n_out);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}

extern "C" int kl_context_mix(const float* planes, size_t ld, const int64_t* offsets, int n_texts, int C, const double* log2prior,
                              float* mix, double* cand_bits, double* mix_bits, double* post, int32_t* best, double* margin,
                              void* stream) {
  if (!planes || !offsets || !cand_bits || !mix_bits || !post || !best || !margin) return KL_ERR_ARG;
  if (n_texts < 1 || C < 1 || C > KL_CTX_CAND_MAX || ld < 1 || ld > (size_t)1 << 40) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(planes) & 3) || (reinterpret_cast<uintptr_t>(mix) & 3) ||
      (reinterpret_cast<uintptr_t>(best) & 3))
    return KL_ERR_ARG;
  const void* wide[] = {offsets, log2prior, cand_bits, mix_bits, post, margin};
  for (const void* p : wide)
    if (reinterpret_cast<uintptr_t>(p) & 7) return KL_ERR_ARG;
  hipLaunchKernelGGL(context_mix_kernel, dim3(n_texts), dim3(64 * MIX_WAVES), 0, static_cast<hipStream_t>(stream), planes,
                     (long long)ld, reinterpret_cast<const long long*>(offsets), C, log2prior, mix, cand_bits, mix_bits, post,
                     best, margin);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
