// Target-only delivery for rating windows (kl_rate_window).
//
// A rater looks at ONE number per character: the probability of the character that actually follows
// (rating.py:493-529).  rate_pick reads a window's logits -- time-major rows, row = t*B + b, as the
// softmax_ce kernels of elementwise.hip read them -- and writes that one float per row, batch-major
// [B][T]: 4 bytes out per row against the V * 4 of the whole softmax, and nothing is written back over
// the logits.  Maximum, sum of exponentials and the picked probability are computed with the operations
// of softmax_ce_kernel / softmax_ce_v256_kernel in their order (expf(x - mx) * inv), so the result is the
// element kl_forward_window would have delivered at that index.
// rate_bits sums -log2(max(p, 1e-99)) (rating.py:531-576) over the valid positions of every stream in f64,
// one wave per stream, in a fixed order: two runs on the same inputs give the same bits.
#include "kl_common.h"
#include "kl_kernels.h"

namespace {

// any V: the strided form (softmax_ce_kernel's passes without its write-back)
__global__ void __launch_bounds__(256) rate_pick_kernel(const float* __restrict__ logits, long ld, int rows, int V,
                                                        const int* __restrict__ tgt, int B, int T,
                                                        float* __restrict__ tprob) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* x = logits + (long)row * ld;
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) {
    const float a = x[v];
    if (a > mx) mx = a;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(mx, off);
    if (o > mx) mx = o;
  }
  float sum = 0.f;
  for (int v = lane; v < V; v += 64) sum += expf(x[v] - mx);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  const float inv = 1.f / sum;
  const int b = row % B, tt = row / B;
  const long at = (long)b * T + tt;
  const int t = tgt[at];
  if (lane == 0) tprob[at] = (t >= 0 && t < V) ? expf(x[t] - mx) * inv : 0.f;
}

// V <= 256 with V and ld multiples of 4: a lane keeps its four logits in registers, one 16-byte load, one pass
__global__ void __launch_bounds__(256) rate_pick_v256_kernel(const float* __restrict__ logits, long ld, int rows, int V,
                                                             const int* __restrict__ tgt, int B, int T,
                                                             float* __restrict__ tprob) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* x = logits + (long)row * ld;
  const int v0 = lane * 4;
  const bool in = v0 < V;
  const float4 a = in ? *reinterpret_cast<const float4*>(x + v0) : float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  float e[4] = {a.x, a.y, a.z, a.w};
  float mx = e[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (e[k] > mx) mx = e[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(mx, off);
    if (o > mx) mx = o;
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = in ? expf(e[k] - mx) : 0.f;
    sum += e[k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  const float inv = 1.f / sum;
  const int b = row % B, tt = row / B;
  const long at = (long)b * T + tt;
  const int t = tgt[at];
  float pt = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (v0 + k == t) pt = e[k] * inv;
  // (exactly one lane holds a non-zero term: the sum over the wave is that term itself)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pt += __shfl_xor(pt, off);
  if (lane == 0) tprob[at] = pt;
}

// bits[b] += sum over the positions t with tgt[b][t] >= 0 of -log2(max(tprob[b][t], 1e-99)); one wave per stream:
// lane j adds up t = j, j + 64, ... in index order, then the 64 partial sums are folded in a fixed butterfly
__global__ void __launch_bounds__(256) rate_bits_kernel(const float* __restrict__ tprob, const int* __restrict__ tgt, int B,
                                                        int T, double* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* p = tprob + (long)b * T;
  const int* y = tgt + (long)b * T;
  double acc = 0.0;
  for (int t = lane; t < T; t += 64)
    if (y[t] >= 0) acc -= log2(fmax((double)p[t], 1e-99));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) bits[b] += acc;
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH; }

}  // namespace

int kl_launch_rate_pick(const float* logits, long ld, int rows, int V, const int* tgt, int B, int T, float* tprob,
                        hipStream_t stream) {
  if (!logits || !tgt || !tprob || rows != B * T) return KL_ERR_ARG;
  dim3 grid((rows + 3) / 4);
  if (V <= 256 && (V & 3) == 0 && (ld & 3) == 0)
    hipLaunchKernelGGL(rate_pick_v256_kernel, grid, dim3(256), 0, stream, logits, ld, rows, V, tgt, B, T, tprob);
  else
    hipLaunchKernelGGL(rate_pick_kernel, grid, dim3(256), 0, stream, logits, ld, rows, V, tgt, B, T, tprob);
  return ok();
}

int kl_launch_rate_bits(const float* tprob, const int* tgt, int B, int T, double* bits, hipStream_t stream) {
  if (!tprob || !tgt || !bits) return KL_ERR_ARG;
  hipLaunchKernelGGL(rate_bits_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, tprob, tgt, B, T, bits);
  return ok();
}
