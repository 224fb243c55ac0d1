// Batch assembly of stateful training (kl_assemble_windows).
//
// The host advances B streams per step (lib/streams.py) and describes the batch by one int64 row per stream:
// [start, vlen, zero_col, zero_ctx, ctx_0 .. ctx_{n_ctx-1}] -- where the window starts in the id corpus, how many of its T
// positions are text (the tail window of a file or segment is shorter), which input column and which context variable
// the train=True augmentation zeroes (-1: none), and the stream's context values.  This kernel turns the rows into
// the three arrays the window calls read, exactly as StreamBatcher.assemble_host does:
//   idx[b][t]    = t < vlen && t != zero_col ? corpus[start + t] : 0
//   tgt[b][t]    = t < vlen ? corpus[start + t + 1] : -1
//   ctx[b][t][c] = t < vlen && c != zero_ctx ? ctx_c : 0
// One workgroup per stream.  The plan row is read through uniform addresses (scalar loads, once per wave); the vlen + 1
// ids of the window come in as lane-consecutive dwords (`start` has no alignment) and are parked in LDS; every thread then
// owns four consecutive output positions and stores them as one 16-byte word.  A row of T or T * n_ctx dwords need not
// start on a 16-byte boundary (T = 7; n_ctx = 3): the up to three positions in front of the first boundary and the
// remainder behind the last whole group leave as single dwords.  Corpus addresses are 64-bit (up to 2^30 ids and more);
// an id at or beyond n_corpus (or in front of 0) reads as 0 without touching memory.
#include "keraslm_hip.h"
#include "kl_common.h"

namespace {

constexpr int KL_ASM_MAX_T = 1024;
constexpr int KL_ASM_MAX_CTX = 8;

// out[0 .. n): four consecutive positions per thread as one 16-byte store from the first 16-byte boundary on, single
// dwords in front of it and behind the last whole group
template <class F>
__device__ __forceinline__ void emit_row(int32_t* __restrict__ out, int n, F value) {
  const int lead = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) >> 2);
  if ((int)threadIdx.x < lead && (int)threadIdx.x < n) out[threadIdx.x] = value((int)threadIdx.x);
  for (int p = lead + 4 * (int)threadIdx.x; p < n; p += 4 * (int)blockDim.x) {
    if (p + 4 <= n) {
      int4 v;
      v.x = value(p);
      v.y = value(p + 1);
      v.z = value(p + 2);
      v.w = value(p + 3);
      *reinterpret_cast<int4*>(out + p) = v;
    } else {
      for (int k = 0; k < 4; ++k)
        if (p + k < n) out[p + k] = value(p + k);
    }
  }
}

__global__ void __launch_bounds__(256) assemble_windows_kernel(const int32_t* __restrict__ corpus, long long n_corpus,
                                                               const long long* __restrict__ plan, int T, int n_ctx,
                                                               int32_t* __restrict__ idx, int32_t* __restrict__ ctx,
                                                               int32_t* __restrict__ tgt) {
  __shared__ int32_t s_ids[KL_ASM_MAX_T + 4];
  __shared__ int32_t s_ctx[KL_ASM_MAX_CTX];
  const int b = blockIdx.x;
  const long long* row = plan + (long long)b * (4 + n_ctx);
  const long long start = row[0];
  const long long vl = row[1], zc = row[2], zx = row[3];
  const int vlen = vl < 0 ? 0 : (vl > T ? T : (int)vl);
  const int zero_col = (zc >= 0 && zc < T) ? (int)zc : -1;
  const int zero_ctx = (zx >= 0 && zx < n_ctx) ? (int)zx : -1;
  // the window's ids and the one behind it (the last target): vlen + 1 lane-consecutive dwords
  if (vlen > 0)
    for (int i = threadIdx.x; i <= vlen; i += blockDim.x) {
      const long long g = start + i;
      s_ids[i] = (g >= 0 && g < n_corpus) ? corpus[g] : 0;
    }
  if ((int)threadIdx.x < n_ctx) s_ctx[threadIdx.x] = (int)threadIdx.x == zero_ctx ? 0 : (int32_t)row[4 + threadIdx.x];
  __syncthreads();
  const long long at = (long long)b * T;
  emit_row(idx + at, T, [&](int t) { return (t < vlen && t != zero_col) ? s_ids[t] : 0; });
  emit_row(tgt + at, T, [&](int t) { return t < vlen ? s_ids[t + 1] : -1; });
  if (n_ctx > 0) {
    const int live = vlen * n_ctx;      // the text positions come first in the row: [t][c]
    emit_row(ctx + at * n_ctx, T * n_ctx, [&](int r) { return r < live ? s_ctx[r % n_ctx] : 0; });
  }
}

}  // namespace

extern "C" int kl_assemble_windows(const int32_t* corpus, size_t n_corpus, const int64_t* plan, int B, int T, int n_ctx,
                                   int32_t* idx, int32_t* ctx, int32_t* tgt, void* stream) {
  if (!corpus || !plan || !idx || !tgt || B < 1 || T < 1 || T > KL_ASM_MAX_T) return KL_ERR_ARG;
  if (n_ctx < 0 || n_ctx > KL_ASM_MAX_CTX || (n_ctx > 0 && !ctx)) return KL_ERR_ARG;
  if (n_corpus > (size_t)1 << 40) return KL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(corpus) & 3) || (reinterpret_cast<uintptr_t>(plan) & 7) ||
      (reinterpret_cast<uintptr_t>(idx) & 3) || (reinterpret_cast<uintptr_t>(ctx) & 3) ||
      (reinterpret_cast<uintptr_t>(tgt) & 3))
    return KL_ERR_ARG;
  // a thread owns four positions: as many waves as the longest row (the contexts') needs, at most four
  const int longest = T * (n_ctx > 1 ? n_ctx : 1);
  int threads = ((longest + 3) / 4 + 63) / 64 * 64;
  if (threads > 256) threads = 256;
  hipLaunchKernelGGL(assemble_windows_kernel, dim3(B), dim3(threads), 0, static_cast<hipStream_t>(stream), corpus,
                     (long long)n_corpus, reinterpret_cast<const long long*>(plan), T, n_ctx, idx, ctx, tgt);
  return hipGetLastError() == hipSuccess ? KL_OK : KL_ERR_LAUNCH;
}
