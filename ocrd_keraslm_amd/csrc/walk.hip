// Edge walk (kl_walk_batch_host): the deferred output layer of a whole lattice edge in ONE launch.
//
// A lattice edge (rating.py:796-851) knows every character its hypotheses will feed, so kl_walk_batch_host runs the
// recurrence of all rows over all their steps with nothing but cell launches (step_small.hip) and leaves the top layer's h
// of every (row, step) pair in that pair's pool slot.  What the decoder looks at is one number per pair: the softmax
// probability of the character the row consumes next.  walk_out_kernel delivers exactly those:
//   * a workgroup takes 16 pairs (one MFMA row tile); every lane reads its pair's state row through the pair's slot,
//     splits it into bf16 hi + lo in registers (no LDS staging, no barrier in the loop: a row tile is read by the eight
//     waves of one workgroup only, out of L2);
//   * wave w contracts column tiles 2w, 2w + 1 (then + 16, ...) of the tied embedding, read fragment-major (one contiguous
//     KiB per wave instruction, see step_tile.hip's frag_major_kernel), three MFMAs per fragment pair in split precision
//     -- hi.hi + lo.hi + hi.lo, the order of out_softmax_kernel and of the thin GEMM;
//   * the logits never leave the registers: every lane keeps a running maximum and sum of its column per row, picks the
//     target's logit when its column is the target, the 16 columns are folded by a butterfly, the eight waves through LDS in
//     a fixed order (two calls on the same inputs are bit-identical, and a pair's result does not depend on its tile row);
//   * 4 bytes per pair go to host memory; further workgroups copy the heads of the rows' final states;
//   * arrival as in step_finish_kernel: every workgroup fences at system scope and takes a ticket, the last one resets the
//     counter and releases the arrival word.
// No [total][V] array goes through HBM.  Serves every vocabulary and width the library accepts (W % 32 == 0).
#include "kl_common.h"
#include "kl_kernels.h"

namespace {

// (m, s) <- (m, s) + (mo, so): maximum and sum of exp(x - maximum).  No contraction here: the four rows a lane holds go
// through four unrolled copies of this, and hipcc fuses s * e + so * eo into an FMA around one product in some copies and
// around the other in others -- a pair's probability then depends on its row in the tile (seen: duplicate rows 2 ulp apart).
__device__ __forceinline__ void walk_fold(float& m, float& s, float mo, float so) {
#pragma clang fp contract(off)
  const float mn = fmaxf(m, mo);
  if (mn > -INFINITY) s = s * expf(m - mn) + so * expf(mo - mn);
  m = mn;
}

template <bool LO>
__global__ __launch_bounds__(512) void walk_out_kernel(const KlWalkOut a) {
  constexpr int NPL = LO ? 2 : 1;
  __shared__ float red_m[8][16];
  __shared__ float red_s[8][16];
  __shared__ float tlog[16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int n_tiles = (a.total + 15) >> 4;
  if ((int)blockIdx.x < n_tiles) {
    const int W = a.W, V = a.V;
    const int r0 = blockIdx.x * 16;
    // A operand: lane holds k 8 fq .. + 7 of pair r0 + fr (pairs beyond the end repeat the last one; never delivered)
    const float* arow = a.pool + (long)a.slots[min(r0 + fr, a.total - 1)] * a.slot_ld + a.h_off + fq * 8;
    // D: lane holds column fr of rows 4 fq + j
    int tg[4];
    float m[4], s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = r0 + 4 * fq + j;
      tg[j] = p < a.total ? a.targets[p] : -1;
      m[j] = -INFINITY;
      s[j] = 0.f;
    }
    if (tid < 16) tlog[tid] = 0.f;
    __syncthreads();
    const int nkb = W >> 5;
    const int nvt = (V + 15) >> 4;      // (the fragment-major embedding has round_up(V, 32) / 16 tiles, pad rows zero)
    for (int vt = wave * 2; vt < nvt; vt += 16) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const bf16_t* e0 = a.EF + (long)vt * nkb * NPL * 512 + lane * 8;
      const bf16_t* e1 = e0 + (long)nkb * NPL * 512;
      for (int kb = 0; kb < nkb; ++kb) {
        const float4 x0 = *reinterpret_cast<const float4*>(arow + kb * 32);
        const float4 x1 = *reinterpret_cast<const float4*>(arow + kb * 32 + 4);
        const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        frag16 ah, al, bh, bl;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          ah.s[i] = f2bf(x[i]);
          if (LO) al.s[i] = f2bf(x[i] - bf2f(ah.s[i]));
        }
        bh.u = *reinterpret_cast<const uint4*>(e0 + (long)kb * NPL * 512);
        acc0 = mfma16(ah.v, bh.v, acc0);
        if (LO) {
          bl.u = *reinterpret_cast<const uint4*>(e0 + (long)kb * NPL * 512 + 512);
          acc0 = mfma16(al.v, bh.v, acc0);
          acc0 = mfma16(ah.v, bl.v, acc0);
        }
        bh.u = *reinterpret_cast<const uint4*>(e1 + (long)kb * NPL * 512);
        acc1 = mfma16(ah.v, bh.v, acc1);
        if (LO) {
          bl.u = *reinterpret_cast<const uint4*>(e1 + (long)kb * NPL * 512 + 512);
          acc1 = mfma16(al.v, bh.v, acc1);
          acc1 = mfma16(ah.v, bl.v, acc1);
        }
      }
      const int v0 = vt * 16 + fr, v1 = v0 + 16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (v0 < V) {
          walk_fold(m[j], s[j], acc0[j], 1.f);
          if (v0 == tg[j]) tlog[4 * fq + j] = acc0[j];
        }
        if (v1 < V) {
          walk_fold(m[j], s[j], acc1[j], 1.f);
          if (v1 == tg[j]) tlog[4 * fq + j] = acc1[j];
        }
      }
    }
    // the 16 columns of a row: butterfly over the low four lane bits (both partners compute the same sum)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float mo = __shfl_xor(m[j], off), so = __shfl_xor(s[j], off);
        walk_fold(m[j], s[j], mo, so);
      }
    }
    if (fr == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        red_m[wave][4 * fq + j] = m[j];
        red_s[wave][4 * fq + j] = s[j];
      }
    }
    __syncthreads();
    if (tid < 16 && r0 + tid < a.total) {
      float mm = red_m[0][tid], ss = red_s[0][tid];
#pragma unroll
      for (int w = 1; w < 8; ++w) walk_fold(mm, ss, red_m[w][tid], red_s[w][tid]);
      const int t = a.targets[r0 + tid];
      a.tprob_host[r0 + tid] = (t >= 0 && t < V) ? expf(tlog[tid] - mm) / ss : 0.f;
    }
  } else {
    // heads of the rows' final states: the first head_k * W floats of a slot, one row per wave
    const int row = ((int)blockIdx.x - n_tiles) * 8 + wave;
    if (row < a.n) {
      const float4* src = reinterpret_cast<const float4*>(a.pool + (long)a.last[row] * a.slot_ld);
      float4* dst = reinterpret_cast<float4*>(a.heads_host + (long)row * a.head_k * a.W);
      const int n4 = a.head_k * a.W / 4;
      for (int i = lane; i < n4; i += 64) dst[i] = src[i];
    }
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned got = atomicAdd(a.counter, 1u);
    if (got == gridDim.x - 1) {
      atomicExch(a.counter, 0u);
      __threadfence_system();
      __hip_atomic_store(a.done_host, a.ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

int kl_launch_walk_out(const KlWalkOut& a, hipStream_t stream) {
  if (a.total < 1 || a.n < 1 || a.V < 1 || a.W < 32 || (a.W & 31)) return KL_ERR_SHAPE;
  if (!a.pool || !a.EF || !a.slots || !a.targets || !a.tprob_host || !a.done_host || !a.counter) return KL_ERR_ARG;
  if (a.head_k > 0 && (!a.last || !a.heads_host)) return KL_ERR_ARG;
  const int grid = (a.total + 15) / 16 + (a.head_k > 0 ? (a.n + 7) / 8 : 0);
  if (a.lo) hipLaunchKernelGGL(walk_out_kernel<true>, dim3(grid), dim3(512), 0, stream, a);
  else hipLaunchKernelGGL(walk_out_kernel<false>, dim3(grid), dim3(512), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH;
}
