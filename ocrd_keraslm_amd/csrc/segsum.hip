// Layer 0's table gradients as sorted segment sums.
//   dEK[v]   = sum of the rows of dZ_0 whose character is v
//   dCtxK[c] = sum of the rows of dZ_0 whose first context value is c
// Stage 1 orders the T*B rows by the joint key (character, context value): histogram, exclusive scan, scatter over the
// ids -- three tiny kernels, rebuilt by every window.  Stage 2 reads dZ_0 ONCE: a wave walks an equal share of the
// sorted order for one slab of 512 columns (a lane owns 8 bf16 columns = one 16-byte load per row), adds rows of equal key
// into a run sum in registers, run sums into the sum of the character they belong to, and hands both to the row-major f32
// tables with hardware float atomics -- the context table once per run, the character table once per character or share.
#include "kl_common.h"
#include "kl_kernels.h"
#include "keraslm_hip.h"

namespace {

constexpr int SEG_SLAB = 512;       // columns a wave owns: 64 lanes x 8 bf16
constexpr int SEG_UNROLL = 8;       // rows whose loads a lane issues together
constexpr int SEG_SCAN_THREADS = 1024;
constexpr int SEG_SCAN_Q = 16;      // int4 groups per thread of the scan: 1024 * 16 * 4 counters, KL_SEGSUM_MAX_BUCKETS + 1 of them used

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__host__ __device__ inline long seg_pad(long n) { return (n + 63) & ~63L; }

// key of a (character, context value) pair: bucket number for the sort, packed halves for the gather pass
__device__ __forceinline__ void seg_key(const int* __restrict__ idx, const int* __restrict__ ctx, int n_ctx, long src, int V, int R,
                                        int& bucket, unsigned& packed) {
  const int v = idx[src];
  const int vv = (v >= 0 && v < V) ? v : V;
  int cc = R;      // (R = 0 without context variables: one bucket per character, its context half always invalid)
  if (n_ctx > 0) {
    const int c = ctx[src * n_ctx];
    if (c >= 0 && c < R) cc = c;
  }
  bucket = vv * (R + 1) + cc;
  packed = ((unsigned)vv << 16) | (unsigned)cc;
}

// zero fill of the bucket counters and of both result tables in one launch (n16 counts 16-byte groups)
__global__ void segsum_init_kernel(uint4* __restrict__ a, size_t na, uint4* __restrict__ b, size_t nb, uint4* __restrict__ c, size_t nc) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  for (size_t i = i0; i < na; i += stride) a[i] = uint4{0, 0, 0, 0};
  for (size_t i = i0; i < nb; i += stride) b[i] = uint4{0, 0, 0, 0};
  for (size_t i = i0; i < nc; i += stride) c[i] = uint4{0, 0, 0, 0};
}

// The lanes of a wave that hold the same bucket go to its counter together: the wave first finds its groups of equal buckets
// by ballots alone (at most 64 rounds of a few scalar instructions), then the groups' first lanes issue their atomics in ONE
// instruction -- a round trip per group would cost a wave of 64 different buckets 64 atomic latencies (measured: 0.21 ms per
// pass over the bench window's ids against 0.04).  A batch with one context value puts a fifth of all rows into one bucket:
// still one atomic per wave.  Returns the lane's slot behind the counter's old value (WANT_SLOT), else only counts.
template <bool WANT_SLOT>
__device__ __forceinline__ int seg_claim(int* __restrict__ counter, int bucket, bool todo) {
  const int lane = threadIdx.x & 63;
  int first = lane, rank = 0, count = 0;
  for (;;) {
    const unsigned long long m = __ballot(todo);
    if (!m) break;
    const int leader = __ffsll((long long)m) - 1;
    const int k0 = __shfl(bucket, leader);
    const bool same = todo && bucket == k0;
    const unsigned long long sm = __ballot(same);
    if (same) {
      first = leader;
      rank = __popcll(sm & ((1ull << lane) - 1ull));
      if (lane == leader) count = __popcll(sm);
      todo = false;
    }
  }
  int base = 0;
  if (count > 0) {
    if (WANT_SLOT) base = atomicAdd(counter + bucket, count);
    else (void)atomicAdd(counter + bucket, count);
  }
  if (!WANT_SLOT) return 0;
  return __shfl(base, first) + rank;
}

// (threads walk the ids batch-major, as they lie in memory: a wave then holds consecutive steps of ONE stream -- one context
//  value, few distinct characters -- and reads whole cache lines; the row it files is the time-major one)
__global__ void segsum_hist_kernel(const int* __restrict__ idx, const int* __restrict__ ctx, int n_ctx, int B, int T, int V, int R,
                                   int* __restrict__ hist) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;      // batch-major position b * T + t
  const bool todo = e < (long)B * T;
  int bucket = 0;
  unsigned packed;
  if (todo) seg_key(idx, ctx, n_ctx, e, V, R, bucket, packed);
  (void)seg_claim<false>(hist, bucket, todo);
}

// exclusive prefix sums of the counters, in place, one workgroup: thread i holds entries [4 * per4 * i, 4 * per4 * (i + 1))
// in registers (n4 int4 groups in all, n4 <= 1024 * SEG_SCAN_Q; the groups past the last bucket hold zeros)
__global__ __launch_bounds__(SEG_SCAN_THREADS) void segsum_scan_kernel(int4* __restrict__ h4, int n4, int per4) {
  __shared__ int wsum[SEG_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 v[SEG_SCAN_Q];
  const int g0 = tid * per4;
  int total = 0;
#pragma unroll
  for (int q = 0; q < SEG_SCAN_Q; ++q) {
    v[q] = int4{0, 0, 0, 0};
    if (q < per4 && g0 + q < n4) v[q] = h4[g0 + q];
    total += v[q].x + v[q].y + v[q].z + v[q].w;
  }
  int inc = total;      // inclusive scan over the wave, then over the waves
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int run = inc - total;
  for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
  for (int q = 0; q < SEG_SCAN_Q; ++q) {
    if (q < per4 && g0 + q < n4) {
      int4 o;
      o.x = run; run += v[q].x;
      o.y = run; run += v[q].y;
      o.z = run; run += v[q].z;
      o.w = run; run += v[q].w;
      h4[g0 + q] = o;
    }
  }
}

// order[slot] = row, skey[slot] = packed key; the counters end as the buckets' END offsets
__global__ void segsum_scatter_kernel(const int* __restrict__ idx, const int* __restrict__ ctx, int n_ctx, int B, int T, int V, int R,
                                      int* __restrict__ offs, int* __restrict__ order, unsigned* __restrict__ skey) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const bool todo = e < (long)B * T;
  int bucket = 0;
  unsigned packed = 0;
  if (todo) seg_key(idx, ctx, n_ctx, e, V, R, bucket, packed);
  const int slot = seg_claim<true>(offs, bucket, todo);
  if (todo) {
    order[slot] = (int)((e % T) * B + e / T);      // time-major row t * B + b
    skey[slot] = packed;
  }
}

__device__ __forceinline__ void seg_add_row(float (&acc)[8], const uint4 d) {
  acc[0] += __builtin_bit_cast(float, d.x << 16);
  acc[1] += __builtin_bit_cast(float, d.x & 0xffff0000u);
  acc[2] += __builtin_bit_cast(float, d.y << 16);
  acc[3] += __builtin_bit_cast(float, d.y & 0xffff0000u);
  acc[4] += __builtin_bit_cast(float, d.z << 16);
  acc[5] += __builtin_bit_cast(float, d.z & 0xffff0000u);
  acc[6] += __builtin_bit_cast(float, d.w << 16);
  acc[7] += __builtin_bit_cast(float, d.w & 0xffff0000u);
}

// a lane's 8 sums -> the table row: through the wave's LDS strip so that each atomic instruction covers 64 consecutive floats
// (lane l holds columns 8l .. 8l+7 of the slab; instruction i adds columns 64i + l)
__device__ __forceinline__ void seg_flush(float* __restrict__ strip, const float (&acc)[8], float* __restrict__ row, int col_base, int cols) {
  const int lane = threadIdx.x & 63;
  *reinterpret_cast<float4*>(strip + lane * 8) = float4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<float4*>(strip + lane * 8 + 4) = float4{acc[4], acc[5], acc[6], acc[7]};
  __builtin_amdgcn_wave_barrier();
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = strip[i * 64 + lane];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int col = col_base + i * 64 + lane;
    if (col < cols) unsafeAtomicAdd(row + col, v[i]);      // (global_atomic_add_f32, nothing returned)
  }
}

__global__ __launch_bounds__(256) void segsum_gather_kernel(const bf16_t* __restrict__ dZ, long ld, int BT, int cols, int n_slabs, int share,
                                                            const int* __restrict__ order, const unsigned* __restrict__ skey, int V,
                                                            int R, float* __restrict__ dEK, float* __restrict__ dCtxK) {
  __shared__ __attribute__((aligned(16))) float strips[4][SEG_SLAB];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const unsigned unit = blockIdx.x * 4u + (unsigned)wave;
  const int slab = (int)(unit % (unsigned)n_slabs);
  const long p0 = (long)(unit / (unsigned)n_slabs) * share;
  if (p0 >= BT) return;
  const long p1 = p0 + share < BT ? p0 + share : BT;
  float* strip = strips[wave];
  const int col_base = slab * SEG_SLAB, col0 = col_base + lane * 8;
  const bool act = col0 < cols;      // (cols is a multiple of 8: a lane's columns are all inside or all outside)
  const bf16_t* src = dZ + (act ? col0 : col_base);

  // eight rows' loads go out together; the waves sharing a SIMD (six at this register count) cover each other's waits
  // (positions past the share's end repeat its last row and are skipped below; lanes beyond the last column read the
  //  slab's first columns and never flush)
  uint4 a[SEG_UNROLL];
  unsigned ka[SEG_UNROLL];
  auto fetch = [&](long p) {
#pragma unroll
    for (int j = 0; j < SEG_UNROLL; ++j) {
      const long q = p + j < p1 ? p + j : p1 - 1;
      const unsigned r = (unsigned)order[q];
      ka[j] = skey[q];
      // (read once: streamed past the caches' keep lists)
      const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + (size_t)r * (size_t)ld));
      a[j] = uint4{t.x, t.y, t.z, t.w};
    }
  };

  float run[8], chr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) run[i] = chr[i] = 0.f;
  unsigned cur = skey[p0];
  // the run ends: its sum goes to the context table and into the character's sum, which leaves when the character changes
  auto close_run = [&](unsigned next, bool last) {
    const unsigned c = cur & 0xffffu, v = cur >> 16;
    if (c < (unsigned)R) seg_flush(strip, run, dCtxK + (size_t)c * cols, col_base, cols);
#pragma unroll
    for (int i = 0; i < 8; ++i) { chr[i] += run[i]; run[i] = 0.f; }
    if (last || (next >> 16) != v) {
      if (v < (unsigned)V) seg_flush(strip, chr, dEK + (size_t)v * cols, col_base, cols);
#pragma unroll
      for (int i = 0; i < 8; ++i) chr[i] = 0.f;
    }
    cur = next;
  };

  for (long p = p0; p < p1; p += SEG_UNROLL) {
    fetch(p);
#pragma unroll
    for (int j = 0; j < SEG_UNROLL; ++j) {
      if (p + j < p1) {
        if (ka[j] != cur) close_run(ka[j], false);
        seg_add_row(run, a[j]);
      }
    }
  }
  close_run(cur, true);
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : KL_ERR_LAUNCH; }

}  // namespace

int kl_segment_sums_buckets(int n_ctx, int V, int R) { return (V + 1) * ((n_ctx > 0 ? R : 0) + 1); }

int kl_segment_sums_share(long BT) {
  // an equal share of the sorted rows per wave and column slab: 256 rows at the training shapes, fewer where that would
  // leave compute units without work (a multiple of the unroll, so that only the last share has a ragged group)
  long s = (BT + 2047) / 2048;
  s = (s + SEG_UNROLL - 1) / SEG_UNROLL * SEG_UNROLL;
  return (int)(s > 256 ? 256 : s);
}

size_t kl_segment_sums_ws_bytes(int B, int T, int n_ctx, int V, int R) {
  const long BT = (long)B * T;
  return (size_t)(seg_pad(kl_segment_sums_buckets(n_ctx, V, R) + 1) + 2 * seg_pad(BT)) * sizeof(int);
}

int kl_launch_segment_sums(const bf16_t* dZ, long ld, int B, int T, int cols, const int* idx, const int* ctx, int n_ctx, int V, int R,
                           float* dEK, float* dCtxK, void* ws, hipStream_t stream) {
  const long BT = (long)B * T;
  if (B < 1 || T < 1 || BT > 0x7fffffffL || V < 1 || n_ctx < 0 || (n_ctx > 0 && R < 1)) return KL_ERR_SHAPE;
  if (n_ctx == 0) R = 0;
  if ((cols & 7) || cols < 8 || (ld & 7) || ld < cols) return KL_ERR_SHAPE;
  if ((long)(V + 1) * (R + 1) > KL_SEGSUM_MAX_BUCKETS) return KL_ERR_SHAPE;
  if (!dZ || !idx || !dEK || !ws || (n_ctx > 0 && (!ctx || !dCtxK))) return KL_ERR_ARG;
  if (((size_t)dZ & 15) || ((size_t)dEK & 15) || ((size_t)dCtxK & 15) || ((size_t)ws & 15)) return KL_ERR_ARG;
  const long nbp = seg_pad((long)(V + 1) * (R + 1) + 1);
  int* offs = reinterpret_cast<int*>(ws);
  int* order = offs + nbp;
  unsigned* skey = reinterpret_cast<unsigned*>(order + seg_pad(BT));

  const size_t n_a = (size_t)nbp / 4, n_b = (size_t)V * cols / 4, n_c = (size_t)R * cols / 4;
  size_t g = (n_a + n_b + n_c + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(segsum_init_kernel, dim3((unsigned)g), dim3(256), 0, stream, reinterpret_cast<uint4*>(offs), n_a,
                     reinterpret_cast<uint4*>(dEK), n_b, reinterpret_cast<uint4*>(dCtxK), n_c);
  const unsigned gr = (unsigned)((BT + 255) / 256);
  hipLaunchKernelGGL(segsum_hist_kernel, dim3(gr), dim3(256), 0, stream, idx, ctx, n_ctx, B, T, V, R, offs);
  const int n4 = (int)(nbp / 4), per4 = (n4 + SEG_SCAN_THREADS - 1) / SEG_SCAN_THREADS;      // (per4 <= SEG_SCAN_Q by the bucket cap)
  hipLaunchKernelGGL(segsum_scan_kernel, dim3(1), dim3(SEG_SCAN_THREADS), 0, stream, reinterpret_cast<int4*>(offs), n4, per4);
  hipLaunchKernelGGL(segsum_scatter_kernel, dim3(gr), dim3(256), 0, stream, idx, ctx, n_ctx, B, T, V, R, offs, order, skey);
  const int n_slabs = (cols + SEG_SLAB - 1) / SEG_SLAB, share = kl_segment_sums_share(BT);
  const long units = (BT + share - 1) / share * n_slabs;
  hipLaunchKernelGGL(segsum_gather_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, stream, dZ, ld, (int)BT, cols, n_slabs, share,
                     order, skey, V, R, dEK, dCtxK);
  return ok();
}
