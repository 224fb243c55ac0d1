// C-ABI orchestration of the Rater hot path on gfx950 (see include/keraslm_hip.h).
//
// The library owns no device memory: parameters, gradients, optimizer moments,
// state rows and workspaces all belong to the caller.  This file lays out the
// workspaces, derives the bf16 operand copies, and issues the launch sequences:
//
//   forward   P1 = table gather (layer-0 input contraction as look-ups) ->
//             layer wavefront of thin fused cell steps (one launch per diagonal:
//             layer l runs time d-l) -> tied-embedding logits -> softmax/CE
//   backward  dH = dlogits.E -> reverse layer wavefront of fused backward cell
//             steps -> weight gradients as big K=B*T GEMMs over transposed
//             activations -> layer-0/embedding gradients through one-hot^T
//             segment sums -> regularisers
//   step      L launches + logits + softmax for n hypotheses with pool slots
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <functional>
#include <utility>

#include <vector>

#include "kl_common.h"
#include "kl_kernels.h"
#include "kl_state_dist.h"

namespace {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int round_up_i(int x, int a) { return (x + a - 1) / a * a; }

// bump allocator; with base == nullptr it only measures
struct Carver {
  unsigned char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(reinterpret_cast<unsigned char*>(b)) {}
  template <typename T>
  T* take(size_t count) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

constexpr int KL_SCAN_FLAGS = 256 * 64;
struct Derived {
  std::vector<bf16_t*> UT_hi, UT_lo, KT_hi, KT_lo, Un, Kn;   // per layer (KT/Kn of layer 0 = rows [0,W) of K0)
  bf16_t *E_hi = nullptr, *E_lo = nullptr, *ET = nullptr;
  std::vector<bf16_t*> WTcat;    // [4W][3*K_l] = [hi | hi | lo] blocks, K_0 = W (U), K_l = 2W (K then U): big-n step path
  std::vector<bf16_t*> UF, KF;   // per layer: U^T / K^T fragment-major (hi and lo planes per 16 x 32 block), step_tile.hip / step_small.hip (W % 32 == 0)
  bf16_t* EF = nullptr;          // the embedding likewise
  std::vector<bf16_t*> WTperm;   // WTcat with rows in (unit block of 32, gate, unit) order: fused cell epilogue (W % 32 == 0)
  bf16_t* Ecat = nullptr;        // [Vp][3W]
  float* EK = nullptr;
  std::vector<float*> CtxK;
  // gate-interleaved copies for the second-generation wide scans (lstm_scan2.hip): column / row u*4+g <- g*W+u
  std::vector<bf16_t*> KTp;      // [4W][W], l >= 1
  std::vector<float*> bp;        // [4W], l >= 1 (layer 0's bias is folded into EKp)
  float* EKp = nullptr;          // [V][4W] = EK + b_0
  bf16_t* comb = nullptr;        // width 512, one context variable: [V * ctx_vocab][W][4] bf16 = EKp[v] + CtxKp_0[c], every gate-input row layer 0 can
                                 // ask for (200 MiB at V = 256) -- the eight-wave forward scan gathers its rows from it (lstm_scan_fwd8.hip, table mode)
  std::vector<float*> CtxKp;     // [ctx_vocab][W][4] per context variable (the scan's table mode reads that of variable 0)
  unsigned* scan_flags = nullptr;   // lstm_scan_bwd_wide2_kernel's flags + epoch (zeroed once per bind: the numbers only grow)
};

struct WindowWs {
  float* P1;
  std::vector<void*> H;        // [(T+1)B][W]  f32 (inference) or bf16 (training)
  std::vector<float*> C;       // [(T+1)B][W]
  float* logits;               // [BT][V]
  float* rowstat;              // [BT][2] per-row (loss, hit)
  int *s_idx, *s_ctx, *s_tgt;  // staged inputs (fixed addresses for graph replay)
  int* ids_tm = nullptr;       // training: [T+1][B][2] table-row byte offsets, time-major (second-generation wide scans)
  int scan2_rows = 0;          // second-generation wide scans planned for this window: rows per forward phase (0: first generation)
  bool scan2_bwd = false;      // ... and the backward scan reads gate-interleaved G
  float *s_masks, *s_probs;
  unsigned *scan_cnt, *scan_status;   // persistent-scan hand-off counters [L][ceil(B/16)][T], status words [2]
  float* reg_scratch;                 // statistics of the embedding regularisers
  // training only
  std::vector<bf16_t*> G, dZ, Hd;
  std::vector<bf16_t*> Cb;            // second-generation wide scans: cell states for the backward scan as bf16 [(T+1)B][W]
  std::vector<bf16_t*> Xhi, Xlo;      // inference: state planes exchanged by the split-precision scan [(T+1)B][W]
  std::vector<bf16_t*> HTf, HdT;      // transposed outputs written by the wide forward scans: [W][(T+1)B], [W][BT]
  bool ht_ready = false;              // ... valid for this window
  bool km_plan = false;               // the weight-gradient GEMMs will read dZ and the activations K-major (row-major as written): no transposed copies
  unsigned p_bf16_mask = 0;           // bit l: layer l's scan took its gate inputs as bf16 rows (noted for kl_test_window_view)
  bf16_t *dZT, *HT, *dlogits, *dlogitsT, *OHT, *dEKT_bf, *dEK_bf;
  std::vector<bf16_t*> OHC;
  bool segsum = false;                // layer 0's character / first-context sums by sorted segment sums (kl_segsum_applicable): dEKT and
                                      // dCtxKT[0] then hold the ROW-major tables [Vp][4W], [ctx_vocab][4W]; OHT and OHC[0] are not carved
  void* seg_ws = nullptr;             // ... the sort's counters, row order and sorted keys (kl_segment_sums_ws_bytes)
  float *dH, *dEKT;
  std::vector<float*> dc0, dc1, dCtxKT;
};

}  // namespace

struct kl_handle {
  kl_config cfg;
  int Vp;                       // voc_size rounded up to 32
  size_t n_params;
  std::vector<size_t> off_K, off_U, off_b, off_Ctx;
  size_t off_E;
  float* params = nullptr;
  void* derived_ws = nullptr;
  size_t derived_bytes = 0;
  Derived d;
  int precision = 0;            // 0 = not prepared
  // hipGraph cache of whole-window launch sequences (keyed by every baked-in pointer)
  struct GraphKey {
    int kind, B, T, flags, precision;
    const void *states, *loss_acc, *ws, *grads;
    int layout = 0;               // workspace layout the body was captured with (kl_forward_window picks it from ws_bytes)
    bool operator==(const GraphKey& o) const {
      return kind == o.kind && B == o.B && T == o.T && flags == o.flags && precision == o.precision &&
             states == o.states && loss_acc == o.loss_acc && ws == o.ws && grads == o.grads && layout == o.layout;
    }
  };
  std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;
  bool graphs_enabled = true;
  bool scan_enabled = true;     // persistent scans (KL_SCAN=0 forces the launch-per-step path)
  bool seq_bwd = true;          // layer-sequential backward scans for many row blocks (KL_SEQ_BWD=0: always fused)
  bool wide_bwd = true;         // ... with 64-unit workgroups (KL_WIDE_BWD=0: thin workgroups)
  void* host_step_ready = nullptr;      // kl_step_batch_host: the workspace whose ticket counter has been zeroed
  std::vector<int32_t> host_pack;       // ... its packed index block for the copy to the device (n > 256, fall-backs)
  bool host_kernarg = true;             // ... indices in the kernel arguments (KL_HOST_KERNARG=0: always the copy)
  void* walk_ready = nullptr;           // kl_walk_batch_host: the workspace whose ticket counter has been zeroed
  bool inc_ready = false;       // the incremental step's fragment-major operands match the current weights (prepare_incremental)
  bool big_ready = false;       // ... and those of the gather + GEMM path (prepare_big_step)
  bool il_ready = false;        // the gate-interleaved set was written by the last prepare_impl (kl_test_derived_view)
  bool comb_ready = false;      // ... and the table of all sums built from it since (build_comb: for kl_test_derived_view only -- a replayed window rebuilds it unnoted)
  int last_only = 0;            // stateless windows: one target per row, at the last position (kl_set_window_mode)
  int loss_rows = 0;            // rows the training means are taken over when the batch carries dummy streams (kl_set_loss_rows; 0: B)
  bool sentinel = true;         // wide scans hand off by data sentinels instead of counters (KL_SENTINEL=0: counters)
  bool gemm_an = true;          // weight gradients read the backward scan's dZ K-major, no transposed copy (KL_GEMM_AN=0: dZ^T)
  bool xcd_local = false;       // KL_XCD_LOCAL=1: sentinel hand-off inside one XCD through its L2 (plain stores) where the placement allows
  bool sentinel_bwd = true;     // sentinel hand-off for the wide backward scan too (KL_SENTINEL_BWD=0, or KL_SENTINEL=0: counters)
  bool sentinel_roll = true;    // KL_SENTINEL_ROLL=0: pre-fill all of dZ instead of re-arming two steps ahead inside the scan
  bool sentinel_bwd_all = false; // KL_SENTINEL_BWD=2: also with one row block per workgroup
  bool xcd_local_bwd = false;    // KL_XCD_LOCAL_BWD=1 (with KL_XCD_LOCAL=1): XCD-local publishes for the wide backward scan too
  bool w32 = true;              // width 1024: the eight-wave scans of lstm_scan_w32.hip (KL_W32=0: the thin scans)
  bool w32_local = false;       // KL_W32_LOCAL=1: ... handing over through the XCD's own L2 where the placement allows (measured slower: 112 vs 104 ms per cfg5 step)
  int w32_min_rb = 8;           // ... from this many row blocks of 16 streams (KL_W32_MIN_RB)
  bool split8 = true;           // width-1024 rating windows with up to 32 streams: two layers per launch, eight units per workgroup (KL_SPLIT8=0: layer by layer)
  bool split_sentinel = true;   // rating windows: the split-precision scan hands over by data sentinels (KL_SPLIT_SENTINEL=0: counters)
  bool inc_small = true;        // incremental step: step_small.hip's kernels (KL_INC_SMALL=0: the launch-per-layer thin kernels + thin GEMM + softmax)
  bool fused_step = true;       // incremental step, n >= 256: cell fused into the GEMM epilogue (KL_FUSED_STEP=0: separate kernels)
  bool inc_tile = true;         // incremental step, n >= 256: step_tile.hip's one launch per layer (KL_INC_TILE=0: gather + [hi|lo|hi] GEMM)
  int tile_var = 0;             // KL_TILE_VAR: timing variants of inc_tile_kernel (never in production)
  int tile_rows = -1;           // KL_TILE_ROWS=64|128: rows per tile of inc_tile_kernel (default: by size)
  bool out_fused = true;        // incremental step: logits + softmax in one launch (KL_OUT_FUSED=0: thin GEMM + softmax kernel)
  int out_fused_min = 512;      // ... from this many hypotheses on (KL_OUT_FUSED_MIN; width 512: 128 rows 25.7 us per step against 24.2, 256 rows 35.8 / 35.1, 1024 rows 41.3 / 43.5)
  int inc_small_min = KL_SMALL_STEP_N;      // step_small.hip's kernel from this many hypotheses on (KL_INC_SMALL_MIN)
  bool scan2 = true;            // second-generation wide scans where their grid plan applies (KL_SCAN2=0: first generation)
  int scan2_rows = 0;           // KL_SCAN2_ROWS = 16 / 32: rows per forward phase (0: chosen by shape)
  int scan2_pf = -1;            // KL_SCAN2_PF: where the forward scan requests its next tile (0: top of a phase, 1: behind the MFMA phase, 2: two phases ahead; -1: by shape)
  bool scan2_bf16 = true;       // KL_SCAN2_BF16=0: f32 instead of bf16 for what the scans exchange with later kernels (P, dH, c for backward)
  bool logits_ws = true;        // KL_LOGITS_WS = 0: GEMM + softmax kernel for the training window's output layer instead of the fused kernel
  bool proj_ws = true;          // KL_PROJ_WS = 0: the ring GEMM for the gate inputs P of the second-generation scans too
  bool w128 = true;             // KL_W128 = 0: the thin fused scans also at width 128 (lstm_scan_w128.hip: a workgroup per 16-row block, all units)
  bool w128_tables = true;      // KL_W128_TABLES = 0: layer 0's gate inputs gathered into f32 rows first instead of inside the scan
  bool w128_multi = true;       // KL_W128_MULTI = 0: one launch per layer also where all layers' workgroups fit the CUs at once
  bool w128_fuse = true;        // KL_W128_FUSE = 0: ... with the input side of the layers above the first from products over all steps
  int w128_min = 1;             // ... from this many streams on (KL_W128_MIN; measured against the thin fused scans, ms per step at 1 / 16 / 64 / 128 / 256 streams:
                                // 1.54 / 1.68 / 1.69 / 1.74 / 1.87 against 1.57 / 1.80 / 1.79 / 1.96 / 2.29)
  bool fwd8 = true;             // KL_FWD8 = 0: the 16-wave forward scan also for the layers above the first (default: the eight-wave scan of
                                // lstm_scan_fwd8.hip there -- 3.06 against 3.36 ms per launch at 3072 streams)
  bool fwd8_all = false;        // KL_FWD8 = 2: ... also for layer 0 (its gate inputs gathered into P rows first)
  bool fwd8_tab = true;         // KL_FWD8_TAB = 0: layer 0 (one context variable) stays on the 16-wave scan's table mode (default: the eight-wave scan,
                                // its gate-input rows gathered from the table of all (character, context value) sums -- 200 MiB more of derived operands;
                                // 23.03 / 23.20 against 23.21 / 23.28 ms per step with 200 context values in the batch, where its gathers leave the L2)
  bool fwd8_ls = true;          // KL_FWD8_LS = 0: the counter form of the eight-wave forward scan instead of the two-barrier form
  bool fwd8_local = true;       // KL_FWD8_LOCAL = 0: write-through publishes in the eight-wave forward scan even where its partners share an XCD
  int fwd8_pf = -1;             // KL_FWD8_PF = 0..3: where it requests its tiles (default by phases per step)
  bool rt_local = true;         // KL_RT_LOCAL = 0: write-through publishes in the register-tile backward scan even where its partners share an XCD
  bool regtile = true;          // KL_REGTILE = 0: the backward scan's tiles by LDS-DMA at every size (else through registers from five blocks per step)
  bool scan2_flags = true;      // KL_SCAN2_FLAGS = 0: the backward scan hands over by data sentinels at every size (else by flags from three blocks per step)
  bool flags_zeroed = false;
  // what kl_test_window_view reports: noted by train_window_body per (B, T, workspace) while it builds the launch sequence (a
  // replayed graph does not run the body again, and windows of other shapes may have run in between)
  struct ViewNote {
    int B, T;
    const void* ws;
    int scan2_rows, g_interleaved, c_in_cb, dh_bf16;
    unsigned p_bf16_mask;
    // the weight-gradient stage (filled in once the stage's launches are built): KL_WG_* bits, dU / dK pairs and scan-summed
    // db per layer, layers whose masked outputs Hd were written
    unsigned wg_route = 0, wg_pair_mask = 0, wg_db_scan_mask = 0, hd_mask = 0;
    unsigned out_route = 0;      // the output layer in front of them: KL_OUT_* bits
  };
  std::vector<ViewNote> view_notes;
  // the note of (B, T, ws); insert: a new one where there is none (the 64 most recent are kept), else null
  ViewNote* view_note(int B, int T, const void* ws, bool insert) {
    for (auto& n : view_notes)
      if (n.B == B && n.T == T && n.ws == ws) return &n;
    if (!insert) return nullptr;
    if (view_notes.size() >= 64) view_notes.erase(view_notes.begin());
    view_notes.push_back(ViewNote{B, T, ws, 0, 0, 0, 0, 0u});
    return &view_notes.back();
  }
  // what kl_test_forward_view reports: noted by the scan families of forward_impl per (B, T, workspace, precision) of an
  // inference-layout window while they build its launch sequence (as ViewNote: a replayed graph does not run them again)
  struct ForwardNote {
    int B, T;
    const void* ws;
    int precision;
    int family = 0, passed_mask = 0, handoff = 0, c_every_step = 0, planes = 0, p1_layer = -1;
    unsigned ring_mask = 0, thin_mask = 0;
  };
  std::vector<ForwardNote> forward_notes;
  // the note of (B, T, ws) in the handle's current precision; insert: a new one where there is none (the 64 most recent are kept), else null
  ForwardNote* forward_note(int B, int T, const void* ws, bool insert) {
    for (auto& n : forward_notes)
      if (n.B == B && n.T == T && n.ws == ws && n.precision == precision) return &n;
    if (!insert) return nullptr;
    if (forward_notes.size() >= 64) forward_notes.erase(forward_notes.begin());
    forward_notes.push_back(ForwardNote{B, T, ws, precision});
    return &forward_notes.back();
  }
  bool segsum = true;           // KL_SEGSUM = 0: layer 0's table gradients as one-hot products (default: sorted segment sums, segsum.hip -- read in
                                // kl_create, it decides the window workspace's size)
  bool fuse_wg = true;          // KL_FUSE_WG = 0: one launch per weight-gradient product (else products over the same dZ share a pass)
  int scan2_pfb = -1;           // KL_SCAN2_PFB: the same for the backward scan (-1: by shape)
  int wide_fwd_min = 96;        // layer-sequential wide forward scans from this many 64-unit workgroups (KL_WIDE_FWD_MIN; 0 = never)
  double trace_flops[2] = {0.0, 0.0};   // algorithmic FLOPs of ONE timed launch
  // optional per-launch timing of the cell-step kernels with HIP events (bench.py's
  // roofline leg).  While tracing, windows run eagerly (events are not captured).
  bool trace_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> trace_ev[2];   // [0] forward steps, [1] backward steps
  size_t trace_used[2] = {0, 0};
  bool trace_open[2] = {false, false};
  bool trace_persistent[2] = {false, false};   // the timed launches were whole-window persistent scans
  const char* trace_name[2] = {"lstm_fwd_step_kernel", "lstm_bwd_step_kernel"};   // kernel the timed launches ran
  void trace_begin(int kind, hipStream_t s) {
    if (!trace_on) return;
    if (trace_used[kind] == trace_ev[kind].size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { trace_on = false; return; }
      trace_ev[kind].emplace_back(a, b);
    }
    (void)hipEventRecord(trace_ev[kind][trace_used[kind]].first, s);
    trace_open[kind] = true;
  }
  void trace_end(int kind, hipStream_t s) {
    if (!trace_on || !trace_open[kind]) return;
    trace_open[kind] = false;
    (void)hipEventRecord(trace_ev[kind][trace_used[kind]].second, s);
    ++trace_used[kind];
  }
  void drop_graphs() {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
    graphs.clear();
  }
};

namespace {

void layout(kl_handle* h) {
  const kl_config& c = h->cfg;
  const size_t W = c.width;
  size_t off = 0;
  h->off_E = off;
  off += (size_t)c.voc_size * W;
  h->off_Ctx.clear();
  for (int n = 0; n < c.n_ctx; ++n) {
    h->off_Ctx.push_back(off);
    off += (size_t)c.ctx_vocab * c.ctx_dim;
  }
  h->off_K.clear();
  h->off_U.clear();
  h->off_b.clear();
  for (int l = 0; l < c.depth; ++l) {
    const size_t D = l == 0 ? W + (size_t)c.ctx_dim * c.n_ctx : W;
    h->off_K.push_back(off);
    off += D * 4 * W;
    h->off_U.push_back(off);
    off += W * 4 * W;
    h->off_b.push_back(off);
    off += 4 * W;
  }
  h->n_params = off;
  h->Vp = round_up_i(c.voc_size, 32);
}

bool config_ok(const kl_config* c) {
  if (!c) return false;
  if (c->depth < 1 || c->depth > 16) return false;
  if (c->width < 32 || (c->width & 31)) return false;
  if (c->voc_size < 1) return false;
  if (c->n_ctx < 0 || c->n_ctx > 8) return false;
  if (c->ctx_vocab < 2 || c->ctx_dim < 1) return false;
  return true;
}

size_t carve_derived(const kl_handle* h, void* base, Derived* d) {
  const kl_config& c = h->cfg;
  const size_t W = c.width, V = c.voc_size, Vp = h->Vp;
  Carver cv(base);
  Derived tmp;
  Derived& o = d ? *d : tmp;
  o.UT_hi.assign(c.depth, nullptr); o.UT_lo.assign(c.depth, nullptr);
  o.KT_hi.assign(c.depth, nullptr); o.KT_lo.assign(c.depth, nullptr);
  o.Un.assign(c.depth, nullptr); o.Kn.assign(c.depth, nullptr);
  for (int l = 0; l < c.depth; ++l) {
    o.UT_hi[l] = cv.take<bf16_t>(4 * W * W);
    o.UT_lo[l] = cv.take<bf16_t>(4 * W * W);
    o.KT_hi[l] = cv.take<bf16_t>(4 * W * W);
    o.KT_lo[l] = cv.take<bf16_t>(4 * W * W);
    o.Un[l] = cv.take<bf16_t>(4 * W * W);
    o.Kn[l] = cv.take<bf16_t>(4 * W * W);
  }
  o.E_hi = cv.take<bf16_t>(Vp * W);
  o.E_lo = cv.take<bf16_t>(Vp * W);
  o.ET = cv.take<bf16_t>(W * Vp);
  o.EK = cv.take<float>(V * 4 * W);
  o.WTcat.assign(c.depth, nullptr);
  for (int l = 0; l < c.depth; ++l) o.WTcat[l] = cv.take<bf16_t>(4 * W * 3 * (l == 0 ? W : 2 * W));
  o.WTperm.assign(c.depth, nullptr);
  if ((W & 31) == 0)
    for (int l = 0; l < c.depth; ++l) o.WTperm[l] = cv.take<bf16_t>(4 * W * 3 * (l == 0 ? W : 2 * W));
  o.Ecat = cv.take<bf16_t>(Vp * 3 * W);
  o.UF.assign(c.depth, nullptr);
  o.KF.assign(c.depth, nullptr);
  if ((W & 31) == 0) {
    for (int l = 0; l < c.depth; ++l) {
      o.UF[l] = cv.take<bf16_t>(4 * W * W * 2);
      if (l > 0) o.KF[l] = cv.take<bf16_t>(4 * W * W * 2);
    }
    o.EF = cv.take<bf16_t>(Vp * W * 2);
  }
  o.CtxK.assign(c.n_ctx, nullptr);
  for (int n = 0; n < c.n_ctx; ++n) o.CtxK[n] = cv.take<float>((size_t)c.ctx_vocab * 4 * W);
  o.KTp.assign(c.depth, nullptr);
  o.bp.assign(c.depth, nullptr);
  for (int l = 1; l < c.depth; ++l) {
    o.KTp[l] = cv.take<bf16_t>(4 * W * W);
    o.bp[l] = cv.take<float>(4 * W);
  }
  o.EKp = cv.take<float>(V * 4 * W);
  o.CtxKp.assign(c.n_ctx, nullptr);
  for (int n = 0; n < c.n_ctx; ++n) o.CtxKp[n] = cv.take<float>((size_t)c.ctx_vocab * 4 * W);
  o.scan_flags = cv.take<unsigned>(KL_SCAN_FLAGS + 64);      // hand-off flags of the backward scan [256 row blocks][64] + the epoch word
  o.comb = nullptr;
  if (h->fwd8_tab && W == 512 && c.n_ctx == 1 && V * (size_t)c.ctx_vocab * 4 * W * sizeof(bf16_t) <= ((size_t)512 << 20))
    o.comb = cv.take<bf16_t>(V * (size_t)c.ctx_vocab * 4 * W);
  return align_up(cv.off, 256);
}

// Layer 0's character and first-context gradient sums as sorted segment sums over dZ_0 (segsum.hip) instead of one-hot
// products?  Asked by carve_window (which arrays exist) and by train_window_body (which launches go out).  The counters of
// all (character, context value) pairs, invalid ones included, must fit the one-workgroup scan: at most
// KL_SEGSUM_MAX_BUCKETS = 65535 of them.  No shape class is excluded beyond that: the pass is one read of dZ_0 at any shape, the
// products it replaces read dZ_0 at least once and the one-hot matrices on top.
bool kl_segsum_applicable(const kl_handle* h, int B, int T) {
  const kl_config& c = h->cfg;
  if (!h->segsum || B < 1 || T < 1 || (long)B * T > 0x7fffffffL) return false;
  return (long)kl_segment_sums_buckets(c.n_ctx, h->Vp, c.ctx_vocab) <= KL_SEGSUM_MAX_BUCKETS;
}

size_t carve_window(const kl_handle* h, void* base, int B, int T, int training, WindowWs* out) {
  const kl_config& c = h->cfg;
  const size_t W = c.width, V = c.voc_size, Vp = h->Vp, L = c.depth;
  const size_t BT = (size_t)B * T, BTp = round_up_i((int)BT, 8);
  Carver cv(base);
  WindowWs tmp;
  WindowWs& o = out ? *out : tmp;
  o.P1 = cv.take<float>(BT * 4 * W);
  o.H.assign(L, nullptr);
  o.C.assign(L, nullptr);
  for (size_t l = 0; l < L; ++l) {
    o.H[l] = training ? (void*)cv.take<bf16_t>((BT + B) * W) : (void*)cv.take<float>((BT + B) * W);
    o.C[l] = cv.take<float>((BT + B) * W);
  }
  o.Xhi.assign(L, nullptr); o.Xlo.assign(L, nullptr);
  if (!training) {
    for (size_t l = 0; l < L; ++l) {
      o.Xhi[l] = cv.take<bf16_t>((BT + B) * W);
      o.Xlo[l] = cv.take<bf16_t>((BT + B) * W);
    }
  }
  o.logits = cv.take<float>(BT * V);
  o.rowstat = cv.take<float>(BT * 2);
  o.s_idx = cv.take<int>(BT);
  o.s_ctx = cv.take<int>(BT * (size_t)(c.n_ctx > 0 ? c.n_ctx : 1));
  o.s_tgt = cv.take<int>(BT);
  o.s_masks = cv.take<float>(training ? L * (size_t)B * W : 1);
  o.s_probs = cv.take<float>(BT * V);      // (training layout too: validation windows run on it, kl_forward_window)
  o.scan_cnt = cv.take<unsigned>(L * ((size_t)(B + 15) / 16) * T);
  o.scan_status = cv.take<unsigned>(4 + 256);   // status words [4] + XCC posts of the wide scans' workgroups [256]
  o.reg_scratch = cv.take<float>(3 * (W > (size_t)c.ctx_dim ? W : (size_t)c.ctx_dim) + (V > (size_t)c.ctx_vocab ? V : (size_t)c.ctx_vocab) + 8);
  if (training) {
    o.G.assign(L, nullptr); o.dZ.assign(L, nullptr); o.Hd.assign(L, nullptr); o.Cb.assign(L, nullptr);
    o.dc0.assign(L, nullptr); o.dc1.assign(L, nullptr);
    for (size_t l = 0; l < L; ++l) {
      o.G[l] = cv.take<bf16_t>(BT * 4 * W);
      o.dZ[l] = cv.take<bf16_t>(BT * 4 * W);
      o.Hd[l] = l > 0 ? cv.take<bf16_t>(BT * W) : nullptr;
      o.Cb[l] = cv.take<bf16_t>((BT + B) * W);
      o.dc0[l] = cv.take<float>((size_t)B * W);
      o.dc1[l] = cv.take<float>((size_t)B * W);
    }
    o.dZT = cv.take<bf16_t>(4 * W * BTp);
    o.HT = cv.take<bf16_t>(W * BTp);
    o.ids_tm = cv.take<int>((BT + B) * 2);
    o.HTf.assign(L, nullptr); o.HdT.assign(L, nullptr);
    if ((B & 7) == 0) {
      for (size_t l = 0; l < L; ++l) {
        o.HTf[l] = cv.take<bf16_t>(W * (BT + B));
        o.HdT[l] = l > 0 ? cv.take<bf16_t>(W * BT) : nullptr;
      }
    }
    o.dlogits = cv.take<bf16_t>(BT * Vp);
    o.dlogitsT = cv.take<bf16_t>(Vp * BTp);
    o.segsum = kl_segsum_applicable(h, B, T);
    o.OHT = o.segsum ? nullptr : cv.take<bf16_t>(Vp * BTp);
    o.seg_ws = o.segsum ? cv.take<char>(kl_segment_sums_ws_bytes(B, T, c.n_ctx, (int)Vp, c.ctx_vocab)) : nullptr;
    o.OHC.assign(c.n_ctx, nullptr);
    o.dCtxKT.assign(c.n_ctx, nullptr);
    for (int n = 0; n < c.n_ctx; ++n) {
      o.OHC[n] = (o.segsum && n == 0) ? nullptr : cv.take<bf16_t>((size_t)c.ctx_vocab * BTp);
      o.dCtxKT[n] = cv.take<float>(4 * W * (size_t)c.ctx_vocab);
    }
    o.dH = cv.take<float>(BT * W);
    o.dEKT = cv.take<float>(4 * W * Vp);
    o.dEKT_bf = cv.take<bf16_t>(4 * W * Vp);
    o.dEK_bf = cv.take<bf16_t>(Vp * 4 * W);
  }
  return align_up(cv.off, 256);
}

#define KL_TRY(expr)            \
  do {                          \
    int _e = (expr);            \
    if (_e != 0) return _e;     \
  } while (0)

int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : KL_ERR_LAUNCH; }

int prepare_impl(kl_handle* h, int precision, hipStream_t s) {
  const kl_config& c = h->cfg;
  const int W = c.width, V = c.voc_size, Vp = h->Vp;
  const float* P = h->params;
  Derived& d = h->d;
  const bool split = precision == KL_PREC_SPLIT;
  if (!h->flags_zeroed) {      // once per bind, and not inside a capture (a replay must not turn the epoch back)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
      KL_TRY(kl_zero_async(d.scan_flags, (size_t)(KL_SCAN_FLAGS + 64) * sizeof(unsigned), s));
      h->flags_zeroed = true;
    }
  }
  // every bf16 operand derived from the parameters, in as few launches as the job list takes (a training step comes here after
  // every Adam update): per layer U^T, K^T (hi [+ lo]) and U, K as they are; the embedding E (rows beyond the vocabulary: zeros)
  // and E^T
  const float* E = P + h->off_E;
  {
    KlConvJob jobs[KL_CONV_MAX_JOBS];
    int nj = 0;
    auto add = [&](const float* in, long ld_in, int rows, int cols, int rows_pad, bf16_t* hi, bf16_t* lo, long ld_out, int tr) -> int {
      jobs[nj++] = KlConvJob{in, ld_in, rows, cols, rows_pad, tr, hi, lo, ld_out};
      if (nj < KL_CONV_MAX_JOBS) return 0;
      nj = 0;
      return kl_launch_f32_to_bf16_jobs(jobs, KL_CONV_MAX_JOBS, s);
    };
    for (int l = 0; l < c.depth; ++l) {
      const float* K = P + h->off_K[l];   // layer 0: rows [0,W) are the char-embedding part
      const float* U = P + h->off_U[l];
      KL_TRY(add(U, 4 * W, W, 4 * W, W, d.UT_hi[l], split ? d.UT_lo[l] : nullptr, W, 1));
      KL_TRY(add(K, 4 * W, W, 4 * W, W, d.KT_hi[l], split ? d.KT_lo[l] : nullptr, W, 1));
      KL_TRY(add(U, 4 * W, W, 4 * W, W, d.Un[l], nullptr, 4 * W, 0));
      KL_TRY(add(K, 4 * W, W, 4 * W, W, d.Kn[l], nullptr, 4 * W, 0));
    }
    KL_TRY(add(E, W, V, W, Vp, d.E_hi, split ? d.E_lo : nullptr, W, 0));
    KL_TRY(add(E, W, V, W, Vp, d.ET, nullptr, Vp, 1));
    if (nj > 0) KL_TRY(kl_launch_f32_to_bf16_jobs(jobs, nj, s));
  }
  // layer-0 look-up tables: EK = E . K0[:W] ; CtxK_n = Ctx_n . K0[W+10n ..]
  KlOperand op;
  memset(&op, 0, sizeof(op));
  op.A = E; op.lda = W; op.a_is_f32 = 1;
  op.WT_hi = d.KT_hi[0]; op.WT_lo = split ? d.KT_lo[0] : nullptr; op.ldw = W; op.K = W;
  KL_TRY(kl_launch_thin_gemm(&op, V, 4 * W, d.EK, 4 * W, nullptr, precision, s));
  for (int n = 0; n < c.n_ctx; ++n) {
    const float* Kc = P + h->off_K[0] + (size_t)(W + n * c.ctx_dim) * 4 * W;
    KL_TRY(kl_launch_small_table(P + h->off_Ctx[n], c.ctx_vocab, c.ctx_dim, Kc, 4 * W, 4 * W, d.CtxK[n], 4 * W, s));
  }
  h->il_ready = precision == KL_PREC_BF16 && h->scan2 && W == 512;
  h->comb_ready = false;
  if (h->il_ready) {
    // gate-interleaved copies for the second-generation wide scans
    for (int l = 1; l < c.depth; ++l) {
      KL_TRY(kl_launch_permute_gate_rows_bf16(d.KT_hi[l], d.KTp[l], W, W, s));
      KL_TRY(kl_launch_permute_gate_cols_f32(P + h->off_b[l], nullptr, d.bp[l], 1, W, s));
    }
    KL_TRY(kl_launch_permute_gate_cols_f32(d.EK, P + h->off_b[0], d.EKp, V, W, s));
    for (int n = 0; n < c.n_ctx; ++n) KL_TRY(kl_launch_permute_gate_cols_f32(d.CtxK[n], nullptr, d.CtxKp[n], c.ctx_vocab, W, s));
  }
  h->precision = precision;
  h->inc_ready = false;      // the incremental step's own operands are rebuilt on their first use (prepare_incremental,
  h->big_ready = false;      // prepare_big_step)
  return 0;
}

// Operands only the incremental step reads.  Built lazily: a training step re-derives the window operands after every
// Adam update and never touches these.
// (1) fragment-major copies of the [4W][W] / [Vp][W] hi / lo arrays kl_prepare keeps (step_small.hip, step_tile.hip)
int prepare_incremental(kl_handle* h, hipStream_t s) {
  const kl_config& c = h->cfg;
  const int W = c.width, Vp = h->Vp;
  Derived& d = h->d;
  const bool split = h->precision == KL_PREC_SPLIT;
  if (d.EF) {
    for (int l = 0; l < c.depth; ++l) {
      KL_TRY(kl_launch_frag_major(d.UT_hi[l], split ? d.UT_lo[l] : nullptr, 4 * W, W, W, d.UF[l], s));
      if (l > 0) KL_TRY(kl_launch_frag_major(d.KT_hi[l], split ? d.KT_lo[l] : nullptr, 4 * W, W, W, d.KF[l], s));
    }
    KL_TRY(kl_launch_frag_major(d.E_hi, split ? d.E_lo : nullptr, Vp, W, W, d.EF, s));
  }
  h->inc_ready = true;
  return 0;
}

// (2) the gather + GEMM path (widths beyond 1024 that are not multiples of 256; vocabularies from 1024 characters on):
// concatenated [hi | hi | lo] weights, their gate-permuted copies and the concatenated embedding
int prepare_big_step(kl_handle* h, hipStream_t s) {
  const kl_config& c = h->cfg;
  const int W = c.width, V = c.voc_size, Vp = h->Vp;
  const float* P = h->params;
  Derived& d = h->d;
  const bool split = h->precision == KL_PREC_SPLIT;
  const float* E = P + h->off_E;
  for (int l = 0; l < c.depth; ++l) {
    const int Kl = l == 0 ? W : 2 * W;
    const long ld = 3L * Kl;
    const float* K = P + h->off_K[l];
    const float* U = P + h->off_U[l];
    bf16_t* base = d.WTcat[l];
    const int uoff = l == 0 ? 0 : W;     // U part follows the K part inside each block
    if (l > 0) {
      KL_TRY(kl_launch_f32_to_bf16_t(K, 4 * W, W, 4 * W, base, split ? base + 2 * Kl : nullptr, ld, 1, s));
      if (split) KL_TRY(kl_launch_f32_to_bf16_t(K, 4 * W, W, 4 * W, base + Kl, nullptr, ld, 1, s));
    }
    KL_TRY(kl_launch_f32_to_bf16_t(U, 4 * W, W, 4 * W, base + uoff, split ? base + 2 * Kl + uoff : nullptr, ld, 1, s));
    if (split) KL_TRY(kl_launch_f32_to_bf16_t(U, 4 * W, W, 4 * W, base + Kl + uoff, nullptr, ld, 1, s));
    if (d.WTperm[l]) KL_TRY(kl_launch_permute_gate_rows(base, d.WTperm[l], W, ld, s));
  }
  KL_TRY(kl_zero_async(d.Ecat, (size_t)Vp * 3 * W * sizeof(bf16_t), s));
  KL_TRY(kl_launch_f32_to_bf16_t(E, W, V, W, d.Ecat, split ? d.Ecat + 2 * W : nullptr, 3 * W, 0, s));
  if (split) KL_TRY(kl_launch_f32_to_bf16_t(E, W, V, W, d.Ecat + W, nullptr, 3 * W, 0, s));
  h->big_ready = true;
  return 0;
}

// (3) every gate-input row layer 0 can ask for: 200 MiB, ~0.05 ms -- built by every window that gathers from it (no "already
// built" test: a captured window is replayed after later updates of the operands, and must then build it again)
int build_comb(kl_handle* h, hipStream_t s) {
  const kl_config& c = h->cfg;
  KL_TRY(kl_launch_comb_table(h->d.EKp, h->d.CtxKp[0], c.voc_size, c.ctx_vocab, 4 * c.width, h->d.comb, s));
  h->comb_ready = true;
  return 0;
}

// Second-generation wide scans (lstm_scan2.hip) for this window?  Returns the rows per forward phase (16 / 32) or 0.
// need_bwd: the window is a training window, i.e. the backward scan must be able to read the gate-interleaved G.
int plan_scan2(const kl_handle* h, int B, int T, bool km_plan, bool need_bwd) {
  const kl_config& c = h->cfg;
  const int W = c.width;
  if (!h->scan2 || !h->scan_enabled || !h->sentinel || !km_plan || T < 3) return 0;
  if (c.n_ctx > 1 && !h->scan2_bf16) return 0;      // (several context variables: layer 0's gate inputs as bf16 P rows, kl_launch_p_gather_il)
  if (W != 512) return 0;      // (one tile row = one 1 KiB DMA piece)
  if (h->wide_fwd_min <= 0 || !kl_scan_fwd_wide_applicable(B, T, W) || ((B + 15) / 16) * (W / 64) < h->wide_fwd_min) return 0;
  if (need_bwd && (!h->wide_bwd || !h->seq_bwd || !h->sentinel_bwd || !h->sentinel_roll || !kl_scan_wide2_phases(B, T, W, 16, 6))) return 0;
  const int p16 = kl_scan_wide2_phases(B, T, W, 16, 5), p32 = kl_scan_wide2_phases(B, T, W, 32, 4);
  if (h->scan2_rows == 16) return p16 ? 16 : 0;
  if (h->scan2_rows == 32) return p32 ? 32 : 0;
  // (by shape, measured at B = 1024 .. 3072: 32-row phases as soon as a workgroup has two of them per step)
  if (p32 >= 2) return 32;
  if (p16) return 16;
  return p32 ? 32 : 0;
}

// ---- the forward half of a window: kl_train_window, kl_rate_window and its kin, kl_forward_window in both layouts ----
struct FwdCall {       // a forward pass over one window as its scan families see it
  kl_handle* h; int B, T; const int *idx, *ctx; float* states; const float* masks; int training, split; WindowWs& w; hipStream_t s;
  int W, L; size_t BW; int n_rb;      // n_rb: row blocks of 16 streams
  kl_handle::ForwardNote* note;       // inference layout: what kl_test_forward_view will say about this window (training layout: null)
};
// a family of the inference layout hands the window on after it has issued launches / has finished it
static void note_passed(const FwdCall& c, int family) { if (c.note) c.note->passed_mask |= family; }
static void note_finished(const FwdCall& c, int family, int handoff, int planes, int c_every_step, int p1_layer) {
  if (!c.note) return;
  c.note->family = family; c.note->handoff = handoff; c.note->planes = planes; c.note->c_every_step = c_every_step; c.note->p1_layer = p1_layer;
}
// a scan family's "not mine" (no public return code -- those are 0 .. 5, keraslm_hip.h)
constexpr int FWD_PASS = -1;
static_assert(FWD_PASS < KL_OK, "FWD_PASS must not be a public return code");

// row block `block` of layer l's H (0: the carried-in state, t + 1: what step t leaves), bf16 in the training layout, else f32
static const void* h_rows(const FwdCall& c, int l, int block) {
  return c.training ? (const void*)((bf16_t*)c.w.H[l] + (size_t)block * c.BW) : (const void*)((float*)c.w.H[l] + (size_t)block * c.BW);
}
// training layout: the bf16 rows layer l > 0 reads at steps 0 .. T-1 -- the outputs of layer l - 1, masked where that layer drops out
static const bf16_t* layer_in(const FwdCall& c, int l) {
  return (c.masks != nullptr && l - 1 > 0) ? c.w.Hd[l - 1] : (const bf16_t*)c.w.H[l - 1] + c.BW;
}
// ... and where layer l writes its own masked outputs, with its mask (both null: no dropout on this layer)
struct LayerMask { bf16_t* Hd; const float* mask; };
static LayerMask layer_mask(const FwdCall& c, int l) {
  if (c.masks == nullptr || l == 0) return {nullptr, nullptr};
  return {c.w.Hd[l], c.masks + (size_t)l * c.BW};
}
// layer 0's gate inputs for all steps, gathered from the look-up tables: P1 = EK[idx] + sum_n CtxK_n[ctx_n] + b_0
static int gather_layer0(const FwdCall& c) {
  const kl_handle* h = c.h; const kl_config& cf = h->cfg;
  std::vector<const float*> ctxk(h->d.CtxK.begin(), h->d.CtxK.end());
  return kl_launch_p1_gather(h->d.EK, ctxk.data(), cf.n_ctx, h->params + h->off_b[0], c.idx, c.ctx, c.B, c.T, 4 * c.W, c.w.P1, c.s);
}
// The gate inputs of layer l > 0 for all steps, one product over layer_in's rows: P1 = X . K_l^T + b_l (p_bf16: as bf16 rows).  il: from the
// gate-interleaved operands of the second-generation scans; ws: ... on the weight-stationary kernel where it takes the shape, else the ring GEMM
static int project_inputs(const FwdCall& c, int l, bool il, bool p_bf16, bool ws) {
  const kl_handle* h = c.h; const Derived& d = h->d; const int W = c.W;
  const bf16_t* X = layer_in(c, l);
  if (ws) {
    const int e = kl_launch_proj_ws(X, d.KTp[l], d.bp[l], reinterpret_cast<bf16_t*>(c.w.P1), (long)c.B * c.T, W, c.w.scan_status, c.s);
    if (e != KL_ERR_SHAPE) return e;
  }
  return kl_launch_gemm_tn(X, il ? d.KTp[l] : d.KT_hi[l], c.w.P1, il ? d.bp[l] : h->params + h->off_b[l], c.B * c.T, 4 * W, W, W, W, 4 * W,
                           p_bf16 ? 1 : 0, 1, 1.f, c.s);
}

enum ArmMode { ARM_ROLLING, ARM_ALL_STEPS, ARM_COUNTERS };      // (arm_publish here, arm_dz in the backward half)
// What a layer's scan hands over from: the row blocks it is going to publish, from `rows` on, as sentinels -- all T steps, or only the
// first two (rolling: the scan arms block t + 3 while it publishes block t + 1) -- or, for a scan that counts, one layer's counters at zero
static int arm_publish(const FwdCall& c, bf16_t* rows, ArmMode mode) {
  if (mode == ARM_COUNTERS) return kl_zero_coherent_async(c.w.scan_cnt, (size_t)c.n_rb * c.T, c.s);
  return kl_fill_u32_async(rows, (size_t)(mode == ARM_ROLLING ? 2 : c.T) * c.BW * sizeof(bf16_t), 0xFFFFFFFFu, c.s);
}
// a whole-window forward scan went out: what the per-launch timing reports about it
static void trace_fwd_scan(const FwdCall& c, const char* kernel, double flops) {
  c.h->trace_persistent[0] = true; c.h->trace_name[0] = kernel; c.h->trace_flops[0] = flops;
  c.h->trace_end(0, c.s);
}
// one layer's recurrent contraction over the window
static double layer_flops(const FwdCall& c) { return (double)c.B * c.T * (2.0 * c.W * 4.0 * c.W); }

// what the wide and the width-128 scans of layer l are told alike (the families add the input side and the hand-off)
static KlScanFwdWide wide_layer_args(const FwdCall& c, int l) {
  const LayerMask m = layer_mask(c, l);
  KlScanFwdWide a;
  memset(&a, 0, sizeof(a));
  a.B = c.B; a.T = c.T; a.W = c.W; a.UT = c.h->d.UT_hi[l];
  a.H = (bf16_t*)c.w.H[l]; a.C = c.w.C[l]; a.G = c.w.G[l];
  a.Hd = m.Hd; a.mask = m.mask; a.status = c.w.scan_status;
  return a;
}
// layer 0 straight from the f32 look-up tables, by the window's own indices (first-generation wide scans, width 128)
static void wide_tables(const FwdCall& c, KlScanFwdWide& a) {
  const kl_handle* h = c.h; const kl_config& cf = h->cfg;
  a.P = nullptr; a.EK = h->d.EK; a.n_ctx = cf.n_ctx; a.idx = c.idx; a.ctx = c.ctx; a.bias = h->params + h->off_b[0];
  for (int n = 0; n < cf.n_ctx; ++n) a.CtxK[n] = h->d.CtxK[n];
}
// the 16-wave wide scans' own table mode for layer 0 (second generation): character row + ONE context row, by time-major row offsets
static int wide2_table_mode(const FwdCall& c, KlScanFwdWide& a) {
  const kl_config& cf = c.h->cfg; const Derived& d = c.h->d;
  KL_TRY(kl_launch_ids_tm(c.idx, c.ctx, cf.n_ctx, c.B, c.T, c.W, cf.voc_size, cf.ctx_vocab, c.w.ids_tm, c.s));
  a.P = nullptr; a.p_bf16 = 0; a.ids_tm = c.w.ids_tm;
  a.EK = d.EKp; a.CtxK[0] = cf.n_ctx > 0 ? d.CtxKp[0] : nullptr; a.n_ctx = cf.n_ctx; a.V = cf.voc_size; a.ctx_vocab = cf.ctx_vocab;
  return 0;
}
// where layer l of a wide scan takes its gate inputs from (v2: second generation; f8, f8_tab: fwd_wide_layer)
static int wide_inputs(const FwdCall& c, int l, bool v2, bool f8, bool f8_tab, KlScanFwdWide& a) {
  kl_handle* h = c.h; WindowWs& w = c.w; const kl_config& cf = h->cfg; const Derived& d = h->d; hipStream_t s = c.s;
  if (l > 0) {
    // (second generation: P in bf16, gate-interleaved -- half the bytes written here and read by the scan)
    const bool p_bf16 = v2 && h->scan2_bf16;
    KL_TRY(project_inputs(c, l, v2, p_bf16, p_bf16 && h->proj_ws));
    a.P = w.P1; a.p_bf16 = p_bf16 ? 1 : 0;
  } else if (f8_tab) {
    KL_TRY(build_comb(h, s));
    KL_TRY(kl_launch_rows_tm(c.idx, c.ctx, cf.n_ctx, c.B, c.T, cf.voc_size, cf.ctx_vocab, w.ids_tm, s));
    a.P = reinterpret_cast<const float*>(d.comb); a.p_bf16 = 1;
    a.ids_tm = w.ids_tm;      // (here: row numbers of d.comb, [T][B])
    a.V = cf.voc_size; a.ctx_vocab = cf.ctx_vocab;
  } else if (v2 && (cf.n_ctx > 1 || f8)) {
    // several context variables: the scan's table mode adds ONE context row to the character row, so the gate inputs
    // of layer 0 are gathered into P rows first (as the layers above get them from proj_ws_kernel)
    KL_TRY(kl_launch_p_gather_il(d.EKp, d.CtxKp.data(), cf.n_ctx, c.idx, c.ctx, c.B, c.T, c.W, cf.voc_size, cf.ctx_vocab, reinterpret_cast<bf16_t*>(w.P1), s));
    a.P = w.P1; a.p_bf16 = 1;
  } else if (v2) return wide2_table_mode(c, a);
  else wide_tables(c, a);
  return 0;
}

// one layer of the wide family: its input side, the hand-off armed, then the first scan that takes it -- eight-wave, second or first generation
static int fwd_wide_layer(const FwdCall& c, int l) {
  kl_handle* h = c.h; WindowWs& w = c.w; const kl_config& cf = h->cfg; const Derived& d = h->d; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W;
  if (!w.km_plan) KL_TRY(kl_launch_transpose_bf16((const bf16_t*)w.H[l], W, w.HTf[l], (long)(T + 1) * B, B, W, s));
  KlScanFwdWide a = wide_layer_args(c, l);
  const bool v2 = w.scan2_rows != 0;
  // the eight-wave scan (lstm_scan_fwd8.hip) takes bf16 P rows only: layer 0's gate inputs are gathered in front of it
  // (layer 0 with one context variable stays on the 16-wave scan's table mode: gathering its P rows first costs more -- 1.25 ms at 3072
  //  streams -- than the eight-wave scan saves; KL_FWD8=2 takes it for layer 0 as well; else it gathers them from the table of all sums, d.comb)
  const bool f8_tab = v2 && l == 0 && h->fwd8 && h->fwd8_tab && !h->fwd8_all && d.comb != nullptr && cf.n_ctx == 1 && w.scan2_rows == 32 &&
                      h->scan2_bf16 && h->sentinel_roll && T >= 3 && h->fwd8_ls;
  const bool f8 = v2 && h->fwd8 && w.scan2_rows == 32 && h->scan2_bf16 && h->sentinel_roll && T >= 3 &&
                  (l > 0 || cf.n_ctx > 1 || h->fwd8_all || f8_tab);
  KL_TRY(wide_inputs(c, l, v2, f8, f8_tab, a));
  a.Cb = (v2 && w.scan2_bwd && h->scan2_bf16) ? w.Cb[l] : nullptr;      // (the backward scans read the cell states as bf16, blocks 0..T)
  a.HT = w.km_plan ? nullptr : w.HTf[l]; a.ldt = (long)(T + 1) * B;       // (K-major GEMMs: no transposed outputs)
  a.HdT = (a.Hd && !w.km_plan) ? w.HdT[l] : nullptr; a.ldt_d = (long)B * T;
  a.counters = w.scan_cnt; a.sentinel = h->sentinel ? 1 : 0;
  a.xcc_slots = (a.sentinel && h->xcd_local) ? w.scan_status + 4 : nullptr;
  a.gen = (unsigned)(1 + l);                   // (the posts are zeroed once per window: a token per launch)
  // hand-off by data: the blocks the scan is going to publish start out as sentinels (rolling: only the first two); else by counters
  if (a.sentinel && v2 && h->sentinel_roll && T >= 3) a.sentinel = 2;
  KL_TRY(arm_publish(c, a.H + c.BW, a.sentinel == 2 ? ARM_ROLLING : a.sentinel ? ARM_ALL_STEPS : ARM_COUNTERS));
  // (two phases ahead needs the rows to have been published a phase before the request: three or more phases per workgroup)
  a.pf_mode = h->scan2_pf >= 0 ? h->scan2_pf : (v2 && kl_scan_wide2_phases(B, T, W, w.scan2_rows, w.scan2_rows == 16 ? 5 : 4) >= 3 ? 2 : 1);
  h->trace_begin(0, s);      // (every layer's scan launch is timed while tracing)
  bool took8 = false;
  if (f8 && a.sentinel == 2) {
    KlScanFwdWide a8 = a;
    a8.xcc_slots = h->fwd8_local ? w.scan_status + 4 : nullptr;
    a8.pf_mode = h->fwd8_pf >= 0 ? h->fwd8_pf : (h->fwd8_ls ? 0 : 1);      // (measured at 3072 streams: two-barrier form 3.06 / 3.32 / 3.30 ms per launch with pf 0 / 1 / 3)
    const int e8 = kl_launch_scan_fwd8(a8, s, h->fwd8_ls);
    if (e8 != KL_ERR_SHAPE) KL_TRY(e8);
    took8 = e8 == 0;
  }
  if (!took8 && f8_tab) KL_TRY(wide2_table_mode(c, a));      // (the eight-wave scan did not take the shape: the 16-wave scan's own table mode)
  if (a.p_bf16) w.p_bf16_mask |= 1u << l;
  if (!took8) KL_TRY(v2 ? kl_launch_scan_fwd_wide2(a, w.scan2_rows, s) : kl_launch_scan_fwd_wide(a, s));
  trace_fwd_scan(c, took8 ? "lstm_scan_fwd8_kernel" : v2 ? "lstm_scan_fwd_wide2_kernel" : "lstm_scan_fwd_wide_kernel", layer_flops(c));
  return 0;
}

// Many streams (B >= 512 at cfg2), widths 512 and 256: one layer per launch with 64-unit workgroups.  The input contraction of
// layers >= 1 comes from one big GEMM over all steps, layer 0 reads the look-up tables directly, and the scans also leave H^T
// for the weight gradients (w.ht_ready: only here, and not where those read K-major).
static int fwd_wide(const FwdCall& c) {
  const kl_handle* h = c.h;
  c.w.ht_ready = false;
  if (!(c.training && h->scan_enabled && h->wide_fwd_min > 0 && kl_scan_fwd_wide_applicable(c.B, c.T, c.W) &&
        c.n_rb * (c.W / 64) >= h->wide_fwd_min)) return FWD_PASS;
  for (int l = 0; l < c.L; ++l) KL_TRY(fwd_wide_layer(c, l));
  c.w.ht_ready = !c.w.km_plan;
  return 0;
}

// Width 128 (the reference's own model sizes): a workgroup = a 16-row block of streams with ALL hidden units of a layer -- no
// hand-off of state between workgroups (lstm_scan_w128.hip).  Layer 0 takes its gate inputs straight from the look-up tables
// (up to two context variables; else the rows gather_layer0 left), the layers above it contract their inputs inside the scan.
static bool fwd_w128_mine(const FwdCall& c) {
  const kl_handle* h = c.h;
  return c.training && h->scan_enabled && h->w128 && c.B >= h->w128_min && kl_scan_w128_applicable(c.B, c.T, c.W);
}
// ... layer 0 from the tables: the one family that does not read gather_layer0's rows
static bool fwd_w128_tables(const FwdCall& c) {
  return fwd_w128_mine(c) && c.h->w128_tables && c.h->cfg.n_ctx <= kl_scan_w128_tables_max_ctx();
}
static int w128_single(const FwdCall& c, const KlScanFwdWide& a) {
  c.h->trace_begin(0, c.s);
  KL_TRY(kl_launch_scan_fwd_w128(a, c.s));
  trace_fwd_scan(c, "lstm_scan_fwd_w128_kernel", layer_flops(c));
  return 0;
}
// All layers in one launch where that fits the CUs (layers x 16-row blocks <= 256: up to 2048 streams at depth 2): a layer
// follows the one below it a step behind, polling the rows that one publishes -- which therefore start out as sentinels.
static int w128_multi(const FwdCall& c, KlScanFwdWide* layer_args) {
  kl_handle* h = c.h;
  if (!kl_scan_w128_multi_fits(c.B, c.L)) return FWD_PASS;
  const bool roll = h->sentinel_roll && c.T >= 3;      // (rolling sentinels: only the first two steps start out armed)
  for (int l = 1; l < c.L; ++l) {
    layer_args[l - 1].sentinel = roll ? 2 : 1;
    KL_TRY(arm_publish(c, const_cast<bf16_t*>(layer_args[l].X), roll ? ARM_ROLLING : ARM_ALL_STEPS));
  }
  h->trace_begin(0, c.s);
  const int e = kl_launch_scan_fwd_w128_multi(layer_args, c.L, c.s);
  if (e != 0) return e == KL_ERR_SHAPE ? FWD_PASS : e;
  trace_fwd_scan(c, "lstm_scan_fwd_w128_multi_kernel", (double)(2 * c.L - 1) * layer_flops(c));      // (recurrent contractions + the input ones)
  return 0;
}
static int fwd_w128(const FwdCall& c) {
  const kl_handle* h = c.h; const int L = c.L;
  if (!fwd_w128_mine(c)) return FWD_PASS;
  const bool tabs = fwd_w128_tables(c);
  KlScanFwdWide layer_args[KL_SCAN_MAXL];
  const bool try_multi = h->w128_multi && h->w128_fuse && L >= 2 && L <= KL_SCAN_MAXL;
  for (int l = 0; l < L; ++l) {
    KlScanFwdWide& a = layer_args[l < KL_SCAN_MAXL ? l : 0];
    a = wide_layer_args(c, l);
    a.P = c.w.P1;
    if (l == 0 && tabs) wide_tables(c, a);
    if (l > 0 && !h->w128_fuse) KL_TRY(project_inputs(c, l, false, false, false));
    if (l > 0 && h->w128_fuse) {      // the input contraction inside the scan: no P rows, no product over all steps
      a.P = nullptr; a.KT = h->d.KT_hi[l]; a.X = layer_in(c, l); a.bias = h->params + h->off_b[l];
    }
    if (!try_multi) KL_TRY(w128_single(c, a));
  }
  if (!try_multi) return 0;
  const int e = w128_multi(c, layer_args);
  if (e != FWD_PASS) return e;
  for (int l = 0; l < L; ++l) KL_TRY(w128_single(c, layer_args[l]));      // (the multi launch did not take the shape)
  return 0;
}

// what a thin, w32 (KlScanFwd) or split-precision (KlScanFwdSplit) scan over n layers is told whichever it is
template <class A> static A scan_args(const FwdCall& c, int n) {
  A a;
  memset(&a, 0, sizeof(a));
  a.B = c.B; a.T = c.T; a.W = c.W; a.L = n;
  a.P1 = c.w.P1; a.counters = c.w.scan_cnt; a.status = c.w.scan_status;
  return a;
}
// layer l as the scan's layer j; input_side: ... with K_l^T and b_l (l > 0), for a scan that contracts the layer's inputs itself
static void thin_layer_args(const FwdCall& c, KlScanFwd& a, int l, int j, bool input_side) {
  const kl_handle* h = c.h; const LayerMask m = layer_mask(c, l);
  a.UT[j] = h->d.UT_hi[l];
  if (input_side && l > 0) { a.KT[j] = h->d.KT_hi[l]; a.bias[j] = h->params + h->off_b[l]; }
  a.H[j] = (bf16_t*)c.w.H[l]; a.C[j] = c.w.C[l]; a.G[j] = c.w.G[l];
  a.Hd[j] = m.Hd; a.mask[j] = m.mask;
}

// Width 1024 (the cfg5 topology): the recurrent weights of 16 units alone fill half of a 256-thread workgroup's registers, so neither
// the fused scans (U and K resident) nor the 64-unit wide scans apply.  One layer per launch with the thin workgroups instead, the
// input side from one GEMM over all steps as in the wide path (layer 0: gather_layer0's rows).  The same layer-by-layer launches
// serve models deeper than the fused scans' four layers (the reference takes up to ten, scripts/run.py:35).
static int fwd_layer_by_layer(const FwdCall& c) {
  kl_handle* h = c.h; WindowWs& w = c.w; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W, L = c.L;
  if (!(c.training && h->scan_enabled && (W == 1024 || L > KL_SCAN_MAXL))) return FWD_PASS;
  for (int l = 0; l < L; ++l) {
    if (l > 0) KL_TRY(project_inputs(c, l, false, false, false));
    KlScanFwd a = scan_args<KlScanFwd>(c, 1);
    thin_layer_args(c, a, l, 0, false);
    // width 1024 from eight row blocks: eight-wave workgroups of 32 units, the state tile through LDS, hand-off by
    // data sentinels inside one XCD (lstm_scan_w32.hip); else the thin workgroups with their counters
    const bool w32 = h->w32 && c.n_rb >= h->w32_min_rb && kl_scan_w32_applicable(B, T, W);
    if (w32) {
      a.sentinel = 1;
      a.xcc_slots = h->w32_local ? w.scan_status + 4 : nullptr;
      a.gen = (unsigned)(1 + l);                   // (the posts are zeroed once per window: a token per launch)
    }
    KL_TRY(arm_publish(c, a.H[0] + c.BW, w32 ? ARM_ALL_STEPS : ARM_COUNTERS));
    h->trace_begin(0, s);      // (every layer's scan launch is timed while tracing)
    const int e = w32 ? kl_launch_scan_fwd_w32(a, s) : kl_launch_scan_fwd(a, s);
    if (e == KL_ERR_SHAPE && l == 0) {
      // too many row blocks: a later family takes the window (P1 still holds gather_layer0's rows: this gather repeats it -- DESIGN.md, the forward half)
      KL_TRY(gather_layer0(c));
      return FWD_PASS;
    }
    if (e != 0) return e;
    trace_fwd_scan(c, w32 ? "lstm_scan_fwd_w32_kernel" : "lstm_scan_fwd_kernel", layer_flops(c));
  }
  return 0;
}

// ---- rating windows in split precision: the scans exchange their state as (hi, lo) bf16 planes ----
// (as thin_layer_args)
static void split_layer_args(const FwdCall& c, KlScanFwdSplit& a, int l, int j, bool input_side) {
  const kl_handle* h = c.h; const Derived& d = h->d;
  a.UT_hi[j] = d.UT_hi[l]; a.UT_lo[j] = d.UT_lo[l];
  if (input_side && l > 0) { a.KT_hi[j] = d.KT_hi[l]; a.KT_lo[j] = d.KT_lo[l]; a.bias[j] = h->params + h->off_b[l]; }
  a.Xhi[j] = c.w.Xhi[l]; a.Xlo[j] = c.w.Xlo[l]; a.Hf[j] = (float*)c.w.H[l]; a.C[j] = c.w.C[l];
}
// layer l's carried-in state as (hi, lo) planes
static int split_planes(const FwdCall& c, int l) {
  return kl_launch_f32_to_bf16_t((const float*)c.w.H[l], c.W, c.B, c.W, c.w.Xhi[l], c.w.Xlo[l], c.W, 0, c.s);
}
// hand-off by data: the blocks of both planes that layer l's scan is going to publish start out as sentinels
static int arm_split(const FwdCall& c, int l) {
  KL_TRY(arm_publish(c, c.w.Xhi[l] + c.BW, ARM_ALL_STEPS));
  return arm_publish(c, c.w.Xlo[l] + c.BW, ARM_ALL_STEPS);
}
// width 1024 (cfg5), where the layers run one after the other: the shapes whose planes the sentinel scans can index
static bool split_w1024(const FwdCall& c, int max_rb) {
  const kl_handle* h = c.h;
  return !c.training && c.split == KL_PREC_SPLIT && h->scan_enabled && h->split_sentinel && c.W == 1024 && c.n_rb <= max_rb &&
         (long)(c.T + 1) * c.B * c.W * 2 <= 0x7fffffffL;
}

// Width 1024 with few streams (two row blocks at most): eight units per workgroup, so that U and K fit and TWO layers
// run as a wavefront per launch (256 workgroups, one per CU): half the chain of fwd_split_layers
static int fwd_split_pairs(const FwdCall& c) {
  if (!(split_w1024(c, 2) && c.h->split8)) return FWD_PASS;
  for (int l0 = 0; l0 < c.L; l0 += 2) {
    const int nl = c.L - l0 < 2 ? c.L - l0 : 2;
    if (l0 + nl > KL_SCAN_MAXL) {
      if (l0 > 0) note_passed(c, KL_FWD_SPLIT_PAIRS);      // (the pairs below l0 have gone out)
      return FWD_PASS;
    }
    KlScanFwdSplit a = scan_args<KlScanFwdSplit>(c, nl);
    a.l0 = l0; a.units8 = 1;
    for (int l = (l0 > 0 ? l0 - 1 : 0); l < l0 + nl; ++l) split_layer_args(c, a, l, l, true);
    a.sentinel = 1;
    for (int l = l0; l < l0 + nl; ++l) {
      KL_TRY(split_planes(c, l));
      KL_TRY(arm_split(c, l));
    }
    const int e = kl_launch_scan_fwd_split(a, c.s);
    if (e == KL_ERR_SHAPE && l0 == 0) {      // (fewer than 256 CUs: layer by layer)
      note_passed(c, KL_FWD_SPLIT_PAIRS);      // (the planes of the first pair were split and armed)
      return FWD_PASS;
    }
    if (e != 0) return e;
  }
  note_finished(c, KL_FWD_SPLIT_PAIRS, KL_FWD_HANDOFF_SENTINELS, 1, 0, 0);      // (P1: gather_layer0's rows)
  return 0;
}

// Width 1024: the (hi, lo) planes of the recurrent weights of 16 units are a workgroup's whole register budget, so the layers run
// one after the other -- per layer ONE split-precision product over all steps for the input side (layer 0: gather_layer0's rows),
// then the persistent scan with U alone (was: a launch per step and layer wavefront, 18 ms per 1 x 512 window)
static int fwd_split_layers(const FwdCall& c) {
  kl_handle* h = c.h; WindowWs& w = c.w; const Derived& d = h->d; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W;
  if (!split_w1024(c, 16)) return FWD_PASS;
  for (int l = 0; l < c.L; ++l) {
    const float* bias = h->params + h->off_b[l];
    if (l > 0 && B * T >= 2048) {
      // many rows: the three products of the split (hi.hi + bias, lo.hi, hi.lo) on the big-tile GEMM, over the (hi, lo)
      // planes the scan below left behind (the thin GEMM re-reads the weights per 32 rows: 2.9 ms per layer at 16 x 512 rows)
      const bf16_t* xh = w.Xhi[l - 1] + c.BW;
      const bf16_t* xl = w.Xlo[l - 1] + c.BW;
      KL_TRY(kl_launch_gemm_tn(xh, d.KT_hi[l], w.P1, bias, B * T, 4 * W, W, W, W, 4 * W, 0, 1, 1.f, s));
      KL_TRY(kl_launch_gemm_tn(xl, d.KT_hi[l], w.P1, nullptr, B * T, 4 * W, W, W, W, 4 * W, 2, 1, 1.f, s));
      KL_TRY(kl_launch_gemm_tn(xh, d.KT_lo[l], w.P1, nullptr, B * T, 4 * W, W, W, W, 4 * W, 2, 1, 1.f, s));
      if (c.note) c.note->ring_mask |= 1u << l;
    } else if (l > 0) {
      KlOperand op;
      memset(&op, 0, sizeof(op));
      op.A = h_rows(c, l - 1, 1); op.lda = W; op.a_is_f32 = 1;
      op.WT_hi = d.KT_hi[l]; op.WT_lo = d.KT_lo[l]; op.ldw = W; op.K = W;
      KL_TRY(kl_launch_thin_gemm(&op, B * T, 4 * W, w.P1, 4 * W, bias, KL_PREC_SPLIT, s));
      if (c.note) c.note->thin_mask |= 1u << l;
    }
    KlScanFwdSplit a = scan_args<KlScanFwdSplit>(c, 1);
    split_layer_args(c, a, l, 0, false);
    a.sentinel = 1;
    KL_TRY(split_planes(c, l));
    KL_TRY(arm_split(c, l));
    KL_TRY(kl_launch_scan_fwd_split(a, s));
  }
  note_finished(c, KL_FWD_SPLIT_LAYERS, KL_FWD_HANDOFF_SENTINELS, 1, 0, c.L - 1);      // (P1: the top layer's gate inputs)
  return 0;
}

// one persistent launch for all layers and steps, hand-off by sentinels or (KL_SPLIT_SENTINEL=0) by counters zeroed write-through
static int fwd_split_fused(const FwdCall& c) {
  const kl_handle* h = c.h; const int L = c.L;
  if (!(!c.training && c.split == KL_PREC_SPLIT && h->scan_enabled && L <= KL_SCAN_MAXL)) return FWD_PASS;
  KlScanFwdSplit a = scan_args<KlScanFwdSplit>(c, L);
  for (int l = 0; l < L; ++l) split_layer_args(c, a, l, l, true);
  for (int l = 0; l < L; ++l) KL_TRY(split_planes(c, l));
  a.sentinel = h->split_sentinel ? 1 : 0;
  if (a.sentinel)
    for (int l = 0; l < L; ++l) KL_TRY(arm_split(c, l));
  else
    KL_TRY(kl_zero_coherent_async(c.w.scan_cnt, (size_t)L * c.n_rb * c.T, c.s));      // (all layers' counters)
  const int e = kl_launch_scan_fwd_split(a, c.s);
  if (e == KL_ERR_SHAPE) note_passed(c, KL_FWD_SPLIT_FUSED);      // (the planes were split and armed, or the counters zeroed)
  if (e == 0) note_finished(c, KL_FWD_SPLIT_FUSED, a.sentinel ? KL_FWD_HANDOFF_SENTINELS : KL_FWD_HANDOFF_COUNTERS, 1, 0, 0);
  return e == KL_ERR_SHAPE ? FWD_PASS : e;
}

// the fused thin training scan: all layers (at most KL_SCAN_MAXL) and steps in one launch where the shape allows it, hand-off by counters
static int fwd_fused_thin(const FwdCall& c) {
  kl_handle* h = c.h; const int L = c.L;
  if (!(c.training && h->scan_enabled && L <= KL_SCAN_MAXL)) return FWD_PASS;
  KlScanFwd a = scan_args<KlScanFwd>(c, L);
  for (int l = 0; l < L; ++l) thin_layer_args(c, a, l, l, true);
  KL_TRY(kl_zero_coherent_async(c.w.scan_cnt, (size_t)L * c.n_rb * c.T, c.s));      // (all layers' counters)
  h->trace_begin(0, c.s);
  const int e = kl_launch_scan_fwd(a, c.s);
  if (e != 0) return e == KL_ERR_SHAPE ? FWD_PASS : e;
  trace_fwd_scan(c, "lstm_scan_fwd_kernel", (2.0 * L - 1.0) * layer_flops(c));   // U_l for all l, K_l for l >= 1
  return 0;
}

// step t of layer l as the launch-per-step kernel takes it: z = [X . K_l^T + b_l | P1 rows (layer 0)] + h_{t-1} . U_l^T, then the cell
static KlFwdStep wavefront_step(const FwdCall& c, int l, int t) {
  const kl_handle* h = c.h; const WindowWs& w = c.w; const Derived& d = h->d;
  const int B = c.B, W = c.W; const size_t BW = c.BW;
  const bool lo = c.split == KL_PREC_SPLIT;
  KlFwdStep S;
  memset(&S, 0, sizeof(S));
  S.n_rows = B; S.W = W; S.split = c.split; S.n_ops = l > 0 ? 2 : 1;
  KlOperand& u = S.op[S.n_ops - 1];      // the recurrent side comes last
  u.A = h_rows(c, l, t); u.a_is_f32 = c.training ? 0 : 1; u.lda = W;
  u.WT_hi = d.UT_hi[l]; u.WT_lo = lo ? d.UT_lo[l] : nullptr; u.ldw = W; u.K = W;
  if (l > 0) {
    KlOperand& o = S.op[0];
    o.A = c.training ? (const void*)(layer_in(c, l) + (size_t)t * BW) : h_rows(c, l - 1, t + 1); o.a_is_f32 = c.training ? 0 : 1;
    o.lda = W; o.WT_hi = d.KT_hi[l]; o.WT_lo = lo ? d.KT_lo[l] : nullptr; o.ldw = W; o.K = W;
    S.bias = h->params + h->off_b[l];
  } else {
    S.T1 = w.P1 + (size_t)t * B * 4 * W; S.t1_ld = 4 * W;
  }
  S.c_prev = w.C[l] + (size_t)t * BW; S.c_prev_ld = W;
  S.c_out = w.C[l] + (size_t)(t + 1) * BW; S.c_out_ld = W;
  if (c.training) {
    const LayerMask m = layer_mask(c, l);
    S.h_out_bf16 = (bf16_t*)w.H[l] + (size_t)(t + 1) * BW; S.h_out_bf16_ld = W;
    S.gates_out = w.G[l] + (size_t)t * B * 4 * W; S.gates_ld = 4 * W;
    if (m.mask) {
      S.hmask = m.mask; S.hmask_ld = W;
      S.hd_out_bf16 = m.Hd + (size_t)t * BW; S.hd_out_ld = W;
    }
  } else {
    S.h_out_f32 = (float*)w.H[l] + (size_t)(t + 1) * BW; S.h_out_f32_ld = W;
  }
  return S;
}

// everything else: the launch-per-step layer wavefront (diagonal dgl: layer l runs step dgl - l)
static int fwd_wavefront(const FwdCall& c) {
  kl_handle* h = c.h; const int T = c.T, L = c.L;
  for (int dgl = 0; dgl < T + L - 1; ++dgl) {
    KlFwdStep steps[16];     // one per layer (config_ok: depth <= 16); launched in packs of 4 below
    int ns = 0;
    for (int l = 0; l < L; ++l)
      if (dgl - l >= 0 && dgl - l < T) steps[ns++] = wavefront_step(c, l, dgl - l);
    // a launch packs at most 4 independent steps
    for (int i = 0; i < ns; i += 4) {
      // trace: one event pair brackets 8 consecutive steady-state launches (dgl = 8k .. 8k+7)
      const bool steady = (ns == L) && dgl >= L && dgl + 8 < T;
      if (steady && dgl % 8 == 0) h->trace_begin(0, c.s);
      KL_TRY(kl_launch_fwd_steps(steps + i, ns - i < 4 ? ns - i : 4, c.s));
      if (steady && dgl % 8 == 7) h->trace_end(0, c.s);
    }
  }
  note_finished(c, KL_FWD_WAVEFRONT, KL_FWD_HANDOFF_NONE, 0, 1, 0);      // (every step writes its C block; no planes; P1: gather_layer0's rows)
  return 0;
}

// forward over one window; fills ws (activations) and states: the carried-in state into row block 0, the first scan family that
// takes the window (asked in this order), the last row block back into the state
int forward_impl(kl_handle* h, int B, int T, const int* idx, const int* ctx, float* states, const float* masks,
                 int training, WindowWs& w, hipStream_t s) {
  const int W = h->cfg.width, L = h->cfg.depth;
  // (the inference layout's P1 is the first array carved: its address is the workspace's)
  kl_handle::ForwardNote* note = training ? nullptr : h->forward_note(B, T, w.P1, true);
  if (note) *note = kl_handle::ForwardNote{B, T, w.P1, h->precision};
  const FwdCall c = {h, B, T, idx, ctx, states, masks, training, training ? 1 : h->precision, w, s, W, L, (size_t)B * W, (B + 15) / 16, note};
  for (int l = 0; l < L; ++l)
    KL_TRY(kl_launch_state_to_rows(states, B, W, L, l, training ? (bf16_t*)w.H[l] : nullptr, training ? nullptr : (float*)w.H[l], w.C[l], s));
  int e = fwd_wide(c);
  // (every family below reads layer 0's gate inputs as P1 rows, but width 128 where it reads the tables itself)
  if (e == FWD_PASS && !fwd_w128_tables(c)) KL_TRY(gather_layer0(c));
  if (e == FWD_PASS) e = fwd_w128(c);
  if (e == FWD_PASS) e = fwd_layer_by_layer(c);
  if (e == FWD_PASS) e = fwd_split_pairs(c);
  if (e == FWD_PASS) e = fwd_split_layers(c);
  if (e == FWD_PASS) e = fwd_split_fused(c);
  if (e == FWD_PASS) e = fwd_fused_thin(c);
  if (e == FWD_PASS) e = fwd_wavefront(c);
  KL_TRY(e);
  for (int l = 0; l < L; ++l)
    KL_TRY(kl_launch_rows_to_state(h_rows(c, l, T), training ? 0 : 1, w.C[l] + (size_t)T * c.BW, B, W, L, l, states, s));
  return 0;
}

__global__ void scan_status_kernel(const unsigned* status, float* loss_acc) {
  if (threadIdx.x == 0 && (status[0] | status[1]) != 0) loss_acc[3] += 1.f;
}

__global__ void state_dist2_kernel(const float* __restrict__ pool, long slot_stride, int W, int k,
                                   const int* __restrict__ a, const int* __restrict__ b, int n,
                                   float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* pa = pool + (long)a[i] * slot_stride + (long)k * W;
  const float* pb = pool + (long)b[i] * slot_stride + (long)k * W;
  const float acc = kl_wave_dist2(pa, pb, W, lane);      // (kl_state_dist.h: shared with kl_edge_decode)
  if (lane == 0) out[i] = acc;
}

}  // namespace

extern "C" {

int kl_abi_version(void) { return KL_ABI_VERSION; }

const char* kl_error_string(int code) {
  switch (code) {
    case KL_OK: return "ok";
    case KL_ERR_SHAPE: return "unsupported or inconsistent dimensions";
    case KL_ERR_LAUNCH: return "HIP launch/runtime error";
    case KL_ERR_STATE: return "call order violated (bind/prepare first)";
    case KL_ERR_WORKSPACE: return "workspace too small";
    case KL_ERR_ARG: return "null or invalid argument";
    default: return "unknown error";
  }
}

size_t kl_param_count(const kl_config* cfg) {
  if (!config_ok(cfg)) return 0;
  kl_handle tmp;
  tmp.cfg = *cfg;
  layout(&tmp);
  return tmp.n_params;
}

int kl_param_layout(const kl_config* cfg, int index, char* name, size_t name_cap, size_t* offset, size_t* rows,
                    size_t* cols) {
  if (!config_ok(cfg) || index < 0) return KL_ERR_ARG;
  kl_handle t;
  t.cfg = *cfg;
  layout(&t);
  const size_t W = cfg->width;
  char buf[32];
  size_t off, r, c;
  const int n_emb = 1 + cfg->n_ctx;
  if (index == 0) {
    snprintf(buf, sizeof buf, "E"); off = t.off_E; r = cfg->voc_size; c = W;
  } else if (index < n_emb) {
    snprintf(buf, sizeof buf, "Ctx%d", index - 1); off = t.off_Ctx[index - 1]; r = cfg->ctx_vocab; c = cfg->ctx_dim;
  } else {
    const int j = index - n_emb, l = j / 3, k = j % 3;
    if (l >= cfg->depth) return KL_ERR_ARG;
    const size_t D = l == 0 ? W + (size_t)cfg->ctx_dim * cfg->n_ctx : W;
    if (k == 0) { snprintf(buf, sizeof buf, "K%d", l); off = t.off_K[l]; r = D; c = 4 * W; }
    else if (k == 1) { snprintf(buf, sizeof buf, "U%d", l); off = t.off_U[l]; r = W; c = 4 * W; }
    else { snprintf(buf, sizeof buf, "b%d", l); off = t.off_b[l]; r = 1; c = 4 * W; }
  }
  if (name && name_cap) { strncpy(name, buf, name_cap - 1); name[name_cap - 1] = 0; }
  if (offset) *offset = off;
  if (rows) *rows = r;
  if (cols) *cols = c;
  return 0;
}

kl_handle* kl_create(const kl_config* cfg) {
  if (!config_ok(cfg)) return nullptr;
  kl_handle* h = new kl_handle();
  h->cfg = *cfg;
  layout(h);
  // (read HERE, not with the other switches in kl_bind: it decides how large the derived workspace is -- kl_derived_bytes)
  const char* env8tb = getenv("KL_FWD8_TAB");
  if (env8tb) h->fwd8_tab = atoi(env8tb) != 0;
  // (... and this one how large a training window's workspace is -- kl_window_workspace_bytes)
  const char* env9 = getenv("KL_SEGSUM");
  if (env9) h->segsum = atoi(env9) != 0;
  return h;
}

void kl_destroy(kl_handle* h) {
  if (h) {
    h->drop_graphs();
    for (auto& list : h->trace_ev)
      for (auto& ev : list) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
      }
  }
  delete h;
}

size_t kl_derived_bytes(const kl_handle* h) { return h ? carve_derived(h, nullptr, nullptr) : 0; }

int kl_bind(kl_handle* h, float* params, void* derived, size_t derived_bytes) {
  if (!h || !params || !derived) return KL_ERR_ARG;
  if (derived_bytes < carve_derived(h, nullptr, nullptr)) return KL_ERR_WORKSPACE;
  h->params = params;
  h->derived_ws = derived;
  h->derived_bytes = derived_bytes;
  carve_derived(h, derived, &h->d);
  h->precision = 0;
  h->drop_graphs();
  const char* env = getenv("KL_GRAPH");
  h->graphs_enabled = !(env && env[0] == '0');
  const char* env2 = getenv("KL_SCAN");
  h->scan_enabled = !(env2 && env2[0] == '0');
  const char* env3 = getenv("KL_SEQ_BWD");
  h->seq_bwd = !(env3 && env3[0] == '0');
  const char* env4 = getenv("KL_WIDE_BWD");
  h->wide_bwd = !(env4 && env4[0] == '0');
  const char* env7 = getenv("KL_SENTINEL");
  h->sentinel = !(env7 && env7[0] == '0');
  const char* env7e = getenv("KL_GEMM_AN");
  h->gemm_an = !(env7e && env7e[0] == '0');
  const char* env7c = getenv("KL_XCD_LOCAL");
  h->xcd_local = env7c && env7c[0] == '1';
  const char* env7b = getenv("KL_SENTINEL_BWD");
  h->sentinel_bwd = h->sentinel && !(env7b && env7b[0] == '0');
  h->sentinel_bwd_all = env7b && env7b[0] == '2';
  const char* env7f = getenv("KL_SENTINEL_ROLL");
  h->sentinel_roll = !(env7f && env7f[0] == '0');
  const char* env7d = getenv("KL_XCD_LOCAL_BWD");
  h->xcd_local_bwd = h->xcd_local && env7d && env7d[0] == '1';
  const char* env6f = getenv("KL_W32");
  h->w32 = !(env6f && env6f[0] == '0');
  const char* env6g = getenv("KL_W32_LOCAL");
  h->w32_local = env6g && env6g[0] == '1';
  const char* env6h = getenv("KL_W32_MIN_RB");
  h->w32_min_rb = env6h ? atoi(env6h) : 8;
  const char* env6j = getenv("KL_SPLIT8");
  h->split8 = !(env6j && env6j[0] == '0');
  const char* env6c = getenv("KL_SPLIT_SENTINEL");
  h->split_sentinel = !(env6c && env6c[0] == '0');
  const char* env6b = getenv("KL_INC_SMALL");
  h->inc_small = !(env6b && env6b[0] == '0');
  const char* env6 = getenv("KL_FUSED_STEP");
  h->fused_step = !(env6 && env6[0] == '0');
  const char* env6k = getenv("KL_INC_TILE");
  h->inc_tile = !(env6k && env6k[0] == '0');
  const char* env6l = getenv("KL_TILE_VAR");
  h->tile_var = env6l ? atoi(env6l) : 0;
  const char* env6r = getenv("KL_TILE_ROWS");
  if (env6r) h->tile_rows = atoi(env6r);
  const char* env6m = getenv("KL_OUT_FUSED");
  h->out_fused = !(env6m && env6m[0] == '0');
  const char* env6n = getenv("KL_OUT_FUSED_MIN");
  if (env6n) h->out_fused_min = atoi(env6n);
  const char* env6o = getenv("KL_INC_SMALL_MIN");
  if (env6o) h->inc_small_min = atoi(env6o);
  const char* env6p = getenv("KL_HOST_KERNARG");
  h->host_kernarg = !(env6p && env6p[0] == '0');
  const char* env8 = getenv("KL_SCAN2");
  if (env8) h->scan2 = atoi(env8) != 0;
  const char* env8b = getenv("KL_SCAN2_ROWS");
  if (env8b) h->scan2_rows = atoi(env8b);
  const char* env8c = getenv("KL_SCAN2_PF");
  if (env8c) h->scan2_pf = atoi(env8c);
  const char* env8e = getenv("KL_SCAN2_BF16");
  if (env8e) h->scan2_bf16 = atoi(env8e) != 0;
  const char* env8i = getenv("KL_LOGITS_WS");
  if (env8i) h->logits_ws = atoi(env8i) != 0;
  const char* env8h = getenv("KL_PROJ_WS");
  if (env8h) h->proj_ws = atoi(env8h) != 0;
  const char* env8p = getenv("KL_W128");
  if (env8p) h->w128 = atoi(env8p) != 0;
  const char* env8s = getenv("KL_W128_FUSE");
  if (env8s) h->w128_fuse = atoi(env8s) != 0;
  const char* env8t = getenv("KL_W128_TABLES");
  if (env8t) h->w128_tables = atoi(env8t) != 0;
  const char* env8mm = getenv("KL_W128_MULTI");
  if (env8mm) h->w128_multi = atoi(env8mm) != 0;
  const char* env8q = getenv("KL_W128_MIN");
  if (env8q) h->w128_min = atoi(env8q);
  const char* env8m = getenv("KL_FWD8");
  if (env8m) { h->fwd8 = atoi(env8m) != 0; h->fwd8_all = atoi(env8m) == 2; }
  const char* env8r = getenv("KL_FWD8_LS");
  if (env8r) h->fwd8_ls = atoi(env8r) != 0;
  const char* env8n = getenv("KL_FWD8_LOCAL");
  if (env8n) h->fwd8_local = atoi(env8n) != 0;
  const char* env8o = getenv("KL_FWD8_PF");
  if (env8o) h->fwd8_pf = atoi(env8o);
  const char* env8l = getenv("KL_RT_LOCAL");
  if (env8l) h->rt_local = atoi(env8l) != 0;
  const char* env8k = getenv("KL_REGTILE");
  if (env8k) h->regtile = atoi(env8k) != 0;
  const char* env8g = getenv("KL_SCAN2_FLAGS");
  if (env8g) h->scan2_flags = atoi(env8g) != 0;
  h->flags_zeroed = false;
  const char* env8f = getenv("KL_FUSE_WG");
  if (env8f) h->fuse_wg = atoi(env8f) != 0;
  const char* env8d = getenv("KL_SCAN2_PFB");
  if (env8d) h->scan2_pfb = atoi(env8d);
  const char* env5 = getenv("KL_WIDE_FWD_MIN");
  if (env5) h->wide_fwd_min = atoi(env5);
  return kl_zero_page_ready();
}

int kl_prepare(kl_handle* h, int precision, void* stream) {
  if (!h) return KL_ERR_ARG;
  if (!h->params) return KL_ERR_STATE;
  if (precision != KL_PREC_BF16 && precision != KL_PREC_SPLIT) return KL_ERR_ARG;
  return prepare_impl(h, precision, (hipStream_t)stream);
}

size_t kl_window_workspace_bytes(const kl_handle* h, int B, int T, int training) {
  if (!h || B < 1 || T < 1) return 0;
  return carve_window(h, nullptr, B, T, training, nullptr);
}

// recurrence + output layer of an inference window (the non-training workspace layout): advances states, leaves the
// logits time-major in w.logits.  Shared by kl_forward_window and kl_rate_window, which differ in what they make of them.
static int window_logits(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, float* states, WindowWs& w,
                         hipStream_t s) {
  const int W = h->cfg.width, V = h->cfg.voc_size, L = h->cfg.depth;
  KL_TRY(kl_zero_async(w.scan_status, (4 + 256) * sizeof(unsigned), s));
  KL_TRY(forward_impl(h, B, T, idx, ctx, states, nullptr, 0, w, s));
  KlOperand op;
  memset(&op, 0, sizeof(op));
  op.A = (float*)w.H[L - 1] + (size_t)B * W; op.lda = W; op.a_is_f32 = 1;
  op.WT_hi = h->d.E_hi; op.WT_lo = h->precision == 3 ? h->d.E_lo : nullptr; op.ldw = W; op.K = W;
  return kl_launch_thin_gemm(&op, B * T, V, w.logits, V, nullptr, h->precision, s);
}

// the tail of a forward window in either layout: softmax + CE (means over mean_rows streams), probabilities batch-major, the scans' status
static int forward_window_tail(kl_handle* h, WindowWs& w, int B, int T, const int32_t* tgt, int mean_rows, float* probs, float* loss_acc, hipStream_t s) {
  const int V = h->cfg.voc_size;
  KL_TRY(kl_launch_softmax_ce(w.logits, V, B * T, V, tgt, B, T, 1.0f / (h->last_only ? (float)mean_rows : (float)mean_rows * (float)T),
                              nullptr, 0, tgt ? loss_acc : nullptr, w.rowstat, 1, s, h->last_only));
  if (probs) {
    if (B == 1) KL_TRY(hip_ok(hipMemcpyAsync(probs, w.logits, (size_t)T * V * sizeof(float), hipMemcpyDeviceToDevice, s)));
    else KL_TRY(kl_launch_rows_tm_to_bm(w.logits, V, probs, B, T, V, s));
  }
  // a timed-out hand-off in the persistent scan surfaces as loss_acc[3] != 0
  if (loss_acc) hipLaunchKernelGGL(scan_status_kernel, dim3(1), dim3(64), 0, s, w.scan_status, loss_acc);
  return hip_ok(hipGetLastError());
}

// ... and of a bf16 window on the TRAINING layout: the training forward -- persistent wide / fused scans and the big GEMMs --
// without the backward, instead of the launch-per-step inference kernels.  Shared by kl_forward_window (validation windows)
// and kl_rate_window_bulk, which differ in what they make of the logits.
static int window_logits_training(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, float* states, WindowWs& w,
                                  hipStream_t s) {
  const int W = h->cfg.width, V = h->cfg.voc_size, L = h->cfg.depth;
  KL_TRY(kl_zero_async(w.scan_status, (4 + 256) * sizeof(unsigned), s));
  w.km_plan = true;                  // (no transposed outputs: nothing is going to contract over the rows)
  w.scan2_rows = plan_scan2(h, B, T, true, false);
  KL_TRY(forward_impl(h, B, T, idx, ctx, states, nullptr, 1, w, s));
  const bf16_t* Htop = (const bf16_t*)w.H[L - 1] + (size_t)B * W;
  return kl_launch_gemm_tn(Htop, h->d.E_hi, w.logits, nullptr, B * T, V, W, W, W, V, 0, 1, 1.f, s);
}

static int forward_window_body(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                      float* states, float* probs, float* loss_acc, void* ws, size_t ws_bytes, void* stream) {
  if (!h || !idx || !states || !ws || B < 1 || T < 1) return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (!h->precision) return KL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  WindowWs w;
  // Windows in bf16 precision (validation after each epoch, rating.py:300-306: a fifth of every epoch's data) with
  // a training-size workspace take the TRAINING forward (window_logits_training; 1024 x 256 characters: 41 ms -> 4.6 ms).
  if (h->precision == KL_PREC_BF16 && ws_bytes >= carve_window(h, nullptr, B, T, 1, nullptr)) {
    carve_window(h, ws, B, T, 1, &w);
    KL_TRY(window_logits_training(h, B, T, idx, ctx, states, w, s));
    const int mean_rows = (h->loss_rows > 0 && h->loss_rows <= B) ? h->loss_rows : B;      // (a padded batch: kl_set_loss_rows)
    return forward_window_tail(h, w, B, T, tgt, mean_rows, probs, loss_acc, s);
  }
  if (ws_bytes < carve_window(h, ws, B, T, 0, &w)) return KL_ERR_WORKSPACE;
  KL_TRY(window_logits(h, B, T, idx, ctx, states, w, s));
  return forward_window_tail(h, w, B, T, tgt, B, probs, loss_acc, s);      // (this layout's means are over all B streams)
}

struct TrainCall {       // a kl_train_window call as the stages of its backward half see it
  kl_handle* h; int B, T; const int32_t *idx, *ctx, *tgt; const float* masks; float *grads, *loss_acc; hipStream_t s;
  WindowWs& w; kl_handle::ViewNote& note;      // what kl_test_window_view will say about this window: the stages note their routes in it
  int W, V, Vp, L, BT, BTp; size_t BW;
  int ksplit;            // split of the B*T contraction in the kl_launch_gemm_tn products
  long ldtf;             // leading dimension of the scans' transposed outputs HTf: (T+1) B
  int dh_mode;           // 1: dH travels as bf16 (second-generation backward scan)
  bool top_masked; float inv_count;
  bool wide_fits, seq128, sequential;      // which backward scans the shape and the switches allow (train_window_body)
};
// a backward-scan path's "not mine" (no public return code -- those are 0 .. 5, keraslm_hip.h)
constexpr int TRAIN_PASS = -1;
static_assert(TRAIN_PASS < KL_OK, "TRAIN_PASS must not be a public return code");

// one operand [B*T][N] of a product that contracts over the B*T rows, in the forms it exists in
struct RowsOperand {
  const bf16_t* km; long ld;      // as a scan wrote it, row-major (null: a one-hot matrix, which only has the transposed form)
  const bf16_t* t; long ldt;      // transposed [N][ldt]: by a scan (B*T columns), one-hot or dZ^T (BTp columns); null: "transpose me" (into w.HT)
};
// the (masked) outputs of layer l at steps 1..T: what layer l + 1 and the output layer read
static RowsOperand layer_out(const TrainCall& c, int l) {
  const WindowWs& w = c.w;
  if (c.masks != nullptr && l > 0) return {w.Hd[l], c.W, w.ht_ready ? w.HdT[l] : nullptr, c.BT};
  return {(const bf16_t*)w.H[l] + c.BW, c.W, w.ht_ready ? w.HTf[l] + c.B : nullptr, c.ldtf};
}

// One product over the B*T rows: out[M][N] (+)= a^T . x, or with out_t its transpose [N][M]; a = gate or logit gradients, a.t in place
// where km is off.  km: both operands as they lie in memory (kl_launch_gemm_an, the hardware transpose read), no transposed copies;
// else over the transposed copies, x's as a scan (or kl_launch_onehot_*) wrote it or made here by an explicit transpose
static int rows_product(const TrainCall& c, bool km, const RowsOperand& a, int M, const RowsOperand& x, int N, float* out, long ldc, bool out_t) {
  const bool onehot = x.km == nullptr;
  if (km) return kl_launch_gemm_an(a.km, onehot ? x.t : x.km, out, M, N, c.BT, a.ld, onehot ? x.ldt : x.ld, ldc, out_t ? 1 : 0, c.s, onehot ? 0 : 1);
  const bf16_t* xT = x.t;
  long ldx = x.ldt; int K = onehot ? c.BTp : c.BT;
  if (!xT) {
    KL_TRY(kl_launch_transpose_bf16(x.km, x.ld, c.w.HT, c.BTp, c.BT, N, c.s));
    xT = c.w.HT; ldx = c.BTp; K = c.BTp;
  }
  return out_t ? kl_launch_gemm_tn(xT, a.t, out, nullptr, N, M, K, ldx, a.ldt, ldc, 2, c.ksplit, 1.f, c.s)
               : kl_launch_gemm_tn(a.t, xT, out, nullptr, M, N, K, a.ldt, ldx, ldc, 2, c.ksplit, 1.f, c.s);
}

// the one-hot matrix [rows][BTp] of variable `var` of src's n_vars: dense where that applies, else zero + scatter; its product's sums [4W][rows] zeroed
static int onehot(const TrainCall& c, const int32_t* src, int classes, int rows, int var, int n_vars, bf16_t* out, float* sums) {
  if (kl_launch_onehot_dense(src, c.B, c.T, rows, var, n_vars, out, c.BTp, c.s) == KL_ERR_SHAPE) {
    KL_TRY(kl_zero_async(out, (size_t)rows * c.BTp * sizeof(bf16_t), c.s));
    KL_TRY(kl_launch_onehot_t(src, c.B, c.T, classes, var, n_vars, out, c.BTp, c.s));
  }
  return kl_zero_async(sums, (size_t)4 * c.W * rows * sizeof(float), c.s);
}

// F5/F6 + B1, the output layer: logits over the (masked) top-layer outputs, softmax, CE, dlogits; dH = dlogits . E; dE += dlogits^T . Htop
static int train_output_layer(const TrainCall& c) {
  kl_handle* h = c.h; WindowWs& w = c.w; const Derived& d = h->d; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W, V = c.V, Vp = c.Vp, BT = c.BT, BTp = c.BTp;
  const RowsOperand top = layer_out(c, c.L - 1);
  // (one kernel where it applies -- V = 256, width 512: the logits never reach memory --, else GEMM + softmax)
  int fe = KL_ERR_SHAPE;
  if (h->logits_ws && c.loss_acc != nullptr && w.rowstat != nullptr && V == Vp)
    fe = kl_launch_logits_ce_ws(top.km, d.E_hi, c.tgt, w.dlogits, w.rowstat, B, T, W, V, Vp, c.inv_count, h->last_only, s);
  // (width 128: ... and dH = dlogits . E in the same pass -- lstm_scan_w128.hip; the scans there take dH as f32 rows)
  bool dh_done = false;
  if (fe == KL_ERR_SHAPE && h->logits_ws && W == 128 && c.loss_acc != nullptr && w.rowstat != nullptr && !w.scan2_bwd) {
    fe = kl_launch_logits_ce_w128(top.km, d.E_hi, d.ET, c.tgt, w.dlogits, w.dH, w.rowstat, B, T, W, V, Vp, c.inv_count, h->last_only, s);
    dh_done = fe == 0;
  }
  if (fe != 0 && fe != KL_ERR_SHAPE) return fe;
  if (fe == 0) c.note.out_route |= dh_done ? KL_OUT_LOGITS_W128 : KL_OUT_LOGITS_WS;
  if (fe == 0) KL_TRY(kl_launch_rowstat_reduce(w.rowstat, BT, c.loss_acc, s));
  else {
    KL_TRY(kl_launch_gemm_tn(top.km, d.E_hi, w.logits, nullptr, BT, V, W, W, W, V, 0, 1, 1.f, s));
    KL_TRY(kl_launch_softmax_ce(w.logits, V, BT, V, c.tgt, B, T, c.inv_count, w.dlogits, Vp, c.loss_acc, w.rowstat, 1, s, h->last_only));
  }
  // B1: dH = dlogits . E ; dE += dlogits^T . Htop
  int de = KL_ERR_SHAPE;
  if (c.dh_mode == 1 && h->logits_ws) de = kl_launch_dh_ws(w.dlogits, d.ET, reinterpret_cast<bf16_t*>(w.dH), BT, W, Vp, s);
  if (de == 0) c.note.out_route |= KL_OUT_DH_WS;
  if (dh_done) de = 0;
  if (de == KL_ERR_SHAPE) de = kl_launch_gemm_tn(w.dlogits, d.ET, w.dH, nullptr, BT, W, Vp, Vp, Vp, W, c.dh_mode, 1, 1.f, s);
  KL_TRY(de);
  if (BTp != BT) {
    KL_TRY(kl_zero_async(w.dlogitsT, (size_t)Vp * BTp * sizeof(bf16_t), s));
    KL_TRY(kl_zero_async(w.HT, (size_t)W * BTp * sizeof(bf16_t), s));
    KL_TRY(kl_zero_async(w.dZT, (size_t)4 * W * BTp * sizeof(bf16_t), s));
  }
  // (dE with both operands as they lie in memory: the window's plan, and the vocabulary unpadded)
  const bool km_e = w.km_plan && Vp == V && kl_gemm_an_applicable(V, W, BT, Vp);
  if (km_e) c.note.out_route |= KL_OUT_DE_KMAJOR;
  if (!km_e) KL_TRY(kl_launch_transpose_bf16(w.dlogits, Vp, w.dlogitsT, BTp, BT, Vp, s));
  return rows_product(c, km_e, {w.dlogits, Vp, w.dlogitsT, BTp}, V, top, W, c.grads + h->off_E, W, false);
}

// B5, layer 0 through the look-up tables: dEK^T = dZ_0^T . OneHot ; dCtxK_n^T likewise; from them dK_0, dE and the context tables
static int table_grads(const TrainCall& c) {
  kl_handle* h = c.h; WindowWs& w = c.w; const kl_config& cf = h->cfg; const Derived& d = h->d; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W, V = c.V, Vp = c.Vp, BT = c.BT, BTp = c.BTp;
  const bool km = w.km_plan, seg = w.segsum;
  const RowsOperand dz = {w.dZ[0], 4 * W, w.dZT, BTp};
  // (segment sums: the characters' and the first context variable's sums from ONE read of dZ's rows in key order, no
  //  one-hot matrices and no multiplications -- the tables come out row-major, dEK [Vp][4W] and dCtxK_0 [ctx_vocab][4W])
  bool pair_ctx = false;
  if (seg) {
    KL_TRY(kl_launch_segment_sums(w.dZ[0], 4 * W, B, T, 4 * W, c.idx, c.ctx, cf.n_ctx, Vp, cf.ctx_vocab, w.dEKT,
                                  cf.n_ctx > 0 ? w.dCtxKT[0] : nullptr, w.seg_ws, s));
    KL_TRY(kl_launch_f32_to_bf16_t(w.dEKT, 4 * W, Vp, 4 * W, w.dEKT_bf, nullptr, Vp, 1, s));
    KL_TRY(kl_launch_f32_to_bf16_t(w.dEKT, 4 * W, Vp, 4 * W, w.dEK_bf, nullptr, 4 * W, 0, s));
  } else {
    KL_TRY(onehot(c, c.idx, V, Vp, 0, 1, w.OHT, w.dEKT));
    // (the first context variable's one-hot product rides along with the characters': one pass over dZ for both)
    pair_ctx = km && h->fuse_wg && cf.n_ctx >= 1 && (Vp % 128) == 0 && kl_gemm_an_applicable(4 * W, Vp + cf.ctx_vocab, BT, 4 * W);
    if (pair_ctx) {
      KL_TRY(onehot(c, c.ctx, cf.ctx_vocab, cf.ctx_vocab, 0, cf.n_ctx, w.OHC[0], w.dCtxKT[0]));
      const int pe = kl_launch_gemm_an2(w.dZ[0], w.OHT, w.dEKT, 4 * W, Vp, BT, 4 * W, BTp, Vp, 0,
                                        w.OHC[0], w.dCtxKT[0], cf.ctx_vocab, BTp, cf.ctx_vocab, 0, s, 0);
      if (pe == KL_ERR_SHAPE) pair_ctx = false;      // (nothing was launched: both products follow one by one)
      else KL_TRY(pe);
    }
    // (a one-hot matrix only has the transposed form: K-major dZ against it, or dZ^T)
    if (!pair_ctx) KL_TRY(rows_product(c, km, dz, 4 * W, {nullptr, 0, w.OHT, BTp}, Vp, w.dEKT, Vp, false));
    KL_TRY(kl_launch_f32_to_bf16_t(w.dEKT, Vp, 4 * W, Vp, w.dEKT_bf, nullptr, Vp, 0, s));
    KL_TRY(kl_launch_f32_to_bf16_t(w.dEKT, Vp, 4 * W, Vp, w.dEK_bf, nullptr, 4 * W, 1, s));
  }
  c.note.wg_route |= (seg ? KL_WG_SEGSUM : 0) | (pair_ctx ? KL_WG_PAIR_CTX : 0);
  // dK0[:W] = E^T . dEK      (C[W][4W] = ET[W][Vp] . dEKT[4W][Vp]^T)
  KL_TRY(kl_launch_gemm_tn(d.ET, w.dEKT_bf, c.grads + h->off_K[0], nullptr, W, 4 * W, Vp, Vp, Vp, 4 * W, 0, 1, 1.f, s));
  // dE += dEK . K0[:W]^T     (C[V][W] = dEK[V][4W] . Kn0[W][4W]^T)
  KL_TRY(kl_launch_gemm_tn(w.dEK_bf, d.Kn[0], c.grads + h->off_E, nullptr, V, W, 4 * W, 4 * W, 4 * W, W, 2, 1, 1.f, s));
  for (int n = 0; n < cf.n_ctx; ++n) {
    const bool seg_n = seg && n == 0;      // (its sums are there already, row-major)
    if (!(pair_ctx && n == 0) && !seg_n) {
      KL_TRY(onehot(c, c.ctx, cf.ctx_vocab, cf.ctx_vocab, n, cf.n_ctx, w.OHC[n], w.dCtxKT[n]));
      KL_TRY(rows_product(c, km, dz, 4 * W, {nullptr, 0, w.OHC[n], BTp}, cf.ctx_vocab, w.dCtxKT[n], cf.ctx_vocab, false));
    }
    const size_t krow = (size_t)(W + n * cf.ctx_dim) * 4 * W;
    KL_TRY(kl_launch_ctx_grads(h->params + h->off_Ctx[n], h->params + h->off_K[0] + krow, 4 * W, cf.ctx_vocab, cf.ctx_dim,
                               w.dCtxKT[n], seg_n ? 1 : cf.ctx_vocab, 4 * W, c.grads + h->off_K[0] + krow, 4 * W,
                               c.grads + h->off_Ctx[n], s, seg_n ? 4 * W : 1));
  }
  return 0;
}

// B4/B5: weight gradients of layer l, contractions over the B*T rows of its dZ (rows_product: K-major where the window's plan
// says so, w.km_plan).  dzt_ready: the scan wrote dZ^T; db_done: ... and summed db
static int weight_grads(const TrainCall& c, int l, bool dzt_ready, bool db_done) {
  kl_handle* h = c.h; WindowWs& w = c.w; hipStream_t s = c.s;
  const int W = c.W, BT = c.BT; const bool km = w.km_plan;
  if (!dzt_ready && !km) KL_TRY(kl_launch_transpose_bf16(w.dZ[l], 4 * W, w.dZT, c.BTp, BT, 4 * W, s));
  // dU_l = Hprev^T . dZ   (Hprev = H blocks 0..T-1); dK_l = X^T . dZ with X = (masked) outputs of layer l-1
  const RowsOperand dz = {w.dZ[l], 4 * W, w.dZT, c.BTp}, Hprev = {(const bf16_t*)w.H[l], W, w.ht_ready ? w.HTf[l] : nullptr, c.ldtf};
  // (K-major: every product over the layer's dZ rows in as few passes over them as possible -- KlGemmSecond, gemm.hip)
  // (a pair has twice the column tiles of a single product; where the launcher does not take it -- KL_ERR_SHAPE -- the
  //  products go out one by one, as km_plan has checked they can)
  bool pair_uk = km && l > 0 && h->fuse_wg && (W % 128) == 0 && kl_gemm_an_applicable(4 * W, 2 * W, BT, 4 * W);
  if (pair_uk) {
    const int pe = kl_launch_gemm_an2(w.dZ[l], Hprev.km, c.grads + h->off_U[l], 4 * W, W, BT, 4 * W, W, 4 * W, 1,
                                      layer_out(c, l - 1).km, c.grads + h->off_K[l], W, W, 4 * W, 1, s, 1);
    if (pe == KL_ERR_SHAPE) pair_uk = false;      // (nothing was launched)
    else KL_TRY(pe);
  }
  c.note.wg_route |= km ? KL_WG_KMAJOR : (w.ht_ready ? KL_WG_SCAN_T : KL_WG_TRANSPOSE);
  if (pair_uk) c.note.wg_pair_mask |= 1u << l;
  if (db_done) c.note.wg_db_scan_mask |= 1u << l;
  if (!pair_uk) KL_TRY(rows_product(c, km, dz, 4 * W, Hprev, W, c.grads + h->off_U[l], 4 * W, true));
  if (!db_done) KL_TRY(kl_launch_colsum_bf16(w.dZ[l], 4 * W, BT, 4 * W, c.grads + h->off_b[l], s));   // (the wide backward scan sums db itself)
  if (l == 0) return table_grads(c);
  if (!pair_uk) KL_TRY(rows_product(c, km, dz, 4 * W, layer_out(c, l - 1), W, c.grads + h->off_K[l], 4 * W, true));
  return 0;
}

// what all backward scans are told alike, for layers [first, first + n) as the scan's 0 .. n - 1 (the callers add Kn, hand-off and bias sums)
static KlScanBwd bwd_scan_args(const TrainCall& c, int first, int n) {
  const Derived& d = c.h->d;
  KlScanBwd a;
  memset(&a, 0, sizeof(a));
  a.B = c.B; a.T = c.T; a.W = c.W; a.L = n;
  for (int j = 0; j < n; ++j) {
    const int l = first + j;
    a.Un[j] = d.Un[l]; a.G[j] = c.w.G[l]; a.C[j] = c.w.C[l]; a.dZ[j] = c.w.dZ[l];
    a.mask[j] = (c.masks != nullptr && l > 0) ? c.masks + (size_t)l * c.BW : nullptr;
  }
  a.dH = c.w.dH; a.status = c.w.scan_status + 1;
  return a;
}

// What layer l's scan hands over from: the dZ rows it is going to publish as sentinels -- all steps, or only the last two (rolling: the
// scan re-arms step t - 2 while it publishes step t) -- or, for a scan that counts, one layer's counters at zero
static int arm_dz(const TrainCall& c, int l, ArmMode mode) {
  const size_t T = c.T, BW = c.BW;
  if (mode == ARM_COUNTERS) return kl_zero_coherent_async(c.w.scan_cnt, (size_t)((c.B + 15) / 16) * T, c.s);
  const size_t first = mode == ARM_ROLLING ? (T - 2) * BW * 4 : 0, steps = mode == ARM_ROLLING ? 2 : T;
  return kl_fill_u32_async(c.w.dZ[l] + first, steps * BW * 4 * sizeof(bf16_t), 0xFFFFFFFFu, c.s);
}

// a whole-window backward scan went out: what the per-launch timing reports about it
static void trace_bwd_scan(const TrainCall& c, const char* kernel, double flops) {
  c.h->trace_persistent[1] = true; c.h->trace_name[1] = kernel; c.h->trace_flops[1] = flops;
  c.h->trace_end(1, c.s);
}

// Width 128, all layers' workgroups fitting the CUs at once: ONE launch, a layer following the one above it a step behind (it
// polls the dZ rows that one publishes, which therefore start out as sentinels), then every layer's weight gradients.
static int bwd_w128_multi(const TrainCall& c) {
  kl_handle* h = c.h;
  const int B = c.B, T = c.T, W = c.W, L = c.L;
  if (!(c.seq128 && h->w128_fuse && h->w128_multi && kl_scan_w128_multi_fits(B, L))) return TRAIN_PASS;
  KlScanBwd a = bwd_scan_args(c, 0, L);
  for (int l = 0; l < L; ++l) { a.Kn[l] = h->d.Kn[l]; a.db_l[l] = c.grads + h->off_b[l]; }
  const bool roll = h->sentinel_roll && T >= 3;      // (rolling sentinels: only the last two steps start out armed)
  a.sentinel = roll ? 2 : 1;
  for (int l = 1; l < L; ++l) KL_TRY(arm_dz(c, l, roll ? ARM_ROLLING : ARM_ALL_STEPS));
  h->trace_begin(1, c.s);
  const int e = kl_launch_scan_bwd_w128_multi(a, c.s);
  if (e != 0) return e == KL_ERR_SHAPE ? TRAIN_PASS : e;
  trace_bwd_scan(c, "lstm_scan_bwd_w128_multi_kernel", (double)(2 * L - 1) * B * T * (2.0 * W * 4.0 * W));      // (recurrent contractions + the from-above ones)
  for (int l = L - 1; l >= 0; --l) KL_TRY(weight_grads(c, l, false, true));
  return 0;
}

enum BwdKernel { BWD_REGTILE, BWD_WIDE2, BWD_WIDE, BWD_W128, BWD_W32, BWD_THIN };
static const char* const BWD_KERNEL_NAME[] = {"lstm_scan_bwd_regtile_kernel", "lstm_scan_bwd_wide2_kernel", "lstm_scan_bwd_wide_kernel",
                                              "lstm_scan_bwd_w128_kernel",    "lstm_scan_bwd_w32_kernel",   "lstm_scan_bwd_kernel"};

// one layer's scan on the first kernel that takes it (*ran), `a` adjusted to what that kernel is told: register-tile or wide2, else wide, w128, w32, thin
static int launch_layer_scan(const TrainCall& c, int l, KlScanBwd& a, bool rt, bool fuse_dx, BwdKernel* ran) {
  kl_handle* h = c.h; WindowWs& w = c.w; hipStream_t s = c.s;
  if (w.scan2_bwd) {
    *ran = rt ? BWD_REGTILE : BWD_WIDE2;
    return rt ? kl_launch_scan_bwd_regtile(a, s) : kl_launch_scan_bwd_wide2(a, s);      // (KL_ERR_SHAPE: an error, planned together -- plan_scan2)
  }
  *ran = BWD_WIDE;
  int e = h->wide_bwd ? kl_launch_scan_bwd_wide(a, s) : KL_ERR_SHAPE;
  if (e == KL_ERR_SHAPE && c.seq128) {
    KlScanBwd a1 = a;
    a1.dZT = nullptr; a1.sentinel = 0;
    if (fuse_dx) { a1.Kn[1] = h->d.Kn[l + 1]; a1.dZ[1] = w.dZ[l + 1]; }
    *ran = BWD_W128; e = kl_launch_scan_bwd_w128(a1, s);
    if (e == KL_ERR_SHAPE && fuse_dx) return KL_ERR_SHAPE;      // (the dX product was skipped for it)
    if (e == 0) a.dZT = nullptr;
  }
  if (e == KL_ERR_SHAPE && h->w32 && (c.B + 15) / 16 >= h->w32_min_rb && kl_scan_w32_applicable(c.B, c.T, c.W)) {
    // width 1024: eight-wave workgroups of 32 units (lstm_scan_w32.hip); every step starts out as sentinels
    if (a.sentinel != 1) KL_TRY(arm_dz(c, l, ARM_ALL_STEPS));
    a.sentinel = 1; a.dZT = nullptr;
    a.xcc_slots = h->w32_local ? w.scan_status + 4 : nullptr;
    *ran = BWD_W32; e = kl_launch_scan_bwd_w32(a, s);
  }
  if (e == KL_ERR_SHAPE) {
    a.dZT = nullptr; a.db = nullptr;
    if (a.sentinel) KL_TRY(arm_dz(c, l, ARM_COUNTERS));   // (the thin scan counts)
    *ran = BWD_THIN; e = kl_launch_scan_bwd(a, s);
  }
  return e;
}

// Layer by layer, from the top: where the plan says so (many row blocks, width 1024, deeper than the fused scan's four layers, width 128)
// and always behind second-generation forward scans.  Per layer: the from-above term for all steps, the hand-off armed, the scan, the
// layer's weight gradients
static int bwd_layer_by_layer(const TrainCall& c) {
  kl_handle* h = c.h; WindowWs& w = c.w; const Derived& d = h->d; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W, L = c.L, BT = c.BT, BTp = c.BTp;
  if (!(c.sequential || w.scan2_bwd)) return TRAIN_PASS;
  for (int l = L - 1; l >= 0; --l) {
    // (width 128: the scan of lstm_scan_w128.hip contracts the layer above's dZ rows itself)
    const bool fuse_dx = c.seq128 && h->w128_fuse && l < L - 1;
    if (l < L - 1 && !fuse_dx)   // dX_l = dZ_{l+1} . K_{l+1}^T  -> w.dH (free once the layer above has been scanned)
      KL_TRY(kl_launch_gemm_tn(w.dZ[l + 1], d.Kn[l + 1], w.dH, nullptr, BT, W, 4 * W, 4 * W, 4 * W, W, c.dh_mode, 1, 1.f, s));
    KlScanBwd a = bwd_scan_args(c, l, 1);
    a.dHb = reinterpret_cast<const bf16_t*>(w.dH); a.counters = w.scan_cnt;
    a.Cb = (w.scan2_bwd && h->scan2_bf16) ? w.Cb[l] : nullptr;
    // (sentinels pay with several row blocks per workgroup, where the next tile is prefetched; with one
    // block the cheap counter poll beats re-fetching 64 KiB tiles; XCD-local publishes measured slower here)
    a.sentinel = (w.scan2_bwd || (h->sentinel_bwd && c.wide_fits && (kl_scan_wide_blocks_per_wg(B, W) > 1 || h->sentinel_bwd_all))) ? 1 : 0;
    // (measured at B = 1024 .. 3072: the request behind the MFMA phase is the best or tied everywhere; at the top of the block
    //  one tile in ten is requested before it is published, and the re-fetch costs more than the earlier request saves)
    a.pf_mode = h->scan2_pfb >= 0 ? h->scan2_pfb : 1;
    a.xcc_slots = (a.sentinel && h->xcd_local_bwd) ? w.scan_status + 4 : nullptr;
    a.gen = (unsigned)(1 + L + l);
    const int np_b = w.scan2_bwd ? kl_scan_wide2_phases(B, T, W, 16, 6) : 0;
    const bool by_flags = w.scan2_bwd && h->scan2_flags && h->flags_zeroed && np_b >= 3;
    // (from five blocks per step: eight waves, the tile through registers two blocks ahead -- lstm_scan_bwd_regtile_kernel)
    const bool rt = by_flags && h->regtile && h->scan2_bf16 && np_b >= kl_scan_bwd_regtile_min_np();
    if (by_flags) {
      // hand-off by flags (lstm_scan_bwd_wide2_kernel): nothing to arm, the epoch moves on
      a.flags = d.scan_flags; a.epoch = d.scan_flags + KL_SCAN_FLAGS;
      // (flags tell before the request whether a tile is there, so it can be asked for TWO blocks ahead, behind the epilogue,
      //  without the re-fetches that cost the sentinel form -- once five or more blocks lie between a publish and its use)
      if (h->scan2_pfb < 0) a.pf_mode = np_b >= 5 ? 2 : 1;
      else if (a.pf_mode == 0) a.pf_mode = 1;
      KL_TRY(kl_launch_scan_epoch(d.scan_flags, KL_SCAN_FLAGS, d.scan_flags + KL_SCAN_FLAGS, (unsigned)T + 2u, s));
    } else if (a.sentinel && h->sentinel_roll && T >= 3) {
      a.sentinel = 2;      // rolling sentinels: only the last two steps start armed
      KL_TRY(arm_dz(c, l, ARM_ROLLING));
    } else {      // hand-off by data: the steps the scan is going to publish start out as sentinels; else by counters
      KL_TRY(arm_dz(c, l, a.sentinel ? ARM_ALL_STEPS : ARM_COUNTERS));
    }
    h->trace_begin(1, s);
    // wide (64-unit) workgroups share the dZ tile through LDS; the weight-gradient GEMMs read dZ K-major
    // as it is (km_plan), else the scan also writes dZ^T
    a.dZT = (!w.km_plan && BTp == BT && (B & 7) == 0) ? w.dZT : nullptr;
    a.ldt = BTp; a.db = c.grads + h->off_b[l];
    if (rt) a.xcc_slots = h->rt_local ? w.scan_status + 4 : nullptr;
    BwdKernel ran;
    KL_TRY(launch_layer_scan(c, l, a, rt, fuse_dx, &ran));
    trace_bwd_scan(c, BWD_KERNEL_NAME[ran], (double)B * T * (2.0 * W * 4.0 * W));   // one layer's recurrent contraction
    // dZ^T lives in ONE buffer: this layer's weight gradients before the next layer's scan
    // (every kernel but the thin one sums db; the wide ones also write dZ^T where a.dZT is left set)
    KL_TRY(weight_grads(c, l, a.dZT != nullptr, ran != BWD_THIN));
  }
  return 0;
}

// the fused thin scan: all layers (at most KL_SCAN_MAXL) in one launch, hand-off by counters
static int bwd_fused_thin(const TrainCall& c) {
  kl_handle* h = c.h;
  const int B = c.B, T = c.T, W = c.W, L = c.L;
  if (!(h->scan_enabled && L <= KL_SCAN_MAXL)) return TRAIN_PASS;
  KlScanBwd a = bwd_scan_args(c, 0, L);
  a.counters = c.w.scan_cnt;
  for (int l = 0; l < L; ++l) a.Kn[l] = h->d.Kn[l];
  KL_TRY(kl_zero_coherent_async(c.w.scan_cnt, (size_t)L * ((B + 15) / 16) * T, c.s));      // (all layers' counters)
  h->trace_begin(1, c.s);
  const int e = kl_launch_scan_bwd(a, c.s);
  if (e != 0) return e == KL_ERR_SHAPE ? TRAIN_PASS : e;
  trace_bwd_scan(c, "lstm_scan_bwd_kernel", (double)B * T * (2.0 * (2.0 * L - 1.0) * W * 4.0 * W));
  return 0;
}

// everything else: the launch-per-step layer wavefront (diagonal dgl: layer l runs step T - 1 - (dgl - (L - 1 - l)))
static int bwd_wavefront(const TrainCall& c) {
  kl_handle* h = c.h; WindowWs& w = c.w; const Derived& d = h->d; hipStream_t s = c.s;
  const int B = c.B, T = c.T, W = c.W, L = c.L;
  const size_t BW = c.BW; const float* masks = c.masks;
  for (int dgl = 0; dgl < T + L - 1; ++dgl) {
    KlBwdStep steps[16];     // one per layer (config_ok: depth <= 16); launched in packs of 4 below
    int ns = 0;
    for (int j = 0; j < L; ++j) {
      const int l = L - 1 - j;
      const int t = T - 1 - (dgl - j);
      if (t < 0 || t >= T) continue;
      KlBwdStep& S = steps[ns++];
      memset(&S, 0, sizeof(S));
      S.n_rows = B; S.W = W;
      int p = 0;
      if (l < L - 1) {   // gradient from the layer above: dZ_{l+1}[t] . K_{l+1}^T
        KlOperand& o = S.op[p++];
        o.A = w.dZ[l + 1] + (size_t)t * B * 4 * W; o.lda = 4 * W; o.a_is_f32 = 0;
        o.WT_hi = d.Kn[l + 1]; o.ldw = 4 * W; o.K = 4 * W;
        if (masks != nullptr && l > 0) { S.op0_mask = masks + (size_t)l * BW; S.op0_mask_ld = W; }
      } else {
        S.dh_in = w.dH + (size_t)t * BW; S.dh_in_ld = W;
        if (c.top_masked) { S.dh_mask = masks + (size_t)l * BW; S.dh_mask_ld = W; }
      }
      if (t < T - 1) {   // recurrent: dZ_l[t+1] . U_l^T
        KlOperand& o = S.op[p++];
        o.A = w.dZ[l] + (size_t)(t + 1) * B * 4 * W; o.lda = 4 * W; o.a_is_f32 = 0;
        o.WT_hi = d.Un[l]; o.ldw = 4 * W; o.K = 4 * W;
        // an op0 mask must only scale the from-above contribution: keep that one first
      }
      S.n_ops = p;
      if (S.op0_mask && !(l < L - 1)) S.op0_mask = nullptr;
      S.gates = w.G[l] + (size_t)t * B * 4 * W; S.gates_ld = 4 * W;
      S.c = w.C[l] + (size_t)(t + 1) * BW; S.c_ld = W;
      S.c_prev = w.C[l] + (size_t)t * BW; S.c_prev_ld = W;
      float* dc_rd = (t & 1) ? w.dc1[l] : w.dc0[l];
      float* dc_wr = (t & 1) ? w.dc0[l] : w.dc1[l];
      if (t < T - 1) { S.dc_in = dc_rd; S.dc_in_ld = W; }
      S.dc_out = dc_wr; S.dc_out_ld = W;
      S.dz_out = w.dZ[l] + (size_t)t * B * 4 * W; S.dz_ld = 4 * W;
    }
    for (int i = 0; i < ns; i += 4) {
      const bool steady = (ns == L) && dgl >= L && dgl + 8 < T;
      if (steady && dgl % 8 == 0) h->trace_begin(1, s);
      KL_TRY(kl_launch_bwd_steps(steps + i, ns - i < 4 ? ns - i : 4, s));
      if (steady && dgl % 8 == 7) h->trace_end(1, s);
    }
  }
  return 0;
}

static int train_window_body(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                    float* states, const float* masks, float* grads, float* loss_acc, void* ws, size_t ws_bytes,
                    void* stream) {
  hipStream_t s = (hipStream_t)stream;      // (kl_train_window has checked the arguments)
  WindowWs w;
  if (ws_bytes < carve_window(h, ws, B, T, 1, &w)) return KL_ERR_WORKSPACE;
  const kl_config& cf = h->cfg;
  const int W = cf.width, V = cf.voc_size, Vp = h->Vp, L = cf.depth;
  const int BT = B * T, BTp = round_up_i(BT, 8);
  const float* P = h->params;
  KL_TRY(kl_zero_async(grads, h->n_params * sizeof(float), s));
  KL_TRY(kl_zero_async(w.scan_status, (4 + 256) * sizeof(unsigned), s));
  // (M = 4W rows of dZ as the K-major A operand: W % 64 == 0, T*B % 64 == 0)
  w.km_plan = h->gemm_an && BTp == BT && kl_gemm_an_applicable(4 * W, W, BT, 4 * W);
  w.scan2_rows = plan_scan2(h, B, T, w.km_plan, true);
  w.scan2_bwd = w.scan2_rows != 0;
  KL_TRY(forward_impl(h, B, T, idx, ctx, states, masks, 1, w, s));
  // Many row blocks (B >= 256 at cfg2): the fused two-layer scan is bound by every
  // workgroup re-reading its 16 x 4W dZ tile for BOTH contractions.  Run the layers one
  // after the other instead -- each scan then only carries the recurrent contraction and
  // twice the row groups fit -- and take the from-above term dZ_{l+1} . K_{l+1}^T for all
  // steps at once from the big GEMM.
  const int n_rb_all = (B + 15) / 16, nug = W / 16;
  const bool thin_fits = (n_rb_all + 512 / nug - 1) / (512 / nug) <= (W == 1024 ? 8 : 4) &&
                         (long)T * B * 4 * W * 2 <= 0xfffffff0L;      // (the scans address dZ with unsigned 32-bit offsets)
  const bool wide_fits = h->wide_bwd && kl_scan_bwd_wide_applicable(B, T, W) && BTp == BT && (B & 7) == 0;
  // (width 1024 has no fused scan at all: always layer by layer)
  // (... and deeper than four layers: the fused scan's limit)
  // (width 128: the one-layer scans of lstm_scan_w128.hip, a workgroup per 16-row block with all units)
  const bool seq128 = h->scan_enabled && h->seq_bwd && h->w128 && B >= h->w128_min && kl_scan_w128_applicable(B, T, W) && !w.scan2_bwd;
  const bool sequential = seq128 || (h->scan_enabled && h->seq_bwd &&
                          ((L > 1 && L <= KL_SCAN_MAXL && (W == 512 || W == 256 || W == 128) && n_rb_all > 512 / (L * nug)) ||
                           W == 1024 || (L > KL_SCAN_MAXL && (W == 512 || W == 256 || W == 128 || W == 64))) &&
                          (thin_fits || wide_fits));
  const int mean_rows = (h->loss_rows > 0 && h->loss_rows <= B) ? h->loss_rows : B;      // (a padded batch: the real streams)
  const TrainCall c = {h, B, T, idx, ctx, tgt, masks, grads, loss_acc, s, w, *h->view_note(B, T, ws, true), W, V, Vp, L, BT, BTp, (size_t)B * W,
                       /*ksplit*/ BT >= 4096 ? 8 : (BT >= 1024 ? 4 : 1), /*ldtf*/ (long)(T + 1) * B,
                       /*dh_mode*/ w.scan2_bwd ? 1 : 0,      // (second-generation backward scan: dH travels as bf16)
                       /*top_masked*/ masks != nullptr && L > 1,
                       /*inv_count*/ 1.0f / (h->last_only ? (float)mean_rows : (float)mean_rows * (float)T), wide_fits, seq128, sequential};
  c.note = kl_handle::ViewNote{B, T, ws, w.scan2_rows, w.scan2_bwd ? 1 : 0, (w.scan2_bwd && h->scan2_bf16) ? 1 : 0, w.scan2_bwd ? 1 : 0,
                               w.p_bf16_mask};
  c.note.hd_mask = masks != nullptr ? ((1u << L) - 1u) & ~1u : 0u;      // (forward_impl: every layer above the first writes Hd)
  KL_TRY(train_output_layer(c));
  // B3: reverse recurrence -- the first path that takes the window, in this order; the first two issue each layer's weight
  // gradients themselves (dZ^T lives in one buffer), the other two leave them all to the end
  int e = bwd_w128_multi(c);
  if (e == TRAIN_PASS) e = bwd_layer_by_layer(c);
  if (e == TRAIN_PASS) {
    e = bwd_fused_thin(c);
    if (e == TRAIN_PASS) e = bwd_wavefront(c);
    for (int l = L - 1; l >= 0 && e == 0; --l) e = weight_grads(c, l, false, false);
  }
  KL_TRY(e);
  // F7: embedding regularisers (training phase only)
  std::vector<const float*> ctabs(cf.n_ctx);
  std::vector<float*> gctabs(cf.n_ctx);
  for (int n = 0; n < cf.n_ctx; ++n) { ctabs[n] = P + h->off_Ctx[n]; gctabs[n] = grads + h->off_Ctx[n]; }
  KL_TRY(kl_launch_regulariser_grads(P + h->off_E, V, W, ctabs.data(), cf.n_ctx, cf.ctx_vocab, cf.ctx_dim,
                                     grads + h->off_E, gctabs.data(), loss_acc, w.reg_scratch, s));
  // a timed-out hand-off in a persistent scan surfaces as loss_acc[3] != 0
  hipLaunchKernelGGL(scan_status_kernel, dim3(1), dim3(64), 0, s, w.scan_status, loss_acc);
  return hip_ok(hipGetLastError());
}

int kl_adam_step_scaled(kl_handle* h, const float* grads, float grad_scale, float* m, float* v, int t, float lr, float b1,
                        float b2, float eps, float clip, void* stream) {
  if (!h || !grads || !m || !v || t < 1) return KL_ERR_ARG;
  if (!h->params) return KL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const double lr_t = (double)lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t));
  KL_TRY(kl_launch_adam(h->params, grads, m, v, h->n_params, (float)lr_t, b1, b2, eps, clip, grad_scale, s));
  return prepare_impl(h, h->precision ? h->precision : KL_PREC_BF16, s);
}

int kl_adam_step(kl_handle* h, const float* grads, float* m, float* v, int t, float lr, float b1, float b2,
                 float eps, float clip, void* stream) {
  return kl_adam_step_scaled(h, grads, 1.0f, m, v, t, lr, b1, b2, eps, clip, stream);
}

namespace {      // (its functions are `static` as well: inside extern "C" the namespace alone leaves their names exported)
struct StepWs {
  float* prow;           // P rows when n_ctx != 1
  float* z;              // z of the gather + GEMM path
  bf16_t* A3;            // ... its [hi | lo | hi] activation rows
  bf16_t* rows[16];      // ... of every layer at once (fused form; config_ok: depth <= 16)
  size_t bytes;
};
static StepWs step_carve(const kl_handle* h, int n, void* ws) {
  const size_t W = h->cfg.width;
  Carver cv(ws);
  StepWs w;
  w.prow = cv.take<float>((size_t)n * 4 * W);
  w.z = cv.take<float>((size_t)n * 4 * W);
  w.A3 = cv.take<bf16_t>((size_t)n * 3 * 2 * W);
  for (int l = 0; l < h->cfg.depth; ++l) w.rows[l] = cv.take<bf16_t>((size_t)n * 3 * (l == 0 ? 1 : 2) * W);
  w.bytes = align_up(cv.off, 256);
  return w;
}

// what is added to a layer's gate inputs: T1[i1 ? i1[row] : row] + T2[i2[row]] + bias (null: none)
struct GateSrc { const float* T1; const int32_t* i1; const float* T2; const int32_t* i2; const float* bias; };
static GateSrc gate_src(const kl_handle* h, int l, const float* prow, const int32_t* idx, const int32_t* ctx) {
  if (l > 0) return {nullptr, nullptr, nullptr, nullptr, h->params + h->off_b[l]};
  if (prow) return {prow, nullptr, nullptr, nullptr, nullptr};      // gathered rows: b_0 is folded in
  return {h->d.EK, idx, h->d.CtxK[0], ctx, h->params + h->off_b[0]};
}

// layer l of a step on step_tile.hip's / step_small.hip's kernels.  With the indices in the kernel arguments (KlHostIdx):
// null slot arrays, the device index block as idx and ctx (non-null = "table rows by index"; the values are KlHostIdx's)
static KlIncCellArgs inc_cell_args(const kl_handle* h, int l, int n, float* pool, const int32_t* slot_in, const int32_t* slot_out,
                                   const float* prow, const int32_t* idx, const int32_t* ctx) {
  const int W = h->cfg.width;
  const GateSrc g = gate_src(h, l, prow, idx, ctx);
  KlIncCellArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n; a.W = W; a.split = h->precision;
  a.pool = pool; a.slot_ld = (long)2 * h->cfg.depth * W; a.slot_in = slot_in; a.slot_out = slot_out;
  a.h_off = 2 * l * W; a.c_off = (2 * l + 1) * W; a.x_off = l > 0 ? 2 * (l - 1) * W : -1;
  a.UF = h->d.UF[l]; a.KF = h->d.KF[l];
  a.T1 = g.T1; a.i1 = g.i1; a.T2 = g.T2; a.i2 = g.i2; a.bias = g.bias;
  return a;
}

// the output layer: logits over the tied embedding from the top layer's new h (pool rows through `slots`) into out[n][V]
// by the thin GEMM, then (softmax) the softmax in place
static int output_thin(const kl_handle* h, int n, const float* pool, const int32_t* slots, float* out, bool softmax, hipStream_t s) {
  const Derived& d = h->d;
  const int W = h->cfg.width, L = h->cfg.depth, V = h->cfg.voc_size, split = h->precision;
  KlOperand op;
  memset(&op, 0, sizeof(op));
  op.A = pool + (size_t)2 * (L - 1) * W; op.lda = (long)2 * L * W; op.row_index = slots; op.a_is_f32 = 1;
  op.WT_hi = d.E_hi; op.WT_lo = split == 3 ? d.E_lo : nullptr; op.ldw = W; op.K = W;
  KL_TRY(kl_launch_thin_gemm(&op, n, V, out, V, nullptr, split, s));
  return softmax ? kl_launch_softmax_ce(out, V, n, V, nullptr, n, 1, 1.f, nullptr, 0, nullptr, nullptr, 0, s) : 0;
}

struct StepCall {        // a kl_step_batch call as its kernel paths see it
  kl_handle* h; int n; const int32_t *idx, *ctx; float* pool; const int32_t *slot_in, *slot_out; float* probs;
  const float* prow;     // layer 0's gathered gate inputs (n_ctx != 1); null: table rows by idx / ctx
  hipStream_t s;
};

// ---- the plan of a step: the kernels a call of n rows goes to.  kl_step_batch and kl_step_batch_host ask it before they
// launch anything, kl_test_step_route reports it; what a launcher does with a shape is its own plan function
// (kl_plan_inc_tile, kl_plan_inc_cell, kl_plan_out_softmax), which the launcher itself asks again.
struct StepPlan {
  int layers, out;              // KL_STEP_*, KL_STEP_OUT_* (keraslm_hip.h)
  KlIncTilePlan tile;           // KL_STEP_TILES
  KlIncCellPlan cell[16];       // KL_STEP_CELLS, per layer (config_ok: depth <= 16)
};

// inc_cell_kernel for every layer of the step?  (All layers are asked before the first is launched: where the layers above
// the first do not fit in LDS -- K = 2W there --, the step goes to another path whole.)
static bool plan_cells(const kl_handle* h, int n, bool host_idx, KlIncCellPlan* cell) {
  for (int l = 0; l < h->cfg.depth; ++l)
    if (!h->d.UF[l] || kl_plan_inc_cell(n, h->cfg.width, l > 0, host_idx, &cell[l]) != 0) return false;
  return true;
}

// The first path that takes the shape, in this order:
// tiles -- 256 hypotheses or more, widths of 256, 512, 768, ...: one launch per layer, tiles of 64 (128) hypotheses x 32 units
//   with the state rows read through the pool slots and the weights from the hi / lo arrays as they are (step_tile.hip)
//   (width 1024 already from 129 hypotheses: inc_cell_kernel cannot hold two row tiles of K = 2048 in LDS there, and with one
//    its W / 16 x n / 16 workgroups read every weight 16 times at 250 hypotheses -- 90 us per step against 51 on 64-row tiles);
// cells -- 16 hypotheses and more (the reference's callers feed at most 128 / 256 rows; also whatever the tile kernel does not
//   take: widths 64 and 128): coalesced state rows through LDS, 16-unit workgroups (step_small.hip);
// gemm -- 256 hypotheses or more and a workspace: gather + split -> one bf16 GEMM over the 3x contraction -> gates; fused
//   form: the cell is the GEMM's epilogue;
// thin -- everything else (fewer than 16 hypotheses, widths the kernels above do not take): a launch per layer of the thin
//   forward-step kernel.
// Behind tiles and cells the output layer is logits + softmax in one launch where that applies, else thin GEMM + softmax;
// behind the GEMMs the thin GEMM while V x W is small (n/32 x V/16 workgroups), else big tiles for the output projection too.
static StepPlan step_plan(const kl_handle* h, int n, bool has_ws) {
  const int W = h->cfg.width, L = h->cfg.depth, V = h->cfg.voc_size;
  const Derived& d = h->d;
  StepPlan p;
  memset(&p, 0, sizeof(p));
  if ((n >= KL_BIG_STEP_N || (W >= 1024 && n > 128)) && h->inc_tile && V < 1024 && d.EF && d.UF[0] &&
      kl_plan_inc_tile(n, W, h->tile_rows, &p.tile) == 0)
    p.layers = KL_STEP_TILES;
  else if (h->inc_small && n >= h->inc_small_min && (n < KL_BIG_STEP_N || V < 1024) && d.EF && plan_cells(h, n, false, p.cell))
    p.layers = KL_STEP_CELLS;
  if (p.layers) {
    const bool fused = h->out_fused && n >= h->out_fused_min && kl_plan_out_softmax(n, W, V, h->precision == 3, nullptr) == 0;
    p.out = fused ? KL_STEP_OUT_FUSED : KL_STEP_OUT_THIN;
    return p;
  }
  if (n >= KL_BIG_STEP_N && has_ws) {
    const int nb = h->precision == 3 ? 3 : 1;
    bool fusable = h->fused_step && (W & 31) == 0 && L <= KL_SCAN_MAXL && V < 1024;
    for (int l = 0; l < L && fusable; ++l) fusable = d.WTperm[l] != nullptr && ((nb * (l == 0 ? W : 2 * W)) % 64) == 0;
    p.layers = fusable ? KL_STEP_GEMM_FUSED : KL_STEP_GEMM_PLAIN;
    p.out = V < 1024 ? KL_STEP_OUT_THIN : KL_STEP_OUT_BIG;
    return p;
  }
  p.layers = KL_STEP_THIN;
  p.out = KL_STEP_OUT_THIN;
  return p;
}

// tiles / cells: a launch per layer of inc_tile_kernel / inc_cell_kernel, then the output layer
// (the plan has asked the launchers' own rules: a KL_ERR_SHAPE from one of them is an error here)
static int step_layers(const StepCall& c, const StepPlan& p) {
  kl_handle* h = c.h;
  const int W = h->cfg.width, L = h->cfg.depth, V = h->cfg.voc_size;
  if (!h->inc_ready) KL_TRY(prepare_incremental(h, c.s));
  for (int l = 0; l < L; ++l) {
    const KlIncCellArgs a = inc_cell_args(h, l, c.n, c.pool, c.slot_in, c.slot_out, c.prow, c.idx, c.ctx);
    KL_TRY(p.layers == KL_STEP_TILES ? kl_launch_inc_tile(a, h->tile_var, c.s, h->tile_rows) : kl_launch_inc_cell(a, c.s));
  }
  if (p.out == KL_STEP_OUT_FUSED)
    return kl_launch_out_softmax(c.pool, (long)2 * L * W, c.slot_out, 2 * (L - 1) * W, h->d.EF, h->precision, c.n, W, V, c.probs, V, c.s);
  return output_thin(h, c.n, c.pool, c.slot_out, c.probs, true, c.s);
}

// gemm: gather + split -> one bf16 GEMM over the 3x contraction -> gates
static int step_gemm(const StepCall& c, const StepPlan& p, void* ws) {
  kl_handle* h = c.h;
  const int n = c.n, W = h->cfg.width, L = h->cfg.depth, V = h->cfg.voc_size;
  hipStream_t s = c.s;
  if (!h->big_ready) KL_TRY(prepare_big_step(h, s));
  Derived& d = h->d;
  float* pool = c.pool;
  const long slot_ld = (long)2 * L * W;
  const StepWs w = step_carve(h, n, ws);
  const int nb = h->precision == 3 ? 3 : 1;
  // fused form: one gather of all layers' recurrent halves, then per layer ONE GEMM whose epilogue is the cell
  // (gates, c', h', and h' as the next layer's input rows)
  if (p.layers == KL_STEP_GEMM_FUSED) {
    KlGatherRec g;
    memset(&g, 0, sizeof(g));
    g.pool = pool; g.slot_ld = slot_ld; g.slot_in = c.slot_in; g.n = n; g.W = W; g.nb = nb;
    for (int l = 0; l < L; ++l) g.out[l] = w.rows[l];
    KL_TRY(kl_launch_gather_recurrent(g, L, s));
    for (int l = 0; l < L; ++l) {
      const int Kl = l == 0 ? W : 2 * W;
      const GateSrc src = gate_src(h, l, c.prow, c.idx, c.ctx);
      KlGateEpi e;
      memset(&e, 0, sizeof(e));
      e.W = W; e.T1 = src.T1; e.i1 = src.i1; e.T2 = src.T2; e.i2 = src.i2; e.bias = src.bias;
      e.c_prev = pool + (size_t)(2 * l + 1) * W; e.c_ld = slot_ld; e.slot_in = c.slot_in;
      e.c_out = pool + (size_t)(2 * l + 1) * W; e.h_out = pool + (size_t)2 * l * W; e.out_ld = slot_ld; e.slot_out = c.slot_out;
      if (l + 1 < L) { e.xn = g.out[l + 1]; e.ldn = 3L * 2 * W; e.kn = 2 * W; e.nbn = nb; }
      KL_TRY(kl_launch_gemm_gates(g.out[l], d.WTperm[l], n, W, nb * Kl, 3L * Kl, &e, s));
    }
    return output_thin(h, n, pool, c.slot_out, c.probs, true, s);
  }
  for (int l = 0; l < L; ++l) {
    const int Kl = l == 0 ? W : 2 * W;
    if (l == 0) {
      KL_TRY(kl_launch_split_gather(pool, slot_ld, c.slot_in, W, nullptr, 0, nullptr, 0, n, nb, w.A3, 3L * Kl, s));
    } else {
      KL_TRY(kl_launch_split_gather(pool + (size_t)2 * (l - 1) * W, slot_ld, c.slot_out, W, pool + (size_t)2 * l * W, slot_ld,
                                    c.slot_in, W, n, nb, w.A3, 3L * Kl, s));
    }
    KL_TRY(kl_launch_gemm_tn(w.A3, d.WTcat[l], w.z, nullptr, n, 4 * W, nb * Kl, 3L * Kl, 3L * Kl, 4 * W, 0, 1, 1.f, s));
    const GateSrc src = gate_src(h, l, c.prow, c.idx, c.ctx);
    KL_TRY(kl_launch_gates_rows(w.z, 4 * W, n, W, src.T1, src.i1, src.T2, src.i2, src.bias, pool + (size_t)(2 * l + 1) * W, slot_ld,
                                c.slot_in, pool + (size_t)(2 * l + 1) * W, pool + (size_t)2 * l * W, slot_ld, c.slot_out, s));
  }
  if (p.out == KL_STEP_OUT_THIN) return output_thin(h, n, pool, c.slot_out, c.probs, true, s);      // V x W is small: n/32 x V/16 workgroups
  // wide vocabulary: big tiles pay off for the output projection too
  KL_TRY(kl_launch_split_gather(pool + (size_t)2 * (L - 1) * W, slot_ld, c.slot_out, W, nullptr, 0, nullptr, 0, n, nb, w.A3, 3L * W, s));
  KL_TRY(kl_launch_gemm_tn(w.A3, d.Ecat, c.probs, nullptr, n, V, nb * W, 3L * W, 3L * W, V, 0, 1, 1.f, s));
  return kl_launch_softmax_ce(c.probs, V, n, V, nullptr, n, 1, 1.f, nullptr, 0, nullptr, nullptr, 0, s);
}

// thin: a launch per layer of the thin forward-step kernel
static int step_thin(const StepCall& c) {
  kl_handle* h = c.h;
  const int n = c.n, W = h->cfg.width, L = h->cfg.depth, split = h->precision;
  const long slot_ld = (long)2 * L * W;
  Derived& d = h->d;
  float* pool = c.pool;
  for (int l = 0; l < L; ++l) {
    const GateSrc src = gate_src(h, l, c.prow, c.idx, c.ctx);
    KlFwdStep S;
    memset(&S, 0, sizeof(S));
    S.n_rows = n; S.W = W; S.split = split;
    S.T1 = src.T1; S.i1 = src.i1; S.t1_ld = src.T1 ? 4 * W : 0;
    S.T2 = src.T2; S.i2 = src.i2; S.t2_ld = src.T2 ? 4 * W : 0;
    S.bias = src.bias;
    int p = 0;
    if (l > 0) {      // the layer below's new h . K^T
      KlOperand& o = S.op[p++];
      o.A = pool + (size_t)2 * (l - 1) * W; o.lda = slot_ld; o.row_index = c.slot_out; o.a_is_f32 = 1;
      o.WT_hi = d.KT_hi[l]; o.WT_lo = split == 3 ? d.KT_lo[l] : nullptr; o.ldw = W; o.K = W;
    }
    KlOperand& u = S.op[p++];      // this layer's h . U^T
    u.A = pool + (size_t)2 * l * W; u.lda = slot_ld; u.row_index = c.slot_in; u.a_is_f32 = 1;
    u.WT_hi = d.UT_hi[l]; u.WT_lo = split == 3 ? d.UT_lo[l] : nullptr; u.ldw = W; u.K = W;
    S.n_ops = p;
    S.c_prev = pool + (size_t)(2 * l + 1) * W; S.c_prev_ld = slot_ld; S.c_prev_index = c.slot_in; S.out_index = c.slot_out;
    S.c_out = pool + (size_t)(2 * l + 1) * W; S.c_out_ld = slot_ld;
    S.h_out_f32 = pool + (size_t)2 * l * W; S.h_out_f32_ld = slot_ld;
    KL_TRY(kl_launch_fwd_steps(&S, 1, c.s));
  }
  return output_thin(h, n, pool, c.slot_out, c.probs, true, c.s);
}

// may the indices of a step of n rows travel in the kernel arguments (KlHostIdx: characters and the one context variable
// as halfwords; inc_cell_hx_kernel's widths)?  The callers still check the range of every index value.
static bool host_idx_in_kernarg(const kl_handle* h, int n) {
  const int W = h->cfg.width;
  return h->cfg.voc_size <= 65535 && h->cfg.ctx_vocab <= 65536 && h->cfg.n_ctx == 1 && h->inc_small && h->d.EF && h->host_kernarg &&
         ((W & 255) == 0 || W == 64 || W == 128) && !(W >= 1024 && n > 128);
}

// kl_step_batch_host: the indices in the kernel arguments of the 16-unit cell kernels?  (Up to 256 hypotheses, any number
// from 1 on; else the packed copy and the device-pointer step.)
static bool step_host_kernarg(const kl_handle* h, int n, KlIncCellPlan* cell) {
  return n <= KL_HOST_STEP_MAX && host_idx_in_kernarg(h, n) && plan_cells(h, n, true, cell);
}

// a host entry point's ticket counter: zeroed when its workspace is not the one remembered (afterwards every delivering
// launch leaves it zero)
static int arm_ticket_counter(void*& armed, unsigned* counter, hipStream_t s) {
  if (armed == counter) return 0;
  KL_TRY(kl_zero_async(counter, 64 * sizeof(unsigned), s));
  armed = counter;
  return 0;
}
}  // namespace

size_t kl_step_workspace_bytes(const kl_handle* h, int n) {
  if (!h || n < 1) return 0;
  return step_carve(h, n, nullptr).bytes;
}

int kl_step_batch(kl_handle* h, int n, const int32_t* idx, const int32_t* ctx, float* pool, const int32_t* slot_in,
                  const int32_t* slot_out, float* probs, void* ws, size_t ws_bytes, void* stream) {
  if (!h || !idx || !pool || !slot_in || !slot_out || !probs || n < 1) return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (!h->precision) return KL_ERR_STATE;
  StepCall c = {h, n, idx, ctx, pool, slot_in, slot_out, probs, nullptr, (hipStream_t)stream};
  if (h->cfg.n_ctx != 1) {      // layer 0's gate inputs gathered first (rows are hypotheses: B = n streams, T = 1)
    const StepWs w = step_carve(h, n, ws);
    if (!ws || ws_bytes < w.bytes) return KL_ERR_WORKSPACE;
    const float* ctxk[8];      // (config_ok: n_ctx <= 8)
    for (int k = 0; k < h->cfg.n_ctx; ++k) ctxk[k] = h->d.CtxK[k];
    KL_TRY(kl_launch_p1_gather(h->d.EK, ctxk, h->cfg.n_ctx, h->params + h->off_b[0], idx, ctx, n, 1, 4 * h->cfg.width, w.prow, c.s));
    c.prow = w.prow;
  }
  const StepPlan p = step_plan(h, n, ws && ws_bytes >= kl_step_workspace_bytes(h, n));
  switch (p.layers) {
    case KL_STEP_TILES:
    case KL_STEP_CELLS: return step_layers(c, p);
    case KL_STEP_GEMM_FUSED:
    case KL_STEP_GEMM_PLAIN: return step_gemm(c, p, ws);
    default: return step_thin(c);
  }
}

// ---- the incremental step as a beam search issues it: one step per character, the GPU idle in between ----------------
// (rating.py:809-826 rate_best, :689-691 generate: predict -> look at the probabilities -> decide -> predict ...)
void* kl_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
  memset(p, 0, bytes);
  return p;
}

void kl_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

size_t kl_step_host_workspace_bytes(const kl_handle* h, int n) {
  if (!h || n < 1) return 0;
  Carver cv(nullptr);
  cv.take<unsigned>(64);                                             // the finish launch's ticket counter (zero between steps)
  cv.take<float>((size_t)n * h->cfg.voc_size);                      // logits / probabilities
  cv.take<int32_t>((size_t)n * (4 + (h->cfg.n_ctx > 0 ? h->cfg.n_ctx : 1)));      // indices on the device (n > 256 and fall-backs)
  return align_up(cv.off, 256) + kl_step_workspace_bytes(h, n);
}

int kl_step_batch_host(kl_handle* h, int n, const int32_t* idx, const int32_t* ctx, const int32_t* slot_in,
                       const int32_t* slot_out, const int32_t* target, float* pool, int head_k, float* probs_host,
                       float* heads_host, uint32_t* done_host, uint32_t ticket, void* ws, size_t ws_bytes, void* stream) {
  if (!h || !idx || !pool || !slot_in || !slot_out || !probs_host || !done_host || n < 1) return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (head_k < 0 || head_k > 2 * h->cfg.depth || (head_k > 0 && !heads_host)) return KL_ERR_ARG;
  if (!h->precision) return KL_ERR_STATE;
  if (!ws || ws_bytes < kl_step_host_workspace_bytes(h, n)) return KL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const kl_config& c = h->cfg;
  const int W = c.width, L = c.depth, V = c.voc_size, C = c.n_ctx;
  Carver cv(ws);
  unsigned* counter = cv.take<unsigned>(64);
  float* logits = cv.take<float>((size_t)n * V);
  int32_t* dev_idx = cv.take<int32_t>((size_t)n * (4 + (C > 0 ? C : 1)));
  unsigned char* rest = reinterpret_cast<unsigned char*>(ws) + align_up(cv.off, 256);
  const size_t rest_bytes = ws_bytes - align_up(cv.off, 256);
  KL_TRY(arm_ticket_counter(h->host_step_ready, counter, s));
  KlStepFinish f;
  memset(&f, 0, sizeof(f));
  f.n = n; f.V = V; f.W = W; f.logits = logits; f.ld = V;
  f.by_target = target != nullptr; f.head_k = head_k;
  f.pool = pool; f.slot_ld = (long)2 * L * W;
  f.probs_host = probs_host; f.heads_host = heads_host; f.done_host = done_host; f.ticket = ticket; f.counter = counter;
  // ---- up to 256 hypotheses on the 16-unit cell kernels: every index travels in the kernel arguments
  KlIncCellPlan cells[16];
  bool in_range = step_host_kernarg(h, n, cells);
  for (int i = 0; i < n && in_range; ++i)
    in_range = idx[i] >= 0 && idx[i] < V && ctx[i] >= 0 && ctx[i] < c.ctx_vocab && (!target || (target[i] >= 0 && target[i] < V));
  if (in_range) {
    static thread_local KlHostIdx hx;
    static thread_local KlHostTargets tx;
    for (int i = 0; i < n; ++i) {
      hx.slot_in[i] = slot_in[i]; hx.slot_out[i] = slot_out[i];
      hx.idx[i] = (unsigned short)idx[i]; hx.ctx[i] = (unsigned short)ctx[i];
      if (target) tx.t[i] = (unsigned short)target[i];
    }
    if (!h->inc_ready) KL_TRY(prepare_incremental(h, s));
    for (int l = 0; l < L; ++l)      // (layer 0 leaves slot_out in dev_idx for the launches behind it)
      KL_TRY(kl_launch_inc_cell(inc_cell_args(h, l, n, pool, nullptr, nullptr, nullptr, dev_idx, dev_idx), s, &hx,
                                l == 0 ? dev_idx : nullptr));
    KL_TRY(output_thin(h, n, pool, dev_idx, logits, false, s));
    f.softmax = 1; f.slot_out = dev_idx;
    return kl_launch_step_finish(f, target ? &tx : nullptr, s);
  }
  // ---- everything else: ONE copy of the packed indices to the device, the device-pointer step, delivery by the finish launch
  {
    std::vector<int32_t>& pk = h->host_pack;
    pk.resize((size_t)n * (4 + (C > 0 ? C : 1)));
    memcpy(pk.data(), idx, (size_t)n * 4);
    memcpy(pk.data() + n, slot_in, (size_t)n * 4);
    memcpy(pk.data() + 2 * (size_t)n, slot_out, (size_t)n * 4);
    if (target) memcpy(pk.data() + 3 * (size_t)n, target, (size_t)n * 4);
    else memset(pk.data() + 3 * (size_t)n, 0, (size_t)n * 4);
    if (C > 0) memcpy(pk.data() + 4 * (size_t)n, ctx, (size_t)n * C * 4);
    if (hipMemcpyAsync(dev_idx, pk.data(), pk.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return KL_ERR_LAUNCH;
    KL_TRY(kl_step_batch(h, n, dev_idx, C > 0 ? dev_idx + 4 * (size_t)n : nullptr, pool, dev_idx + n, dev_idx + 2 * (size_t)n, logits,
                         rest, rest_bytes, stream));
    f.softmax = 0; f.slot_out = dev_idx + 2 * (size_t)n;
    f.target = target ? dev_idx + 3 * (size_t)n : nullptr;
    return kl_launch_step_finish(f, nullptr, s);
  }
}

// ---- a lattice edge in one call: every row walks through ALL its characters, no host round trip in between ------------
// (rating.py:796-851: a track's characters are its alternative's text, known before the first step)
namespace {
struct WalkWs {
  unsigned* counter; int32_t* idx; float* probs; unsigned char* rest; size_t rest_bytes, bytes;
};
// staged index words: slot_step | target (caller's ragged order), last slot per row, then -- only where the device-pointer
// step is chained -- per step idx | slot_in | slot_out | ctx of the rows still active, longest rows first
size_t walk_head_words(int n, int total) { return 2 * (size_t)total + (size_t)n; }
size_t walk_stage_words(const kl_handle* h, int n, int total) {
  return walk_head_words(n, total) + (size_t)total * (3 + (h->cfg.n_ctx > 0 ? h->cfg.n_ctx : 1));
}
WalkWs walk_carve(const kl_handle* h, int n, int total, void* ws, size_t ws_bytes) {
  Carver cv(ws);
  WalkWs w;
  w.counter = cv.take<unsigned>(64);                                 // the output launch's ticket counter (zero between calls)
  w.idx = cv.take<int32_t>(walk_stage_words(h, n, total));
  w.probs = cv.take<float>((size_t)n * h->cfg.voc_size);            // what the chained device-pointer steps write (never read)
  const size_t head = align_up(cv.off, 256);
  w.rest = ws ? reinterpret_cast<unsigned char*>(ws) + head : nullptr;
  w.bytes = head + kl_step_workspace_bytes(h, n);
  w.rest_bytes = ws_bytes > head ? ws_bytes - head : 0;
  return w;
}
}  // namespace

size_t kl_walk_workspace_bytes(const kl_handle* h, int n, int total) {
  if (!h || n < 1 || total < n) return 0;
  return walk_carve(h, n, total, nullptr, 0).bytes;
}

size_t kl_walk_stage_bytes(const kl_handle* h, int n, int total) {
  if (!h || n < 1 || total < n) return 0;
  return align_up(walk_stage_words(h, n, total) * sizeof(int32_t), 256);
}

int kl_walk_batch_host(kl_handle* h, int n, const int32_t* len, const int32_t* idx, const int32_t* target, const int32_t* ctx,
                       const int32_t* slot_in, const int32_t* slot_step, float* pool, int head_k, float* tprob_host,
                       float* heads_host, void* stage_host, uint32_t* done_host, uint32_t ticket, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!h || !len || !idx || !target || !slot_in || !slot_step || !pool || !tprob_host || !stage_host || !done_host || n < 1)
    return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (head_k < 0 || head_k > 2 * h->cfg.depth || (head_k > 0 && !heads_host)) return KL_ERR_ARG;
  long total_l = 0;
  int max_len = 0;
  for (int i = 0; i < n; ++i) {
    if (len[i] < 1 || len[i] > 1024) return KL_ERR_ARG;
    total_l += len[i];
    if (len[i] > max_len) max_len = len[i];
  }
  if (total_l > 0x3fffffff) return KL_ERR_ARG;
  if (!h->precision) return KL_ERR_STATE;
  const int total = (int)total_l;
  if (!ws || ws_bytes < kl_walk_workspace_bytes(h, n, total)) return KL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const kl_config& c = h->cfg;
  const int W = c.width, L = c.depth, V = c.voc_size, C = c.n_ctx;
  const WalkWs w = walk_carve(h, n, total, ws, ws_bytes);
  // rows ordered so that those still active at step t form a prefix: longest first, equal lengths in the caller's order
  // (a counting sort over the lengths 1 .. 1024)
  static thread_local std::vector<int32_t> order, off, count;
  order.resize(n); off.resize(n); count.assign(max_len + 2, 0);
  {
    int o = 0;
    for (int i = 0; i < n; ++i) { off[i] = o; o += len[i]; ++count[len[i]]; }
    int at = 0;
    for (int l = max_len; l >= 1; --l) { const int k = count[l]; count[l] = at; at += k; }      // first position of length l
    for (int i = 0; i < n; ++i) order[count[len[i]]++] = i;
    // (count[l] is now the number of rows of length >= l: the rows active at step l - 1)
  }
  int32_t* st = reinterpret_cast<int32_t*>(stage_host);
  memcpy(st, slot_step, (size_t)total * 4);
  memcpy(st + total, target, (size_t)total * 4);
  for (int i = 0; i < n; ++i) st[2 * (size_t)total + i] = slot_step[off[i] + len[i] - 1];
  const size_t head_words = walk_head_words(n, total);
  KL_TRY(arm_ticket_counter(h->walk_ready, w.counter, s));
  if (!h->inc_ready) KL_TRY(prepare_incremental(h, s));
  if (!h->d.EF) return KL_ERR_SHAPE;
  KlWalkOut f;
  memset(&f, 0, sizeof(f));
  f.total = total; f.n = n; f.V = V; f.W = W; f.lo = h->precision == 3; f.head_k = head_k;
  f.pool = pool; f.slot_ld = (long)2 * L * W; f.h_off = 2 * (L - 1) * W; f.EF = h->d.EF;
  f.slots = w.idx; f.targets = w.idx + total; f.last = w.idx + 2 * (size_t)total;
  f.tprob_host = tprob_host; f.heads_host = heads_host; f.done_host = done_host; f.ticket = ticket; f.counter = w.counter;
  // ---- the 16-unit cell kernels with every index of a step in the kernel arguments, groups of up to 256 rows
  bool in_range = host_idx_in_kernarg(h, n);
  for (int i = 0; i < n && in_range; ++i) in_range = ctx[i] >= 0 && ctx[i] < c.ctx_vocab;
  for (int p = 0; p < total && in_range; ++p) in_range = idx[p] >= 0 && idx[p] < V;
  if (in_range) {
    static thread_local KlHostIdx hx;
    for (int g0 = 0; g0 < n && in_range; g0 += KL_HOST_STEP_MAX) {
      const int g1 = g0 + KL_HOST_STEP_MAX < n ? g0 + KL_HOST_STEP_MAX : n;
      const int g_len = len[order[g0]];
      for (int t = 0; t < g_len && in_range; ++t) {
        const int active = (count[t + 1] < g1 ? count[t + 1] : g1) - g0;      // rows of the group with len > t
        for (int j = 0; j < active; ++j) {
          const int r = order[g0 + j], p = off[r] + t;
          hx.slot_in[j] = t ? slot_step[p - 1] : slot_in[r];
          hx.slot_out[j] = slot_step[p];
          hx.idx[j] = (unsigned short)idx[p];
          hx.ctx[j] = (unsigned short)ctx[r];
        }
        for (int l = 0; l < L && in_range; ++l) {
          const int e = kl_launch_inc_cell(inc_cell_args(h, l, active, pool, nullptr, nullptr, nullptr, w.idx, w.idx), s, &hx, nullptr);
          if (e == KL_ERR_SHAPE && !(g0 || t || l)) in_range = false;      // (the first launch decides for all: the shapes are the same)
          else if (e) return e;
        }
      }
    }
    if (in_range) {
      if (hipMemcpyAsync(w.idx, st, head_words * 4, hipMemcpyHostToDevice, s) != hipSuccess) return KL_ERR_LAUNCH;
      return kl_launch_walk_out(f, s);
    }
  }
  // ---- everything else: ONE staged upload of all indices, then the device-pointer step chained over the active prefix
  {
    const int Cc = C > 0 ? C : 1;
    size_t at = head_words;
    static thread_local std::vector<size_t> step_at;
    step_at.resize(max_len);
    for (int t = 0; t < max_len; ++t) {
      const int active = count[t + 1];
      step_at[t] = at;
      int32_t* q = st + at;
      for (int j = 0; j < active; ++j) {
        const int r = order[j], p = off[r] + t;
        q[j] = idx[p];
        q[active + j] = t ? slot_step[p - 1] : slot_in[r];
        q[2 * (size_t)active + j] = slot_step[p];
        for (int k = 0; k < Cc; ++k) q[3 * (size_t)active + (size_t)j * Cc + k] = C > 0 ? ctx[(size_t)r * C + k] : 0;
      }
      at += (size_t)active * (3 + Cc);
    }
    if (hipMemcpyAsync(w.idx, st, at * 4, hipMemcpyHostToDevice, s) != hipSuccess) return KL_ERR_LAUNCH;
    for (int t = 0; t < max_len; ++t) {
      const int active = count[t + 1];
      const int32_t* q = w.idx + step_at[t];
      KL_TRY(kl_step_batch(h, active, q, C > 0 ? q + 3 * (size_t)active : nullptr, pool, q + active, q + 2 * (size_t)active, w.probs,
                           w.rest, w.rest_bytes, stream));
    }
    return kl_launch_walk_out(f, s);
  }
}

int kl_step_wait(const uint32_t* done_host, uint32_t ticket, double timeout_s) {
  if (!done_host) return KL_ERR_ARG;
  const volatile uint32_t* flag = done_host;
  struct timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return 0;
    __builtin_ia32_pause();
    if ((spins & 0x3ff) == 0x3ff) {
      struct timespec t1;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      if ((double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > timeout_s) {
        // (a failed launch never writes the word: report what the runtime says rather than spin for ever)
        return hipGetLastError() == hipSuccess ? KL_ERR_STATE : KL_ERR_LAUNCH;
      }
    }
  }
}

int kl_state_dist2(const kl_handle* h, int n, const float* pool, const int32_t* a, const int32_t* b, int k, float* out,
                   void* stream) {
  if (!h || !pool || !a || !b || !out || n < 1) return KL_ERR_ARG;
  if (k < 0 || k >= 2 * h->cfg.depth) return KL_ERR_ARG;
  const int W = h->cfg.width;
  hipLaunchKernelGGL(state_dist2_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, pool,
                     (long)2 * h->cfg.depth * W, W, k, a, b, n, out);
  return hip_ok(hipGetLastError());
}

// ---- the beam bookkeeping of many lattice edges on the device (edge_decode.hip) ----------------------------------------
int kl_edge_costs(long n_pairs, const float* probs, const int32_t* pair_alt, const double* alt_conf, double lm_weight,
                  double* cost, void* stream) {
  if (!probs || !pair_alt || !alt_conf || !cost || n_pairs < 1 || n_pairs > (1L << 40) || lm_weight != lm_weight) return KL_ERR_ARG;
  if (((uintptr_t)probs | (uintptr_t)pair_alt) & 3 || ((uintptr_t)alt_conf | (uintptr_t)cost) & 7) return KL_ERR_ARG;
  return kl_launch_edge_costs(n_pairs, probs, pair_alt, alt_conf, lm_weight, cost, (hipStream_t)stream);
}

static size_t edge_up8(size_t n) { return (n + 7) & ~(size_t)7; }

size_t kl_edge_decode_out_bytes(int n_edges, int beam_width, long n_tracks, long n_pairs) {
  if (n_edges < 1 || beam_width < 1 || n_tracks < 1 || n_pairs < 0 || n_tracks > (1L << 40) || n_pairs > (1L << 40)) return 0;
  const size_t eb = (size_t)n_edges * beam_width;
  return eb * 8 + edge_up8((size_t)n_edges * 4) * 2 + edge_up8(eb * 4) + edge_up8((size_t)n_tracks * 4) + edge_up8((size_t)n_pairs * 4);
}

int kl_edge_decode(const kl_handle* h, int n_edges, const int32_t* desc, const double* cum_in, const int32_t* alt_len,
                   const int32_t* alt_class, const int32_t* step_off, const int32_t* final_slot,
                   const double* pre_cost, const int32_t* pre_class, const int32_t* pre_slot, const double* cost,
                   const float* pool, int depth_k, double dist, int batch_size, int beam_width, int cap_tracks, long n_tracks,
                   long n_pairs, void* out, size_t out_bytes, void* stream) {
  if (!h || !desc || !cum_in || !alt_len || !alt_class || !step_off || !final_slot || !cost || !out) return KL_ERR_ARG;
  if (n_edges < 1 || batch_size < 1 || beam_width < 1 || cap_tracks < 1 || cap_tracks > KL_EDGE_MAX_TRACKS) return KL_ERR_ARG;
  if (n_tracks < 1 || n_pairs < 0 || n_tracks > (1L << 40) || n_pairs > (1L << 40)) return KL_ERR_ARG;
  if (depth_k < 0 || depth_k > 2 * h->cfg.depth || (depth_k > 0 && (!pool || !(dist == dist)))) return KL_ERR_ARG;
  if (((uintptr_t)cum_in | (uintptr_t)cost | (uintptr_t)out | (uintptr_t)pre_cost) & 7) return KL_ERR_ARG;
  if (out_bytes < kl_edge_decode_out_bytes(n_edges, beam_width, n_tracks, n_pairs)) return KL_ERR_WORKSPACE;
  KlEdgeDecode a;
  memset(&a, 0, sizeof(a));
  a.n_edges = n_edges; a.batch_size = batch_size; a.beam_width = beam_width; a.cap_tracks = cap_tracks; a.depth_k = depth_k;
  a.W = h->cfg.width; a.slot_stride = (long)2 * h->cfg.depth * h->cfg.width; a.dist2 = dist * dist;
  a.desc = desc; a.cum_in = cum_in; a.alt_len = alt_len; a.alt_class = alt_class; a.step_off = step_off;
  a.final_slot = final_slot; a.pre_cost = pre_cost; a.pre_class = pre_class; a.pre_slot = pre_slot; a.cost = cost; a.pool = pool;
  // the output block: [cost f64 E x bw][count E][status E][ref E x bw][consumed tracks][when pairs], every part 8-byte aligned
  char* o = (char*)out;
  const size_t eb = (size_t)n_edges * beam_width;
  a.out_cost = (double*)o; o += eb * 8;
  a.out_count = (int*)o; o += edge_up8((size_t)n_edges * 4);
  a.out_status = (int*)o; o += edge_up8((size_t)n_edges * 4);
  a.out_ref = (int*)o; o += edge_up8(eb * 4);
  a.out_consumed = (int*)o; o += edge_up8((size_t)n_tracks * 4);
  a.out_when = (int*)o;
  return kl_launch_edge_decode(a, (hipStream_t)stream);
}

size_t kl_beam_workspace_bytes(const kl_handle* h, int rows, int fan) {
  if (!h || rows < 1 || rows > KL_BEAM_MAX_ROWS || fan < 1 || fan > KL_BEAM_MAX_FAN) return 0;
  return kl_beam_ws_bytes(rows, fan);
}

int kl_beam_expand(kl_handle* h, int rows, int fan, float floor, const float* probs, const uint8_t* valid, const float* cum_in,
                   const int32_t* slot_new, int32_t zero_slot, int32_t* idx_next, int32_t* slot_in_next, float* cum_next,
                   int32_t* parent_log, int32_t* idx_log, float* cum_log, int32_t* n_live, void* ws, size_t ws_bytes,
                   void* stream) {
  if (!h || !probs || !cum_in || !slot_new || !idx_next || !slot_in_next || !cum_next || !parent_log || !idx_log || !cum_log ||
      !n_live)
    return KL_ERR_ARG;
  if (rows < 1 || rows > KL_BEAM_MAX_ROWS || fan < 1 || fan > KL_BEAM_MAX_FAN) return KL_ERR_ARG;
  if (!ws || ws_bytes < kl_beam_ws_bytes(rows, fan)) return KL_ERR_WORKSPACE;
  KlBeamExpand a;
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.fan = fan; a.V = h->cfg.voc_size; a.floor = floor;
  a.probs = probs; a.valid = valid; a.cum_in = cum_in; a.slot_new = slot_new; a.zero_slot = zero_slot;
  a.idx_next = idx_next; a.slot_in_next = slot_in_next; a.cum_next = cum_next;
  a.parent_log = parent_log; a.idx_log = idx_log; a.cum_log = cum_log; a.n_live = n_live;
  return kl_launch_beam_expand(a, ws, (hipStream_t)stream);
}

size_t kl_sample_workspace_bytes(const kl_handle* h, int rows) {
  if (!h || rows < 1 || rows > KL_SAMPLE_MAX_ROWS) return 0;
  return kl_sample_ws_bytes(rows, h->cfg.voc_size);
}

int kl_sample_pick_from(kl_handle* h, int rows, uint32_t row0, const float* probs, const uint8_t* valid, float temperature,
                        int top_k, float floor, uint64_t seed, uint32_t step, const float* cum_in, int32_t* idx_next,
                        float* cum_next, float* u_log, void* ws, size_t ws_bytes, void* stream) {
  if (!h || !probs || !cum_in || !idx_next || !cum_next) return KL_ERR_ARG;
  if (rows < 1 || rows > KL_SAMPLE_MAX_ROWS || top_k < 0 || top_k > KL_SAMPLE_MAX_TOPK) return KL_ERR_ARG;
  if (!(temperature >= 0.f) || temperature == INFINITY || !(floor >= 0.f)) return KL_ERR_ARG;      // (NaN fails both comparisons)
  if (!ws || ws_bytes < kl_sample_ws_bytes(rows, h->cfg.voc_size)) return KL_ERR_WORKSPACE;
  KlSamplePick a;
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.V = h->cfg.voc_size; a.top_k = top_k; a.temperature = temperature; a.floor = floor;
  a.key0 = (unsigned)(seed & 0xffffffffu); a.key1 = (unsigned)(seed >> 32); a.step = step; a.row0 = row0;
  a.probs = probs; a.valid = valid; a.cum_in = cum_in; a.idx_next = idx_next; a.cum_next = cum_next; a.u_log = u_log;
  return kl_launch_sample_pick(a, ws, (hipStream_t)stream);
}

int kl_sample_pick(kl_handle* h, int rows, const float* probs, const uint8_t* valid, float temperature, int top_k, float floor,
                   uint64_t seed, uint32_t step, const float* cum_in, int32_t* idx_next, float* cum_next, float* u_log, void* ws,
                   size_t ws_bytes, void* stream) {
  return kl_sample_pick_from(h, rows, 0, probs, valid, temperature, top_k, floor, seed, step, cum_in, idx_next, cum_next, u_log,
                             ws, ws_bytes, stream);
}

int kl_test_gemm_tn(const uint16_t* A, const uint16_t* B, void* C, const float* bias, int M, int N, int K, long lda,
                    long ldb, long ldc, int out_mode, int splits, void* stream) {
  return kl_launch_gemm_tn(A, B, C, bias, M, N, K, lda, ldb, ldc, out_mode, splits, 1.f, (hipStream_t)stream);
}

int kl_test_gemm_an(const uint16_t* A_km, const uint16_t* B, float* C, int M, int N, int K, long lda_km, long ldb,
                    long ldc, int c_transposed, int b_km, void* stream) {
  return kl_launch_gemm_an(A_km, B, C, M, N, K, lda_km, ldb, ldc, c_transposed, (hipStream_t)stream, b_km);
}

int kl_test_gemm_an2(const uint16_t* A_km, const uint16_t* B, float* C, int M, int N, int K, long lda_km, long ldb, long ldc,
                     int c_transposed, const uint16_t* B2, float* C2, int N2, long ldb2, long ldc2, int c_transposed2, int b_km,
                     void* stream) {
  return kl_launch_gemm_an2(A_km, B, C, M, N, K, lda_km, ldb, ldc, c_transposed, B2, C2, N2, ldb2, ldc2, c_transposed2,
                            (hipStream_t)stream, b_km);
}

int kl_test_gemm_tn_route(int M, int N, int K, long lda, long ldb, long ldc, int out_mode, int splits, size_t c_addr, int has_bias,
                          int* eff_splits) {
  const KlGemmTnRoute rt = kl_gemm_tn_route(reinterpret_cast<const void*>(c_addr), has_bias != 0, M, N, K, lda, ldb, ldc, out_mode, splits);
  if (eff_splits) *eff_splits = rt.splits;
  return rt.route;
}

int kl_test_gemm_an_route(int M, int N, int N2, int K, long lda_km, long ldb, long ldb2, int b_km, int* rows_per_split) {
  const KlGemmAnRoute rt = kl_gemm_an_route(N2 > 0, M, N, N2, K, lda_km, ldb, ldb2, b_km);
  if (rows_per_split) *rows_per_split = rt.rows_per_split;
  return rt.route;
}

size_t kl_test_segment_sums_ws_bytes(int B, int T, int n_ctx, int V, int R) {
  if (B < 1 || T < 1 || V < 1 || n_ctx < 0 || (n_ctx > 0 && R < 1)) return 0;
  return kl_segment_sums_ws_bytes(B, T, n_ctx, V, R);
}

int kl_test_segment_sums_share(int B, int T) { return B < 1 || T < 1 ? 0 : kl_segment_sums_share((long)B * T); }

int kl_test_segment_sums(const uint16_t* dZ, long ld, int B, int T, int cols, const int32_t* idx, const int32_t* ctx, int n_ctx,
                         int V, int R, float* dEK, float* dCtxK, void* ws, void* stream) {
  return kl_launch_segment_sums(dZ, ld, B, T, cols, idx, ctx, n_ctx, V, R, dEK, dCtxK, ws, (hipStream_t)stream);
}

int kl_test_thin_gemm(const float* A, long lda, const uint16_t* WT_hi, const uint16_t* WT_lo, long ldw, int M, int N,
                      int K, float* C, long ldc, int split, void* stream) {
  KlOperand op;
  memset(&op, 0, sizeof(op));
  op.A = A; op.lda = lda; op.a_is_f32 = 1; op.WT_hi = WT_hi; op.WT_lo = WT_lo; op.ldw = ldw; op.K = K;
  return kl_launch_thin_gemm(&op, M, N, C, ldc, nullptr, split, (hipStream_t)stream);
}

int kl_test_thin_gemm_ex(const void* A, long lda, int a_is_f32, const int32_t* row_index, const uint16_t* WT_hi, const uint16_t* WT_lo,
                         long ldw, int M, int N, int K, float* C, long ldc, const float* bias, int split, void* stream) {
  KlOperand op;
  memset(&op, 0, sizeof(op));
  op.A = A; op.lda = lda; op.a_is_f32 = a_is_f32 ? 1 : 0; op.row_index = row_index; op.WT_hi = WT_hi; op.WT_lo = WT_lo; op.ldw = ldw; op.K = K;
  return kl_launch_thin_gemm(&op, M, N, C, ldc, bias, split, (hipStream_t)stream);
}

int kl_test_softmax_ce(float* logits, long ld, int rows, int V, const int32_t* tgt, int B, int T, float inv_count, uint16_t* dlogits,
                       long ld_dl, float* rowstat, float* loss_acc, int last_only, void* stream) {
  return kl_launch_softmax_ce(logits, ld, rows, V, tgt, B, T, inv_count, dlogits, ld_dl, loss_acc, rowstat, 1, (hipStream_t)stream, last_only);
}

int kl_test_logits_ce_ws(const uint16_t* X, const uint16_t* E, const int32_t* tgt, uint16_t* dlogits, float* rowstat, int B, int T,
                         float inv_count, int last_only, void* stream) {
  return kl_launch_logits_ce_ws(X, E, tgt, dlogits, rowstat, B, T, 512, 256, 256, inv_count, last_only, (hipStream_t)stream);
}

int kl_test_logits_ce_w128(const uint16_t* X, const uint16_t* E, const uint16_t* ET, const int32_t* tgt, uint16_t* dlogits, float* dH,
                           float* rowstat, int B, int T, int V, int Vp, float inv_count, int last_only, void* stream) {
  return kl_launch_logits_ce_w128(X, E, ET, tgt, dlogits, dH, rowstat, B, T, 128, V, Vp, inv_count, last_only, (hipStream_t)stream);
}

int kl_test_dh_ws(const uint16_t* dlogits, const uint16_t* ET, uint16_t* dH, long M, void* stream) {
  return kl_launch_dh_ws(dlogits, ET, dH, M, 512, 256, (hipStream_t)stream);
}

int kl_test_regulariser_grads(const float* X, int R, int D, int mode, float* gX, float* loss_acc, float* scratch, void* stream) {
  if (!X || !gX || !scratch || R < 1 || D < 1 || (mode != 0 && mode != 1)) return KL_ERR_ARG;
  if (mode == 0) return kl_launch_regulariser_grads(X, R, D, nullptr, 0, 0, 0, gX, nullptr, loss_acc, scratch, (hipStream_t)stream);
  return kl_launch_regulariser_grads(nullptr, 0, 0, &X, 1, R, D, nullptr, &gX, loss_acc, scratch, (hipStream_t)stream);
}

int kl_test_rate_topk(const float* logits, long ld, int rows, int V, const int32_t* tgt, int B, int T, int K,
                      float* tprob, int32_t* alt_id, float* alt_p, int32_t* rank, void* stream) {
  return kl_launch_rate_topk(logits, ld, rows, V, tgt, B, T, K, tprob, alt_id, alt_p, rank, (hipStream_t)stream);
}

}  // extern "C"

// Tuning hook: launch `iters` identical forward cell steps (bf16 A, split 1) on raw
// buffers, `fused` copies per launch.  Used by tools/probe_step.py only.
extern "C" int kl_test_fwd_step(const uint16_t* A, long lda, const uint16_t* WT, long ldw, int K, int n_ops,
                                int n_rows, int W, int fused, int iters, float* c_out, uint16_t* h_out,
                                void* stream) {
  KlFwdStep st[4];
  if (fused < 1 || fused > 4 || n_ops < 1 || n_ops > 2) return KL_ERR_ARG;
  for (int f = 0; f < fused; ++f) {
    KlFwdStep& S = st[f];
    memset(&S, 0, sizeof(S));
    S.n_rows = n_rows; S.W = W; S.split = 1; S.n_ops = n_ops;
    for (int p = 0; p < n_ops; ++p) {
      KlOperand& o = S.op[p];
      o.A = A; o.lda = lda; o.WT_hi = WT + (size_t)(f * 2 + p) * (size_t)4 * W * ldw; o.ldw = ldw;
      o.K = K; o.a_is_f32 = 0;
    }
    S.c_out = c_out + (size_t)f * n_rows * W; S.c_out_ld = W;
    S.h_out_bf16 = h_out + (size_t)f * n_rows * W; S.h_out_bf16_ld = W;
  }
  for (int i = 0; i < iters; ++i) {
    int e = kl_launch_fwd_steps(st, fused, (hipStream_t)stream);
    if (e) return e;
  }
  return 0;
}


// ---- whole-window hipGraph replay ------------------------------------------------
// A window is 2(T+L-1) dependent step launches plus ~40 helper launches; issued
// eagerly the host launch rate (~4.5 us per launch) bounds it.  The sequence is
// captured once per (shape, pointer set) and replayed.  Inputs are first staged
// into fixed workspace slots so that replays read the new batch.
namespace {

int run_graphed(kl_handle* h, const kl_handle::GraphKey& key, hipStream_t s, const std::function<int()>& body) {
  if (!h->graphs_enabled || h->trace_on || s == nullptr) return body();   // (the legacy default stream cannot be captured)
  for (auto& g : h->graphs)
    if (g.first == key) return hip_ok(hipGraphLaunch(g.second, s));
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    h->graphs_enabled = false;
    return body();
  }
  const int e = body();
  hipGraph_t graph = nullptr;
  const hipError_t ce = hipStreamEndCapture(s, &graph);
  if (e != 0 || ce != hipSuccess || graph == nullptr) {
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    h->graphs_enabled = false;
    return e != 0 ? e : body();
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ie != hipSuccess || exec == nullptr) {
    (void)hipGetLastError();
    h->graphs_enabled = false;
    return body();
  }
  if (h->graphs.size() >= 16) h->drop_graphs();
  h->graphs.emplace_back(key, exec);
  return hip_ok(hipGraphLaunch(exec, s));
}

}  // namespace

extern "C" int kl_set_loss_rows(kl_handle* h, int rows) {
  if (!h || rows < 0) return KL_ERR_ARG;
  h->loss_rows = rows;
  return 0;
}

extern "C" int kl_set_window_mode(kl_handle* h, int last_only) {
  if (!h) return KL_ERR_ARG;
  h->last_only = last_only ? 1 : 0;
  return 0;
}

namespace {

// the caller's idx / ctx / tgt (and a training window's masks) into the window's staging slots: what a captured body reads
int stage_window(const kl_handle* h, const WindowWs& w, int B, int T, const int32_t* idx, const int32_t* ctx,
                 const int32_t* tgt, const float* masks, hipStream_t s) {
  const size_t BT = (size_t)B * T;
  KL_TRY(hip_ok(hipMemcpyAsync(w.s_idx, idx, BT * sizeof(int), hipMemcpyDeviceToDevice, s)));
  if (h->cfg.n_ctx > 0)
    KL_TRY(hip_ok(hipMemcpyAsync(w.s_ctx, ctx, BT * h->cfg.n_ctx * sizeof(int), hipMemcpyDeviceToDevice, s)));
  if (tgt) KL_TRY(hip_ok(hipMemcpyAsync(w.s_tgt, tgt, BT * sizeof(int), hipMemcpyDeviceToDevice, s)));
  if (masks)
    KL_TRY(hip_ok(hipMemcpyAsync(w.s_masks, masks, (size_t)h->cfg.depth * B * h->cfg.width * sizeof(float),
                                 hipMemcpyDeviceToDevice, s)));
  return 0;
}

}  // namespace

extern "C" int kl_forward_window(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                                 float* states, float* probs, float* loss_acc, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (!h || !idx || !states || !ws || B < 1 || T < 1) return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (!h->precision) return KL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  WindowWs w;
  // (bf16 windows on a training-size workspace run the training forward: the staging slots must come from the
  // same layout the body is going to carve -- see forward_window_body)
  const int layout = (h->precision == KL_PREC_BF16 && ws_bytes >= carve_window(h, nullptr, B, T, 1, nullptr)) ? 1 : 0;
  if (ws_bytes < carve_window(h, ws, B, T, layout, &w)) return KL_ERR_WORKSPACE;
  const size_t BT = (size_t)B * T;
  KL_TRY(stage_window(h, w, B, T, idx, ctx, tgt, nullptr, s));
  kl_handle::GraphKey key{0, B, T, (tgt ? 1 : 0) | (probs ? 2 : 0) | (h->last_only ? 4 : 0) | (h->loss_rows << 3), h->precision, states, loss_acc, ws, nullptr, layout};      // (loss_rows: baked into the captured launches)
  KL_TRY(run_graphed(h, key, s, [&]() {
    return forward_window_body(h, B, T, w.s_idx, w.s_ctx, tgt ? w.s_tgt : nullptr, states, probs ? w.s_probs : nullptr,
                               loss_acc, ws, ws_bytes, stream);
  }));
  if (probs)
    KL_TRY(hip_ok(hipMemcpyAsync(probs, w.s_probs, BT * h->cfg.voc_size * sizeof(float), hipMemcpyDeviceToDevice, s)));
  return 0;
}

// ---- rating windows (rating.py:493-529 `rate`, many texts at once) --------------------------------------------
// The window of kl_forward_window, but the [B][T][V] softmax is never formed.  Four deliveries of one body, rate_window_impl:
//                             layout                                  K    leaves the window
//   kl_rate_window            0: inference (window_logits)            0    the target's probability per position and/or
//   kl_rate_window_bulk       1: training (window_logits_training)    0      one f64 sum of bits per stream
//   kl_rate_window_alts       0                                       >0   ... and the top K characters and the target's rank
//   kl_rate_window_alts_bulk  1                                       >0
// Layout 0 takes any prepared precision and 256 streams per scan launch; layout 1 is bf16's: the wide persistent scans of
// a validation window take thousands of streams per launch.  The workspace is the layout's window (carve_window); with
// K = 0 its probability staging slot holds the [B][T] picks.  With K > 0 the results are staged behind it in an area of
// their own (carve_alts) -- the slot holds B*T*V floats, fewer than the B*T*(2K + 2) words of a call once V < 2K + 2 --
// and copied out after the graph, as tprob is.
namespace {

struct AltsWs {
  float* tprob;      // [B][T]
  int* alt_id;       // [B][T][K]
  float* alt_p;      // [B][T][K]
  int* rank;         // [B][T]
};

// the staging area at `base` (the first byte behind the window's workspace): bytes taken
size_t carve_alts(void* base, size_t BT, int K, AltsWs* out) {
  Carver cv(base);
  AltsWs tmp;
  AltsWs& o = out ? *out : tmp;
  o.tprob = cv.take<float>(BT);
  o.alt_id = cv.take<int>(BT * K);
  o.alt_p = cv.take<float>(BT * K);
  o.rank = cv.take<int>(BT);
  return align_up(cv.off, 256);
}

int rate_window_impl(kl_handle* h, int layout, int K, int B, int T, const int32_t* idx, const int32_t* ctx,
                     const int32_t* tgt, float* states, float* tprob, int32_t* alt_id, float* alt_p, int32_t* rank,
                     double* bits, float* status, void* ws, size_t ws_bytes, void* stream) {
  const bool alts = K != 0;
  if (!h || !idx || !states || !ws || B < 1 || T < 1) return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (alts ? !tgt || !alt_id || !alt_p || K < 1 || K > KL_RATE_ALTS_MAX : (tprob || bits) && !tgt) return KL_ERR_ARG;
  // (the training forward is bf16's; one target per window is the stateless graph's: kl_forward_window)
  if ((layout ? h->precision != KL_PREC_BF16 : !h->precision) || h->last_only) return KL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  WindowWs w;
  AltsWs a{};
  const size_t BT = (size_t)B * T;
  const size_t n_window = carve_window(h, nullptr, B, T, layout, nullptr);      // (a multiple of 256: the staging area starts aligned)
  if (ws_bytes < n_window + (alts ? carve_alts(nullptr, BT, K, nullptr) : 0)) return KL_ERR_WORKSPACE;
  carve_window(h, ws, B, T, layout, &w);
  if (alts) carve_alts(reinterpret_cast<unsigned char*>(ws) + n_window, BT, K, &a);
  else a.tprob = w.s_probs;
  const bool pick = alts || tprob || bits;
  KL_TRY(stage_window(h, w, B, T, idx, ctx, pick ? tgt : nullptr, nullptr, s));
  // (baked into the captured launches: K, states, status, bits and the workspace -- all in the key; tprob, alt_id, alt_p and
  // rank are staged, and which of the optional ones the caller takes is in the key's flags.  A kind per delivery and
  // layout: the same arrays may serve all four calls)
  const int flags = (tprob ? 1 : 0) | (bits ? 2 : 0) | (alts ? (rank ? 4 : 0) | (K << 3) : 0);
  kl_handle::GraphKey key{(alts ? 3 : 2) + 2 * layout, B, T, flags, h->precision, states, status, ws, bits, layout};
  KL_TRY(run_graphed(h, key, s, [&]() {
    const int V = h->cfg.voc_size;
    KL_TRY(layout ? window_logits_training(h, B, T, w.s_idx, w.s_ctx, states, w, s)
                  : window_logits(h, B, T, w.s_idx, w.s_ctx, states, w, s));
    if (alts) KL_TRY(kl_launch_rate_topk(w.logits, V, B * T, V, w.s_tgt, B, T, K, a.tprob, a.alt_id, a.alt_p, a.rank, s));
    else if (pick) KL_TRY(kl_launch_rate_pick(w.logits, V, B * T, V, w.s_tgt, B, T, a.tprob, s));
    if (bits) KL_TRY(kl_launch_rate_bits(a.tprob, w.s_tgt, B, T, bits, s));
    if (status) hipLaunchKernelGGL(scan_status_kernel, dim3(1), dim3(64), 0, s, w.scan_status, status);
    return hip_ok(hipGetLastError());
  }));
  if (tprob) KL_TRY(hip_ok(hipMemcpyAsync(tprob, a.tprob, BT * sizeof(float), hipMemcpyDeviceToDevice, s)));
  if (!alts) return 0;
  KL_TRY(hip_ok(hipMemcpyAsync(alt_id, a.alt_id, BT * K * sizeof(int), hipMemcpyDeviceToDevice, s)));
  KL_TRY(hip_ok(hipMemcpyAsync(alt_p, a.alt_p, BT * K * sizeof(float), hipMemcpyDeviceToDevice, s)));
  if (rank) KL_TRY(hip_ok(hipMemcpyAsync(rank, a.rank, BT * sizeof(int), hipMemcpyDeviceToDevice, s)));
  return 0;
}

}  // namespace

extern "C" size_t kl_rate_workspace_bytes(const kl_handle* h, int B, int T) {
  if (!h || B < 1 || T < 1) return 0;
  return carve_window(h, nullptr, B, T, 0, nullptr);
}

extern "C" size_t kl_rate_bulk_workspace_bytes(const kl_handle* h, int B, int T) {
  if (!h || B < 1 || T < 1) return 0;
  return carve_window(h, nullptr, B, T, 1, nullptr);
}

extern "C" size_t kl_rate_alts_workspace_bytes(const kl_handle* h, int B, int T, int K) {
  if (!h || B < 1 || T < 1 || K < 1 || K > KL_RATE_ALTS_MAX) return 0;
  return carve_window(h, nullptr, B, T, 0, nullptr) + carve_alts(nullptr, (size_t)B * T, K, nullptr);
}

extern "C" size_t kl_rate_alts_bulk_workspace_bytes(const kl_handle* h, int B, int T, int K) {
  if (!h || B < 1 || T < 1 || K < 1 || K > KL_RATE_ALTS_MAX) return 0;
  return carve_window(h, nullptr, B, T, 1, nullptr) + carve_alts(nullptr, (size_t)B * T, K, nullptr);
}

extern "C" int kl_rate_window(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                              float* states, float* tprob, double* bits, float* status, void* ws, size_t ws_bytes,
                              void* stream) {
  return rate_window_impl(h, 0, 0, B, T, idx, ctx, tgt, states, tprob, nullptr, nullptr, nullptr, bits, status, ws, ws_bytes, stream);
}

extern "C" int kl_rate_window_bulk(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                                   float* states, float* tprob, double* bits, float* status, void* ws, size_t ws_bytes,
                                   void* stream) {
  return rate_window_impl(h, 1, 0, B, T, idx, ctx, tgt, states, tprob, nullptr, nullptr, nullptr, bits, status, ws, ws_bytes, stream);
}

extern "C" int kl_rate_window_alts(kl_handle* h, int B, int T, int K, const int32_t* idx, const int32_t* ctx,
                                   const int32_t* tgt, float* states, float* tprob, int32_t* alt_id, float* alt_p,
                                   int32_t* rank, double* bits, float* status, void* ws, size_t ws_bytes, void* stream) {
  if (K == 0) return KL_ERR_ARG;      // (rate_window_impl reads K = 0 as target-only delivery)
  return rate_window_impl(h, 0, K, B, T, idx, ctx, tgt, states, tprob, alt_id, alt_p, rank, bits, status, ws, ws_bytes, stream);
}

extern "C" int kl_rate_window_alts_bulk(kl_handle* h, int B, int T, int K, const int32_t* idx, const int32_t* ctx,
                                        const int32_t* tgt, float* states, float* tprob, int32_t* alt_id, float* alt_p,
                                        int32_t* rank, double* bits, float* status, void* ws, size_t ws_bytes, void* stream) {
  if (K == 0) return KL_ERR_ARG;
  return rate_window_impl(h, 1, K, B, T, idx, ctx, tgt, states, tprob, alt_id, alt_p, rank, bits, status, ws, ws_bytes, stream);
}

extern "C" int kl_train_window(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                               float* states, const float* masks, float* grads, float* loss_acc, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!h || !idx || !tgt || !states || !grads || !ws || B < 1 || T < 1) return KL_ERR_ARG;
  if (h->cfg.n_ctx > 0 && !ctx) return KL_ERR_ARG;
  if (h->precision != KL_PREC_BF16) return KL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  WindowWs w;
  if (ws_bytes < carve_window(h, ws, B, T, 1, &w)) return KL_ERR_WORKSPACE;
  KL_TRY(stage_window(h, w, B, T, idx, ctx, tgt, masks, s));
  kl_handle::GraphKey key{1, B, T, (masks ? 1 : 0) | (h->last_only ? 4 : 0), h->precision, states, loss_acc, ws, grads, h->loss_rows};      // (last field: the count baked into the captured launches)
  return run_graphed(h, key, s, [&]() {
    return train_window_body(h, B, T, w.s_idx, w.s_ctx, w.s_tgt, states, masks ? w.s_masks : nullptr, grads, loss_acc,
                             ws, ws_bytes, stream);
  });
}


extern "C" int kl_test_window_view(const kl_handle* h, int B, int T, const void* ws, kl_window_view* out) {
  if (!h || !ws || !out || B < 1 || T < 1) return KL_ERR_ARG;
  const kl_handle::ViewNote* note = const_cast<kl_handle*>(h)->view_note(B, T, ws, false);
  if (!note) return KL_ERR_STATE;
  WindowWs w;
  carve_window(h, const_cast<void*>(ws), B, T, 1, &w);
  memset(out, 0, sizeof(*out));
  out->depth = h->cfg.depth; out->width = h->cfg.width; out->B = B; out->T = T;
  out->g_interleaved = note->g_interleaved; out->c_in_cb = note->c_in_cb; out->dh_bf16 = note->dh_bf16;
  out->p_bf16_mask = (int32_t)note->p_bf16_mask; out->scan2_rows = note->scan2_rows;
  out->wg_route = (int32_t)note->wg_route; out->wg_pair_mask = (int32_t)note->wg_pair_mask;
  out->wg_db_scan_mask = (int32_t)note->wg_db_scan_mask; out->out_route = (int32_t)note->out_route;
  const unsigned char* base = reinterpret_cast<const unsigned char*>(ws);
  auto off = [&](const void* p) { return (uint64_t)(reinterpret_cast<const unsigned char*>(p) - base); };
  for (int l = 0; l < h->cfg.depth; ++l) {      // (config_ok: at most 16 layers)
    out->off_H[l] = off(w.H[l]); out->off_C[l] = off(w.C[l]); out->off_Cb[l] = off(w.Cb[l]);
    out->off_G[l] = off(w.G[l]); out->off_dZ[l] = off(w.dZ[l]);
    out->off_Hd[l] = ((note->hd_mask >> l) & 1u) ? off(w.Hd[l]) : 0;
  }
  out->off_dlogits = off(w.dlogits); out->ld_dlogits = (uint64_t)h->Vp;
  return 0;
}

extern "C" int kl_test_forward_view(const kl_handle* h, int B, int T, const void* ws, kl_forward_view* out) {
  if (!h || !ws || !out || B < 1 || T < 1) return KL_ERR_ARG;
  const kl_handle::ForwardNote* note = const_cast<kl_handle*>(h)->forward_note(B, T, ws, false);
  if (!note || !note->family) return KL_ERR_STATE;      // (no family finished: the window's launch sequence failed half built)
  WindowWs w;
  carve_window(h, const_cast<void*>(ws), B, T, 0, &w);
  memset(out, 0, sizeof(*out));
  out->depth = h->cfg.depth; out->width = h->cfg.width; out->B = B; out->T = T;
  out->family = note->family; out->passed_mask = note->passed_mask;
  out->ring_mask = (int32_t)note->ring_mask; out->thin_mask = (int32_t)note->thin_mask;
  out->handoff = note->handoff; out->c_every_step = note->c_every_step; out->precision = note->precision; out->p1_layer = note->p1_layer;
  const unsigned char* base = reinterpret_cast<const unsigned char*>(ws);
  auto off = [&](const void* p) { return (uint64_t)(reinterpret_cast<const unsigned char*>(p) - base); };
  for (int l = 0; l < h->cfg.depth; ++l) {      // (config_ok: at most 16 layers)
    out->off_H[l] = off(w.H[l]); out->off_C[l] = off(w.C[l]);
    out->off_Xhi[l] = note->planes ? off(w.Xhi[l]) : 0; out->off_Xlo[l] = note->planes ? off(w.Xlo[l]) : 0;
  }
  out->off_P1 = off(w.P1);
  return 0;
}

extern "C" int kl_test_derived_view(const kl_handle* h, kl_derived_view* out) {
  if (!h || !out) return KL_ERR_ARG;
  if (!h->derived_ws) return KL_ERR_STATE;
  const kl_config& c = h->cfg;
  const Derived& d = h->d;
  memset(out, 0, sizeof(*out));
  out->depth = c.depth; out->width = c.width; out->voc_size = c.voc_size; out->Vp = h->Vp;
  out->n_ctx = c.n_ctx; out->ctx_vocab = c.ctx_vocab; out->ctx_dim = c.ctx_dim; out->precision = h->precision;
  if (h->precision) {
    out->current = KL_DV_EAGER | (h->precision == KL_PREC_SPLIT ? KL_DV_LO : 0) | (h->il_ready ? KL_DV_INTERLEAVED : 0) |
                   (h->inc_ready ? KL_DV_INC : 0) | (h->big_ready ? KL_DV_BIG : 0) | (h->comb_ready ? KL_DV_COMB : 0);
  }
  const unsigned char* base = reinterpret_cast<const unsigned char*>(h->derived_ws);
  auto off = [&](const void* p) { return p ? (uint64_t)(reinterpret_cast<const unsigned char*>(p) - base) : (uint64_t)0; };
  for (int l = 0; l < c.depth; ++l) {      // (config_ok: at most 16 layers, 8 context variables)
    out->off_UT_hi[l] = off(d.UT_hi[l]); out->off_UT_lo[l] = off(d.UT_lo[l]);
    out->off_KT_hi[l] = off(d.KT_hi[l]); out->off_KT_lo[l] = off(d.KT_lo[l]);
    out->off_Un[l] = off(d.Un[l]); out->off_Kn[l] = off(d.Kn[l]);
    out->off_KTp[l] = off(d.KTp[l]); out->off_bp[l] = off(d.bp[l]);
    out->off_UF[l] = off(d.UF[l]); out->off_KF[l] = off(d.KF[l]);
    out->off_WTcat[l] = off(d.WTcat[l]); out->off_WTperm[l] = off(d.WTperm[l]);
    if (d.KTp[l]) out->mask_il |= 1 << l;
    if (d.KF[l]) out->mask_KF |= 1 << l;
  }
  for (int n = 0; n < c.n_ctx; ++n) { out->off_CtxK[n] = off(d.CtxK[n]); out->off_CtxKp[n] = off(d.CtxKp[n]); }
  out->off_E_hi = off(d.E_hi); out->off_E_lo = off(d.E_lo); out->off_ET = off(d.ET);
  out->off_EK = off(d.EK); out->off_EKp = off(d.EKp); out->off_EF = off(d.EF); out->off_Ecat = off(d.Ecat);
  out->has_comb = d.comb ? 1 : 0;
  out->off_comb = off(d.comb);
  out->bytes = (uint64_t)carve_derived(h, nullptr, nullptr);
  return 0;
}

extern "C" int kl_test_step_route(const kl_handle* h, int n, int has_ws, int host, kl_step_route* out) {
  if (!h || !out || n < 1) return KL_ERR_ARG;
  if (!h->params) return KL_ERR_STATE;
  const int L = h->cfg.depth;
  memset(out, 0, sizeof(*out));
  StepPlan p;
  memset(&p, 0, sizeof(p));
  if (host && step_host_kernarg(h, n, p.cell)) {
    p.layers = KL_STEP_CELLS;
    p.out = KL_STEP_OUT_THIN;
    out->idx = KL_STEP_IDX_KERNARG;
  } else {
    if (h->cfg.n_ctx != 1 && !host && !has_ws) return KL_ERR_WORKSPACE;
    p = step_plan(h, n, host || has_ws);
    out->idx = host ? KL_STEP_IDX_PACKED : KL_STEP_IDX_DEVICE;
    out->gathered = h->cfg.n_ctx != 1;
  }
  out->layers = p.layers; out->out = p.out; out->depth = L;
  out->lo = h->precision == KL_PREC_SPLIT;
  if (p.layers == KL_STEP_TILES) { out->tile_rows = p.tile.rows; out->px = p.tile.px; out->py = p.tile.py; }
  if (p.layers == KL_STEP_CELLS)
    for (int l = 0; l < L; ++l) { out->nmt[l] = p.cell[l].nmt; out->gen[l] = p.cell[l].gen; }
  return 0;
}

extern "C" int kl_test_prepare_lazy(kl_handle* h, int mask, void* stream) {
  if (!h || mask < 1 || mask > 7) return KL_ERR_ARG;
  if (!h->precision) return KL_ERR_STATE;
  if ((mask & 4) && (!h->d.comb || !h->il_ready)) return KL_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (mask & 1) KL_TRY(prepare_incremental(h, s));
  if (mask & 2) KL_TRY(prepare_big_step(h, s));
  if (mask & 4) KL_TRY(build_comb(h, s));
  return 0;
}

// ---- per-launch timing of the step kernels (bench.py roofline leg) -----------------
extern "C" int kl_trace_enable(kl_handle* h, int on) {
  if (!h) return KL_ERR_ARG;
  h->trace_on = on != 0;
  h->trace_used[0] = h->trace_used[1] = 0;
  h->trace_persistent[0] = h->trace_persistent[1] = false;
  h->trace_name[0] = "lstm_fwd_step_kernel";
  h->trace_name[1] = "lstm_bwd_step_kernel";
  return 0;
}

// kind 0 = forward cell-step launches, 1 = backward; call after synchronising the stream
extern "C" const char* kl_trace_kernel_name(kl_handle* h, int kind) {
  if (!h || kind < 0 || kind > 1) return "";
  return h->trace_name[kind];
}

extern "C" int kl_trace_read(kl_handle* h, int kind, int* n_launches, float* total_ms, int* persistent,
                             double* flops_per_launch) {
  if (!h || kind < 0 || kind > 1 || !n_launches || !total_ms) return KL_ERR_ARG;
  float total = 0.f;
  int n = 0;
  for (size_t i = 0; i < h->trace_used[kind]; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->trace_ev[kind][i].first, h->trace_ev[kind][i].second) == hipSuccess) {
      total += ms;
      ++n;
    }
  }
  // a pair brackets one persistent scan launch, or 8 consecutive launch-per-step launches
  *n_launches = h->trace_persistent[kind] ? n : 8 * n;
  *total_ms = total;
  if (persistent) *persistent = h->trace_persistent[kind] ? 1 : 0;
  // persistent scans report the contractions they actually carry; the step path carries
  // every layer's cell (recurrent + input contraction above layer 0) for B rows per launch
  if (flops_per_launch) *flops_per_launch = h->trace_persistent[kind] ? h->trace_flops[kind] : 0.0;
  return 0;
}
