"""What the recurrence scans of a training window leave in the workspace, held to the oracle tile by tile.

Shared by tests/test_window_view_ref.py (CPU: decoders, references, the checker's own sensitivity, the choice of inputs),
tests/test_window_intermediates_gpu.py (every scan family against the references) and `check_train_window_gradients`
of tests/test_gpu_kernels.py (the exact checks only).

* `decode_window` / `encode_window`: the arrays behind a `kl_window_view` (include/keraslm_hip.h) <-> canonical numpy arrays,
  h and c [L][B][T][W], gates and dz [L][B][T][4][W] in i,f,c,o order; `decode_dlogits` / `encode_dlogits`: the output layer's
  gradient of the logits, [B*T][Vp] time-major.
* `references`: the f64 oracle and the "bf16-storage oracle" (oracle.lstm_oracle.Storage: the same arithmetic in f32 with bf16
  rounding wherever the HIP path stores bf16, following the flags of the view) -- both from oracle/lstm_oracle.py alone.
* `check_tiles`: a TILE is one layer x one step x 16 consecutive streams, the hand-off unit of every scan.  Tile error =
  |got - f64|_2 / max(|f64|_2, floor), floor = FLOOR_FRAC x the array's RMS over the layer x sqrt(tile elements).  The bound
  of array X in layer l is FACTOR = 2 x the LARGEST tile error of the bf16-storage oracle for the same X, l and inputs: the
  kernels differ from that emulation only in f32 summation order and their transcendental approximations, and a maximum
  over tiles of an RMS over >= 1024 elements is tightly concentrated -- twice it is generous for rounding and, with the
  emulation's own maximum held below EMU_MAX = 0.1, at least five times below a tile that is wrong by O(1).  No number is
  fixed in advance.
* `exact_checks`: no tolerance -- no NaN / Inf halfword (a surviving 0xFFFF sentinel is a NaN), dummy streams' dZ exactly
  zero, block 0 = the carried-in state, block T = the carried-out state.

FLOOR_FRAC = 0.02: a tile whose f64 norm is below 2 % of a typical tile's is measured against that 2 % instead (its own
rounding is relative to the LARGER quantities it was computed from); with at most FLOOR_SHARE_MAX = 5 % of the tiles in
that regime (asserted from the f64 oracle alone, `floor_share`) the check still sees every tile at full strength or nearly.
"""
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import lstm_oracle as O

TILE = 16
FLOOR_FRAC = 0.02
FLOOR_SHARE_MAX = 0.05
FACTOR = 2.0
EMU_MAX = 0.1
ARRAYS = ("h", "c", "gates", "dz")

Case = namedtuple("Case", "name family env depth width voc B T n_ctx fwd bwd last_only")

_W2, _F8 = "lstm_scan_fwd_wide2_kernel", "lstm_scan_fwd8_kernel"
_BW2, _RT = "lstm_scan_bwd_wide2_kernel", "lstm_scan_bwd_regtile_kernel"


def _case(name, family, env, shape, fwd, bwd, n_ctx=1, last_only=False):
    fwd = (fwd,) if isinstance(fwd, str) else tuple(fwd)
    bwd = (bwd,) if isinstance(bwd, str) else tuple(bwd)
    return Case(name, family, dict(env), *shape, n_ctx, fwd, bwd, last_only)


# the smallest shapes of the tables in tests/test_gpu_kernels.py that still give a workgroup a second visit or a second phase
CASES = [
    _case("thin-256", "thin fused", {}, (2, 256, 40, 5, 9), "lstm_scan_fwd_kernel", "lstm_scan_bwd_kernel"),
    _case("thin-128", "thin fused", {"KL_W128": "0"}, (3, 128, 30, 20, 6), "lstm_scan_fwd_kernel", "lstm_scan_bwd_kernel", n_ctx=2),
    _case("per-step", "launch per step", {"KL_SCAN": "0"}, (2, 128, 40, 20, 9), "lstm_fwd_step_kernel", "lstm_bwd_step_kernel"),
    _case("padded-width", "padded width", {}, (2, 100, 50, 24, 9), "lstm_scan_fwd_w128_multi_kernel", "lstm_scan_bwd_w128_multi_kernel"),
    _case("wide1-counters", "wide, first generation", {"KL_WIDE_FWD_MIN": "1", "KL_SCAN2": "0"}, (2, 512, 64, 144, 6),
          "lstm_scan_fwd_wide_kernel", "lstm_scan_bwd_wide_kernel"),
    _case("wide1-sentinels", "wide, first generation", {"KL_WIDE_FWD_MIN": "1", "KL_SCAN2": "0"}, (2, 512, 64, 1040, 3),
          "lstm_scan_fwd_wide_kernel", "lstm_scan_bwd_wide_kernel"),
    _case("wide1-sentinels-noroll", "wide, first generation", {"KL_WIDE_FWD_MIN": "1", "KL_SCAN2": "0", "KL_SENTINEL_ROLL": "0"},
          (2, 512, 64, 1040, 3), "lstm_scan_fwd_wide_kernel", "lstm_scan_bwd_wide_kernel"),
    _case("scan2-1024", "second generation", {}, (2, 512, 64, 1024, 4), (_W2, _F8), _BW2),
    _case("scan2-2048-flags", "second generation", {}, (2, 512, 64, 2048, 3), (_W2, _F8), _BW2),
    _case("scan2-pf2", "second generation, prefetch", {"KL_SCAN2_PF": "2"}, (2, 512, 64, 1024, 4), (_W2, _F8), _BW2),
    _case("scan2-f32", "second generation, f32 exchange", {"KL_SCAN2_BF16": "0"}, (2, 512, 64, 2048, 3), _W2, _BW2),
    _case("regtile", "second generation, register tile", {}, (2, 512, 64, 3072, 5), (_W2, _F8), _RT),
    _case("regtile-off", "second generation, register tile", {"KL_REGTILE": "0"}, (2, 512, 64, 3072, 5), (_W2, _F8), _BW2),
    _case("regtile-wt", "second generation, register tile", {"KL_RT_LOCAL": "0"}, (2, 512, 64, 3072, 5), (_W2, _F8), _RT),
    _case("fwd8", "eight-wave forward", {"KL_FWD8": "2", "KL_SCAN2_ROWS": "32"}, (2, 512, 64, 2048, 6), _F8, (_BW2, _RT)),
    _case("fwd8-counters", "eight-wave forward, counters", {"KL_FWD8": "2", "KL_FWD8_LS": "0", "KL_SCAN2_ROWS": "32"},
          (2, 512, 64, 2048, 6), _F8, (_BW2, _RT)),
    _case("fwd8-table", "eight-wave forward, table mode", {}, (1, 512, 64, 3072, 6), _F8, (_BW2, _RT)),
    _case("w1024-nine", "width 1024", {"KL_W32_MIN_RB": "1"}, (2, 1024, 40, 144, 5), "lstm_scan_fwd_w32_kernel", "lstm_scan_bwd_w32_kernel"),
    _case("w1024-ragged", "width 1024", {"KL_W32_MIN_RB": "1"}, (2, 1024, 40, 40, 4), "lstm_scan_fwd_w32_kernel", "lstm_scan_bwd_w32_kernel"),
    _case("w128-multi", "width 128, multi", {"KL_W128_MIN": "1"}, (2, 128, 70, 40, 12),
          "lstm_scan_fwd_w128_multi_kernel", "lstm_scan_bwd_w128_multi_kernel"),
    _case("w128-multi-ragged", "width 128, multi", {"KL_W128_MIN": "1"}, (4, 128, 30, 33, 5),
          "lstm_scan_fwd_w128_multi_kernel", "lstm_scan_bwd_w128_multi_kernel"),
    _case("w128-single", "width 128, single", {"KL_W128_MIN": "1", "KL_W128_MULTI": "0"}, (2, 128, 70, 40, 12),
          "lstm_scan_fwd_w128_kernel", "lstm_scan_bwd_w128_kernel"),
    _case("w128-unfused", "width 128, unfused", {"KL_W128_FUSE": "0"}, (2, 128, 70, 40, 12),
          "lstm_scan_fwd_w128_kernel", "lstm_scan_bwd_w128_kernel"),
    # the stateless graph: one target per window, at its last position (the other cases: the stateful graph)
    _case("last-only", "width 128, multi", {"KL_W128_MIN": "1"}, (2, 128, 70, 40, 4),
          "lstm_scan_fwd_w128_multi_kernel", "lstm_scan_bwd_w128_multi_kernel", last_only=True),
]
# the two further tests of tests/test_window_intermediates_gpu.py (their inputs are held to the floor-share cap as well)
REPLAY_A = _case("replay-A", "second generation", {}, (2, 512, 64, 1024, 4), (_W2, _F8), _BW2)
REPLAY_B = _case("replay-B", "second generation", {}, (2, 512, 64, 2048, 3), (_W2, _F8), _BW2)
CONSECUTIVE = _case("consecutive", "wide, first generation", {"KL_WIDE_FWD_MIN": "1", "KL_SCAN2": "0"}, (2, 512, 64, 1040, 3),
                    "lstm_scan_fwd_wide_kernel", "lstm_scan_bwd_wide_kernel")


# ---------------------------------------------------------------------------------------------- inputs
def first_dummy(B):
    """Dummy streams (targets -2 at every position) are a suffix of the batch, as kl_set_loss_rows takes them: the last
    16-row block (ragged or not) entirely and the upper half of the block before it; with a single block its upper half."""
    nb = -(-B // TILE)
    if nb == 1:
        return max(1, (B + 1) // 2)
    return TILE * (nb - 2) + TILE // 2


def make_inputs(case, seed=21, state_scale=0.5, states=None):
    """Everything one window of `case` needs, from the case alone: indices, contexts, targets (a padded tail of -1 in stream
    0, dummy streams -2 from `n_real` on), carried-in states [B][2L][W] (f32; `states` overrides the drawn ones), keep-masks
    [L][B][W].  Inputs were chosen on the f64 oracle alone so that `floor_share` stays below FLOOR_SHARE_MAX:
    emb_std = 0.3 (a trained model's scale), carried-in states of standard deviation 0.5 (saturating cells would make whole
    dz tiles tiny), a target at every position of the real streams."""
    rng = np.random.default_rng(seed)
    L, W, V, B, T = case.depth, case.width, case.voc, case.B, case.T
    idx = rng.integers(0, V, (B, T))
    ctx = rng.integers(0, 200, (B, 1, case.n_ctx)).repeat(T, axis=1)
    tgt = rng.integers(0, V, (B, T))
    if case.last_only:
        tgt[:, :-1] = -1
    else:
        tgt[0, (-2 if T > 4 else -1):] = -1
    n_real = first_dummy(B)
    tgt[n_real:] = -2
    drawn = (rng.standard_normal((B, 2 * L, W)) * state_scale).astype(np.float32)
    keep = rng.random((L, B, W)) >= O.DROPOUT_RATE
    masks = (keep / (1.0 - O.DROPOUT_RATE)).astype(np.float32)
    masks[0] = 1.0
    return dict(idx=idx, ctx=ctx, tgt=tgt, states=drawn if states is None else np.asarray(states, dtype=np.float32),
                masks=masks, n_real=n_real, seed=seed)


def dummy_blocks(B, n_real):
    """16-row blocks without a real stream"""
    nb = -(-B // TILE)
    return [b for b in range(nb) if b * TILE >= n_real]


# ---------------------------------------------------------------------------------------------- references
_ref_cache = OrderedDict()


def _window(case, w, inp, dtype, storage):
    cfg = O.ModelConfig(case.depth, case.width, case.voc, case.n_ctx)
    L, T = case.depth, case.T
    wd = {k: v.astype(dtype) for k, v in w.items()}
    st = [inp["states"][:, k].astype(dtype) for k in range(2 * L)]
    om = [None] + [inp["masks"][l].astype(dtype) for l in range(1, L)]
    probs, _st, cache = O.forward_window(cfg, wd, inp["idx"], inp["ctx"], st, om, keep_cache=True, storage=storage)
    count = inp["n_real"] * (1 if case.last_only else T)
    _g, dz = O.backward_window(cfg, wd, inp["idx"], inp["ctx"], inp["tgt"], probs, cache, om, with_regularisers=False,
                               keep_dz=True, storage=storage, count=count)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # (f64 -> f32: 6e-8, far below what is measured here)
    return dict(h=[f32(a) for a in cache["hpre"]], c=[f32(a) for a in cache["c"]], gates=[f32(a) for a in cache["gates"]],
                dz=[f32(a) for a in dz])


def references(case, w, inp, storage=None, tag=None):
    """-> dict of the canonical arrays (lists per layer, f32 copies): the f64 oracle (storage None) or the bf16-storage
    oracle.  Computed once per (case, inputs, storage) and shared (read-only) between the tests that need it -- `tag` names
    inputs that the case and the seed do not determine (carried states).  The few most recent are kept."""
    key = (case.name if tag is None else tag, case[3:9], case.last_only, inp["seed"], None if storage is None else storage.key())
    ref = _ref_cache.get(key)
    if ref is None:
        ref = _window(case, w, inp, np.float64 if storage is None else np.float32, storage)
        for arrs in ref.values():
            for a in arrs:
                a.setflags(write=False)
        _ref_cache[key] = ref
        while len(_ref_cache) > 3:
            _ref_cache.popitem(last=False)
    else:
        _ref_cache.move_to_end(key)
    return ref


def storage_of(view):
    """the rounding points a window's plan chose (a kl_window_view or a dict with its fields)"""
    g = (lambda k: view[k]) if isinstance(view, dict) else (lambda k: getattr(view, k))
    L = g("depth")
    return O.Storage(L, [(g("p_bf16_mask") >> l) & 1 for l in range(L)], g("dh_bf16"), g("c_in_cb"))


# ---------------------------------------------------------------------------------------------- layouts
def _torch():
    import torch
    return torch


def view_dict(view):
    d = {k: getattr(view, k) for k in ("depth", "width", "B", "T", "g_interleaved", "c_in_cb", "dh_bf16", "p_bf16_mask", "scan2_rows")}
    for k in ("wg_route", "wg_pair_mask", "wg_db_scan_mask"):      # (the weight-gradient stage: tests/window_grads.py)
        d[k] = getattr(view, k)
    for k in ("off_H", "off_C", "off_Cb", "off_G", "off_dZ", "off_Hd"):
        d[k] = [int(v) for v in getattr(view, k)[:view.depth]]
    for k in ("out_route", "off_dlogits", "ld_dlogits"):      # (the output layer: tests/table_grads.py)
        d[k] = int(getattr(view, k))
    return d


def _rows(ws, off, dtype, blocks, B, cols):
    torch = _torch()
    size = 2 if dtype == torch.bfloat16 else 4
    return ws[off:off + blocks * B * cols * size].view(dtype).view(blocks, B, cols)


def decode_window(ws, view, width=None, n=None):
    """ws: the uint8 workspace tensor (device or host); view: `view_dict`.  -> canonical numpy arrays, trimmed to the model's
    own `width` and the first `n` streams: h, c [L][n][T][W] (blocks 1..T; c from Cb where the view says so), gates, dz
    [L][n][T][4][W], h0, c0 [L][n][W] (block 0), cT [L][n][W] (block T of the f32 cell states), and `finite`: per array, whether
    every halfword of every row and padded column is a number."""
    torch = _torch()
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    W = Wp if width is None else width
    n = B if n is None else n
    out = {k: [] for k in ("h", "c", "gates", "dz", "h0", "c0", "cT")}
    finite = {k: True for k in ("h", "gates", "dz", "cb")}
    host = lambda t: t.float().cpu().numpy()
    for l in range(L):
        H = _rows(ws, view["off_H"][l], torch.bfloat16, T + 1, B, Wp)
        Cf = _rows(ws, view["off_C"][l], torch.float32, T + 1, B, Wp)
        G = _rows(ws, view["off_G"][l], torch.bfloat16, T, B, 4 * Wp)
        dZ = _rows(ws, view["off_dZ"][l], torch.bfloat16, T, B, 4 * Wp)
        finite["h"] &= bool(torch.isfinite(H[1:].float()).all())
        finite["gates"] &= bool(torch.isfinite(G.float()).all())
        finite["dz"] &= bool(torch.isfinite(dZ.float()).all())
        if view["c_in_cb"]:
            Cb = _rows(ws, view["off_Cb"][l], torch.bfloat16, T + 1, B, Wp)
            finite["cb"] &= bool(torch.isfinite(Cb[1:].float()).all())
            Cs = Cb[1:]
        else:
            Cs = Cf[1:]
        G = G.view(T, B, Wp, 4).permute(0, 1, 3, 2) if view["g_interleaved"] else G.view(T, B, 4, Wp)
        out["h"].append(host(H[1:, :n, :W].permute(1, 0, 2)))
        out["c"].append(host(Cs[:, :n, :W].permute(1, 0, 2)))
        out["gates"].append(host(G[:, :n, :, :W].permute(1, 0, 2, 3)))
        out["dz"].append(host(dZ.view(T, B, 4, Wp)[:, :n, :, :W].permute(1, 0, 2, 3)))
        out["h0"].append(host(H[0, :n, :W]))
        out["c0"].append(host(Cf[0, :n, :W]))
        out["cT"].append(host(Cf[T, :n, :W]))
    out["finite"] = finite
    return out


def decode_hd(ws, view, width=None, n=None):
    """The dropout-masked outputs behind `off_Hd`, per layer: [n][T][W] like `decode_window`'s h (row t * B + b = step t), None
    where the view has none (offset 0: layer 0, a window without masks, a view dict from before the field)."""
    torch = _torch()
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    W = Wp if width is None else width
    n = B if n is None else n
    out = []
    for l in range(L):
        off = view.get("off_Hd", [0] * L)[l]
        out.append(_rows(ws, off, torch.bfloat16, T, B, Wp)[:, :n, :W].permute(1, 0, 2).float().cpu().numpy() if off else None)
    return out


def decode_dlogits(ws, view):
    """The gradient of the logits behind `off_dlogits`: [B*T][Vp] f32, time-major (row t * B + b = step t), every row and padded
    column of it; None for a view from before the field (ld_dlogits 0)"""
    torch = _torch()
    ld = view.get("ld_dlogits", 0)
    if not ld:
        return None
    rows = view["B"] * view["T"]
    off = view["off_dlogits"]
    return ws[off:off + rows * ld * 2].view(torch.bfloat16).view(rows, ld).float().cpu().numpy()


def encode_dlogits(ws, view, dlogits):
    """the inverse of `decode_dlogits`, into a workspace that `encode_window` laid out: [B*T][<= Vp] f32 -> bf16 rows of ld_dlogits"""
    torch = _torch()
    rows, ld, off = view["B"] * view["T"], view["ld_dlogits"], view["off_dlogits"]
    a = np.asarray(dlogits, dtype=np.float32)
    assert a.shape[0] == rows and a.shape[1] <= ld, (a.shape, rows, ld)
    ws[off:off + rows * ld * 2].view(torch.bfloat16).view(rows, ld)[:, :a.shape[1]] = torch.from_numpy(a).to(torch.bfloat16)
    return ws


def window_bytes(view):
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    end = view.get("off_dlogits", 0) + B * T * view.get("ld_dlogits", 0) * 2
    for l in range(L):
        if view.get("off_Hd", [0] * L)[l]:
            end = max(end, view["off_Hd"][l] + T * B * Wp * 2)
        end = max(end, view["off_H"][l] + (T + 1) * B * Wp * 2, view["off_C"][l] + (T + 1) * B * Wp * 4,
                  view["off_Cb"][l] + (T + 1) * B * Wp * 2, view["off_G"][l] + T * B * 4 * Wp * 2, view["off_dZ"][l] + T * B * 4 * Wp * 2)
    return end


def encode_window(arrs, view, fill=0xFF):
    """The inverse of `decode_window` (host tensors): canonical arrays of n <= B streams and width <= the padded width ->
    a workspace laid out as `view` says, everything else -- padded columns, further streams, the unused cell-state blocks --
    filled with `fill` bytes."""
    torch = _torch()
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    ws = torch.full((window_bytes(view),), fill, dtype=torch.uint8)
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))
    for l in range(L):
        n, _T, W = arrs["h"][l].shape
        H = _rows(ws, view["off_H"][l], torch.bfloat16, T + 1, B, Wp)
        Cf = _rows(ws, view["off_C"][l], torch.float32, T + 1, B, Wp)
        G = _rows(ws, view["off_G"][l], torch.bfloat16, T, B, 4 * Wp)
        dZ = _rows(ws, view["off_dZ"][l], torch.bfloat16, T, B, 4 * Wp)
        H[0, :n, :W] = t(arrs["h0"][l]).to(torch.bfloat16)
        H[1:, :n, :W] = t(arrs["h"][l]).permute(1, 0, 2).to(torch.bfloat16)
        Cf[0, :n, :W] = t(arrs["c0"][l])
        Cf[T, :n, :W] = t(arrs["cT"][l])
        if view["c_in_cb"]:
            Cb = _rows(ws, view["off_Cb"][l], torch.bfloat16, T + 1, B, Wp)
            Cb[1:, :n, :W] = t(arrs["c"][l]).permute(1, 0, 2).to(torch.bfloat16)
        else:
            Cf[1:, :n, :W] = t(arrs["c"][l]).permute(1, 0, 2)
        g = t(arrs["gates"][l]).permute(1, 0, 2, 3).to(torch.bfloat16)      # [T][n][4][W]
        if view["g_interleaved"]:
            G.view(T, B, Wp, 4)[:, :n, :W, :] = g.permute(0, 1, 3, 2)
        else:
            G.view(T, B, 4, Wp)[:, :n, :, :W] = g
        dZ.view(T, B, 4, Wp)[:, :n, :, :W] = t(arrs["dz"][l]).permute(1, 0, 2, 3).to(torch.bfloat16)
        if view.get("off_Hd", [0] * L)[l]:
            _rows(ws, view["off_Hd"][l], torch.bfloat16, T, B, Wp)[:, :n, :W] = t(arrs["hd"][l]).permute(1, 0, 2).to(torch.bfloat16)
    return ws


def read_window(lm):
    """The arrays of the engine's last training window (HipLM.window_view): `decode_window`'s dict over ALL streams the kernels
    ran -- the engine's own dummy streams are rows [info['n'], info['B']) -- plus `view` (dict) and `info`.  With stream groups
    the workspace holds the last group only (info['groups'] > 1, its real streams are [first, first + n) of the batch)."""
    view, ws, info = lm.window_view()
    vd = view_dict(view)
    out = decode_window(ws, vd, width=lm.width)
    out["view"], out["info"] = vd, info
    return out


def read_window_padded(lm):
    """... the same at the PADDED width, with the masked outputs (`decode_hd`) as "hd": what the weight-gradient products of
    tests/window_grads.py were computed from, every row and column of it"""
    view, ws, info = lm.window_view()
    vd = view_dict(view)
    out = decode_window(ws, vd)
    out["hd"] = decode_hd(ws, vd)
    out["dlogits"] = decode_dlogits(ws, vd)      # (the output layer's: tests/table_grads.py)
    out["view"], out["info"] = vd, info
    return out


# ---------------------------------------------------------------------------------------------- the tile check
def tile_errors(got, ref, floor_frac=FLOOR_FRAC):
    """got, ref [B][T][...] -> (err [blocks][T], floored [blocks][T]): the tile errors against `ref` and where the floor is
    in force.  A NaN anywhere in a tile makes its error NaN."""
    B, T = ref.shape[:2]
    ref2 = ref.reshape(B, T, -1).astype(np.float64)
    d2 = got.reshape(B, T, -1).astype(np.float64) - ref2
    starts = np.arange(0, B, TILE)
    rows = np.minimum(starts + TILE, B) - starts
    num = np.sqrt(np.add.reduceat((d2 * d2).sum(axis=2), starts, axis=0))
    den = np.sqrt(np.add.reduceat((ref2 * ref2).sum(axis=2), starts, axis=0))
    rms = np.sqrt((ref2 * ref2).mean())
    floor = floor_frac * rms * np.sqrt(rows * ref2.shape[2])[:, None]
    floored = den < floor
    return num / np.maximum(np.maximum(den, floor), 1e-300), floored


def floor_share(ref64, n_real, B):
    """{(array, layer): share of the non-dummy tiles whose f64 norm is below the floor} -- from the f64 oracle alone"""
    skip = dummy_blocks(B, n_real)
    out = {}
    for name in ARRAYS:
        for l, ref in enumerate(ref64[name]):
            _e, floored = tile_errors(ref, ref)
            keep = np.ones(floored.shape[0], dtype=bool)
            if name == "dz":
                keep[skip] = False      # (no target: exactly zero, see exact_checks)
            out[(name, l)] = float(floored[keep].mean())
    return out


def check_tiles(got, ref64, emu, n_real, where=""):
    """Holds every tile of h, c, gates and dz in `got` (canonical arrays over the same streams as the references) to FACTOR x
    the bf16-storage oracle's largest tile error for that array and layer.  Returns {(array, layer): dict(emu_max, worst,
    ratio, at)}; raises AssertionError naming every (array, layer, step, block) beyond its bound."""
    B = ref64["h"][0].shape[0]
    skip = dummy_blocks(B, n_real)
    report, bad = {}, []
    for name in ARRAYS:
        for l in range(len(ref64[name])):
            ref = ref64[name][l]
            e_emu, _f = tile_errors(emu[name][l], ref)
            e_got, _f = tile_errors(got[name][l], ref)
            keep = np.ones(e_emu.shape, dtype=bool)
            if name == "dz":
                keep[skip] = False
            emu_max = float(e_emu[keep].max())
            assert emu_max < EMU_MAX, (where, name, l, "the emulation's own largest tile error", emu_max)
            bound = FACTOR * emu_max
            e = np.where(keep, e_got, 0.0)
            blk, t = np.unravel_index(np.argmax(np.where(np.isnan(e), np.inf, e)), e.shape)
            report[(name, l)] = dict(emu_max=emu_max, worst=float(e[blk, t]), ratio=float(e[blk, t] / emu_max), at=(int(t), int(blk)))
            for b_, t_ in zip(*np.nonzero(~(e <= bound))):      # (NaN fails)
                bad.append((name, "layer %d" % l, "step %d" % t_, "block %d" % b_, "error %.4g" % e[b_, t_], "bound %.4g" % bound))
    assert not bad, (where, "%d tiles beyond their bound" % len(bad), bad[:12])
    return report


def exact_checks(win, states_in, states_out, dummy_from, where=""):
    """The checks without tolerance.  win: `decode_window`'s dict; states_in / states_out [n][2L][W] f32: the state the window's
    first n streams started from and the state it left them in; streams from `dummy_from` on carry no target at all."""
    assert all(win["finite"].values()), (where, "NaN / Inf halfwords (a sentinel that survived?)", win["finite"])
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    n = states_in.shape[0]
    for l in range(len(win["h"])):
        dz = win["dz"][l][dummy_from:]
        assert not dz.any(), (where, "layer %d" % l, "dZ of dummy streams", np.argwhere(dz)[:4])
        h_in, c_in = states_in[:, 2 * l], states_in[:, 2 * l + 1]
        h_out, c_out = states_out[:, 2 * l], states_out[:, 2 * l + 1]
        assert np.array_equal(bits(win["h0"][l][:n]), bits(O.bf16_round(h_in))), (where, "layer %d" % l, "H block 0")
        assert np.array_equal(bits(win["c0"][l][:n]), bits(c_in)), (where, "layer %d" % l, "C block 0")
        assert np.array_equal(bits(win["cT"][l][:n]), bits(c_out)), (where, "layer %d" % l, "C block T against the carried-out state")
        hT = win["h"][l][:n, -1]
        assert (np.abs(hT - h_out) <= np.abs(h_out) * 2.0 ** -8).all(), (where, "layer %d" % l, "H block T against the carried-out state")


def zero_dc_tile(ref, l, t, blk):
    """dz of one tile as a backward scan would write it had it dropped the cell gradient carried in from step t + 1:
    recomputed from the arrays of `ref` (f64 arithmetic; t < T - 1)."""
    rows = slice(blk * TILE, (blk + 1) * TILE)
    gs, dz = ref["gates"][l][rows, t].astype(np.float64), ref["dz"][l][rows, t].astype(np.float64)
    i, f, g, o = gs[:, 0], gs[:, 1], gs[:, 2], gs[:, 3]
    tc = np.tanh(ref["c"][l][rows, t].astype(np.float64))
    safe = lambda num, den: np.where(np.abs(den) > 1e-9, num / np.where(np.abs(den) > 1e-9, den, 1.0), 0.0)
    dh = safe(dz[:, 3], tc * o * (1 - o))
    dc_full = safe(dz[:, 2], i * (1 - g * g))
    dc = dh * o * (1 - tc * tc)
    cprev = safe(safe(dz[:, 1], f * (1 - f)), dc_full)
    out = dz.copy()
    out[:, 0] = dc * g * i * (1 - i)
    out[:, 1] = dc * cprev * f * (1 - f)
    out[:, 2] = dc * i * (1 - g * g)
    return out.astype(np.float32)
