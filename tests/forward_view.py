"""What the scan families of an INFERENCE-layout window (split-precision kl_forward_window, kl_rate_window) leave in the
workspace, held to the oracle per layer and step.

Shared by tests/test_forward_view_ref.py (CPU: decoders, the checker's own sensitivity, the choice of inputs) and
tests/test_forward_view_gpu.py (every family and branch of the dispatch in `forward_impl`, api.hip).

* `CASES`: (depth, width, voc, n_ctx, B, T) with the family, branch masks and hand-off the view must report.  The stream
  counts ASSUME 256 compute units, as SPLIT_ARM_CASES of tests/test_gpu_kernels.py do (the GPU module asserts them).
* `decode_forward` / `encode_forward`: the arrays behind a `kl_forward_view` (include/keraslm_hip.h) <-> canonical numpy
  arrays at the PADDED width, every block: H, C f32 [L][T+1][B][W], Xhi, Xlo uint16 (the bf16 bit patterns) [L][T+1][B][W] or
  None, P1 f32 [T*B][4][W].
* `exact_checks`: no tolerance.  Block 0 of H and C = the carried-in state, block T = the carried-out state, bit for bit;
  with planes: no arming pattern left (`arm_publish` fills 0xFFFF halfwords -- a NaN no published value is, the scans clamp h
  into (-1, 1)), and every block of them is the split of the engine's own H: hi = RNE-bf16(h), lo = RNE-bf16(h - hi), the
  kernel's hx, hh, hl, which are h itself while |h| < 1 (asserted of the engine's H); units beyond the model's own width are
  exactly zero in H, C and both planes.
* `oracle_checks`: H of every (layer, step) and every WRITTEN block of C (all with c_every_step, else block T) against the
  f64 oracle, largest absolute difference: H_C_BOUND[precision] -- 1e-4 in split precision, what test_forward_window_parity
  holds the final state to, 3e-2 in bf16, the state bound of test_validation_windows_bf16.
* `p1_check`: where P1 holds the gate inputs of a layer l >= 1 (fwd_split_layers: one product over all steps per layer),
  P1 against the exact f64 product of what the scan below left: the engine's own f32 H rows of layer l - 1 x f32 K_l + b_l.
  No number is fixed in advance: `p1_emulation` does on the CPU what both branches do -- operands split as the planes and
  KT_hi / KT_lo are (RNE hi, RNE lo of the remainder), the three products hi.hi + b, lo.hi, hi.lo accumulated in np.float32
  and stored as f32 (the thin GEMM issues the same three per k-step) -- and the kernel's largest error may be at most
  FACTOR = 2 x the emulation's largest error (the margin of tests/window_ref.py: the two differ in f32 summation order only;
  what both leave out, lo.lo, is the bulk of either error).  A dropped lo.hi or hi.lo product is two orders beyond that
  (tests/test_forward_view_ref.py plants one).
"""
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import lstm_oracle as O

PAIRS, LAYERS, FUSED, WAVEFRONT = 1, 2, 4, 8          # kl_forward_view.family / .passed_mask (include/keraslm_hip.h)
NONE, SENTINELS, COUNTERS = 0, 1, 2                   # .handoff
FAMILY_NAMES = {PAIRS: "SPLIT_PAIRS", LAYERS: "SPLIT_LAYERS", FUSED: "SPLIT_FUSED", WAVEFRONT: "WAVEFRONT"}
PREC_BF16, PREC_SPLIT = 1, 3
H_C_BOUND = {PREC_SPLIT: 1e-4, PREC_BF16: 3e-2}
PROBS_BOUND = 2e-5
FACTOR = 2.0
SENTINEL = 0xFFFF

Case = namedtuple("Case", "name env depth width voc n_ctx B T precision abi family passed ring thin handoff planes p1_layer")


def _case(name, shape, family, env=(), precision=PREC_SPLIT, abi=False, passed=0, ring=0, thin=0, handoff=SENTINELS, planes=True,
          p1_layer=0):
    return Case(name, dict(env), *shape, precision, abi, family, passed, ring, thin, handoff, planes, p1_layer)


# shape = (depth, width, voc, n_ctx, B, T).  abi: run through the library on a workspace of the test's own (the engine would
# split 272 streams into groups, and gives a bf16 window the training-size workspace)
CASES = [
    _case("pairs", (2, 1024, 40, 1, 20, 5), PAIRS),
    _case("pair-and-single", (3, 1024, 40, 1, 20, 3), PAIRS),
    # five layers: the pairs launch layers 0..3, then hand the window on; it is redone from layer 0 over planes the pairs armed and published
    _case("pairs-hand-on", (5, 1024, 30, 1, 20, 3), LAYERS, passed=PAIRS, thin=0b11110, p1_layer=4),
    _case("split8-off", (2, 1024, 40, 1, 20, 5), LAYERS, env={"KL_SPLIT8": "0"}, thin=0b10, p1_layer=1),
    _case("thin-2047-rows", (2, 1024, 40, 1, 89, 23), LAYERS, thin=0b10, p1_layer=1),
    _case("ring-2048-rows", (2, 1024, 40, 1, 64, 32), LAYERS, ring=0b10, p1_layer=1),
    _case("ring-ragged-two-contexts", (2, 1024, 40, 2, 48, 43), LAYERS, ring=0b10, p1_layer=1),
    _case("ring-16-row-blocks-p1-reused", (3, 1024, 40, 1, 256, 8), LAYERS, ring=0b110, p1_layer=2),
    _case("ring-partial-row-block-no-context", (2, 1024, 30, 0, 250, 9), LAYERS, ring=0b10, p1_layer=1),
    # 17 row blocks: beyond fwd_split_layers; the fused family splits and arms the planes before its launcher refuses the shape
    _case("beyond-16-row-blocks", (1, 1024, 30, 1, 272, 2), WAVEFRONT, abi=True, passed=FUSED, handoff=NONE, planes=False),
    _case("fused-sentinels", (3, 256, 30, 2, 40, 9), FUSED),
    _case("fused-counters", (3, 256, 30, 2, 40, 9), FUSED, env={"KL_SPLIT_SENTINEL": "0"}, handoff=COUNTERS),
    _case("padded-width", (2, 100, 50, 1, 3, 12), FUSED),
    _case("deeper-than-maxl", (6, 128, 30, 1, 5, 9), WAVEFRONT, handoff=NONE, planes=False),
    _case("scan-off", (2, 128, 40, 1, 20, 5), WAVEFRONT, env={"KL_SCAN": "0"}, handoff=NONE, planes=False),
    _case("bf16-inference-workspace", (2, 128, 40, 1, 20, 5), WAVEFRONT, precision=PREC_BF16, abi=True, handoff=NONE, planes=False),
]
RING_CASE = next(c for c in CASES if c.name == "ring-2048-rows")
# the shapes the suite ran before this module existed at width 1024 in split precision (test_forward_window_parity,
# test_rate_window_is_forward_window_picked): what the view says of them is asserted too -- none reaches the ring branch
OLD_SHAPES = [
    _case("old-4x1024-2x6", (4, 1024, 64, 2, 2, 6), PAIRS),
    _case("old-3x1024-20x5", (3, 1024, 40, 1, 20, 5), PAIRS),
    _case("old-2x1024-5x7", (2, 1024, 96, 1, 5, 7), PAIRS),
    _case("old-1x1024-65x3", (1, 1024, 30, 1, 65, 3), LAYERS),
    _case("old-2x1024-40x4", (2, 1024, 40, 1, 40, 4), LAYERS, thin=0b10, p1_layer=1),
]


def physical_width(width):
    for w in (64, 128, 256, 512, 1024):
        if width <= w:
            return w
    return (width + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(case, seed=31, states=None):
    """One window of `case`: indices, contexts, targets (a -1 tail) and NON-ZERO carried-in states [B][2L][W] f32 (`states`
    overrides the drawn ones): h within (-0.95, 0.95) -- an output of o * tanh(c) --, c of standard deviation 0.5."""
    rng = np.random.default_rng(seed)
    L, W, V, B, T = case.depth, case.width, case.voc, case.B, case.T
    idx = rng.integers(0, V, (B, T))
    ctx = rng.integers(0, 200, (B, 1, case.n_ctx)).repeat(T, axis=1)
    tgt = rng.integers(0, V, (B, T))
    tgt[:, -1:] = -1
    drawn = (rng.standard_normal((B, 2 * L, W)) * 0.5).astype(np.float32)
    drawn[:, 0::2] = np.clip(0.6 * drawn[:, 0::2], -0.95, 0.95)
    return dict(idx=idx, ctx=ctx, tgt=tgt, states=drawn if states is None else np.asarray(states, dtype=np.float32), seed=seed)


# ---------------------------------------------------------------------------------------------- references
_ref_cache = OrderedDict()


def references(case, w, inp, tag=None):
    """The f64 oracle over one window: dict(probs [B][T][V], h, c [L][B][T][W], states [B][2L][W]) -- computed once per (shape,
    inputs) and shared read-only; `tag` names inputs the case and the seed do not determine (carried states)."""
    key = (tag, case[2:8], inp["seed"])
    ref = _ref_cache.get(key)
    if ref is None:
        cfg = O.ModelConfig(case.depth, case.width, case.voc, case.n_ctx)
        w64 = {k: v.astype(np.float64) for k, v in w.items()}
        st = [inp["states"][:, k].astype(np.float64) for k in range(2 * case.depth)]
        probs, st_out, cache = O.forward_window(cfg, w64, inp["idx"], inp["ctx"], st, keep_cache=True)
        ref = dict(probs=probs, h=cache["hpre"], c=cache["c"], states=np.stack(st_out, axis=1))
        for v in (ref["probs"], ref["states"], *ref["h"], *ref["c"]):
            v.setflags(write=False)
        _ref_cache[key] = ref
        while len(_ref_cache) > 2:
            _ref_cache.popitem(last=False)
    return ref


# ---------------------------------------------------------------------------------------------- the split
def bf16_bits(x):
    """RNE f32 -> bf16, as uint16 bit patterns"""
    return (O.bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def bits_f32(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def split_planes(x):
    """f32 -> (hi, lo) uint16 bit patterns: hi = RNE-bf16(x), lo = RNE-bf16(x - hi)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_bits(x)
    return hi, bf16_bits(x - bits_f32(hi))


# ---------------------------------------------------------------------------------------------- layouts
def view_dict(view):
    d = {k: int(getattr(view, k)) for k in ("depth", "width", "B", "T", "family", "passed_mask", "ring_mask", "thin_mask", "handoff",
                                             "c_every_step", "precision", "p1_layer")}
    for k in ("off_H", "off_C", "off_Xhi", "off_Xlo"):
        d[k] = [int(v) for v in getattr(view, k)[:view.depth]]
    d["off_P1"] = int(view.off_P1)
    return d


def _region(ws, off, n):
    part = ws[off:off + n]
    return part if isinstance(part, np.ndarray) else part.cpu().numpy()      # (a device tensor: this region alone is copied)


def has_planes(view):
    return view["off_Xhi"][0] != 0


def decode_forward(ws, view):
    """ws: the uint8 workspace (numpy array, or a host / device torch tensor); view: `view_dict` -> the canonical arrays"""
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    n = (T + 1) * B * Wp
    f32 = lambda off: _region(ws, off, n * 4).view(np.float32).reshape(T + 1, B, Wp).copy()
    u16 = lambda off: _region(ws, off, n * 2).view(np.uint16).reshape(T + 1, B, Wp).copy()
    out = dict(H=[f32(view["off_H"][l]) for l in range(L)], C=[f32(view["off_C"][l]) for l in range(L)], Xhi=None, Xlo=None)
    if has_planes(view):
        out["Xhi"] = [u16(view["off_Xhi"][l]) for l in range(L)]
        out["Xlo"] = [u16(view["off_Xlo"][l]) for l in range(L)]
    out["P1"] = _region(ws, view["off_P1"], T * B * 4 * Wp * 4).view(np.float32).reshape(T * B, 4, Wp).copy()
    return out


def window_bytes(view):
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    n = (T + 1) * B * Wp
    end = view["off_P1"] + T * B * 4 * Wp * 4
    for l in range(L):
        end = max(end, view["off_H"][l] + n * 4, view["off_C"][l] + n * 4)
        if has_planes(view):
            end = max(end, view["off_Xhi"][l] + n * 2, view["off_Xlo"][l] + n * 2)
    return end


def encode_forward(arrs, view, fill=0xFF):
    """the inverse of `decode_forward`: a numpy uint8 workspace laid out as `view` says, everything else `fill` bytes"""
    L = view["depth"]
    ws = np.full(window_bytes(view), fill, dtype=np.uint8)

    def put(off, a, dtype):
        raw = np.ascontiguousarray(a, dtype=dtype).reshape(-1).view(np.uint8)
        ws[off:off + raw.size] = raw
    put(view["off_P1"], arrs["P1"], np.float32)
    for l in range(L):
        put(view["off_H"][l], arrs["H"][l], np.float32)
        put(view["off_C"][l], arrs["C"][l], np.float32)
        if has_planes(view):
            put(view["off_Xhi"][l], arrs["Xhi"][l], np.uint16)
            put(view["off_Xlo"][l], arrs["Xlo"][l], np.uint16)
    return ws


def synthetic_view(depth, Wp, B, T, planes=True, family=LAYERS, p1_layer=None, precision=PREC_SPLIT, c_every_step=0):
    """a view dict with the arrays carved as carve_window does (256-byte aligned, P1 first), 512 bytes of nothing between them"""
    off = [0]

    def take(n):
        at = off[0]
        off[0] = (at + n + 512 + 255) // 256 * 256
        return at
    n = (T + 1) * B * Wp
    v = dict(depth=depth, width=Wp, B=B, T=T, family=family, passed_mask=0, ring_mask=0, thin_mask=0, handoff=SENTINELS,
             c_every_step=c_every_step, precision=precision, p1_layer=depth - 1 if p1_layer is None else p1_layer)
    v["off_P1"] = take(T * B * 4 * Wp * 4)
    v["off_H"], v["off_C"] = [], []
    for _l in range(depth):
        v["off_H"].append(take(n * 4))
        v["off_C"].append(take(n * 4))
    v["off_Xhi"] = [take(n * 2) if planes else 0 for _l in range(depth)]
    v["off_Xlo"] = [take(n * 2) if planes else 0 for _l in range(depth)]
    return v


# ---------------------------------------------------------------------------------------------- checks
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def written_c_blocks(view):
    return list(range(1, view["T"] + 1)) if view["c_every_step"] else [view["T"]]


def exact_checks(win, view, states_in, states_out, width, where=""):
    """The checks without tolerance.  win: `decode_forward`'s dict; states_in / states_out [B][2L][width] f32: what the window
    started from and what it left in the state buffer; width: the model's own (<= the padded width of the arrays)."""
    L, T = view["depth"], view["T"]
    for l in range(L):
        H, C = win["H"][l], win["C"][l]
        at = (where, "layer %d" % l)
        assert np.array_equal(_bits(H[0][:, :width]), _bits(states_in[:, 2 * l])), at + ("H block 0 is not the carried-in state",)
        assert np.array_equal(_bits(C[0][:, :width]), _bits(states_in[:, 2 * l + 1])), at + ("C block 0 is not the carried-in state",)
        assert np.array_equal(_bits(H[T][:, :width]), _bits(states_out[:, 2 * l])), at + ("H block T is not the carried-out state",)
        assert np.array_equal(_bits(C[T][:, :width]), _bits(states_out[:, 2 * l + 1])), at + ("C block T is not the carried-out state",)
        assert not H[:, :, width:].any(), at + ("H: non-zero padded unit", np.argwhere(H[:, :, width:])[:4])
        blocks = [0] + written_c_blocks(view)
        assert not C[blocks][:, :, width:].any(), at + ("C: non-zero padded unit", np.argwhere(C[blocks][:, :, width:])[:4])
        if win["Xhi"] is None:
            continue
        hi, lo = win["Xhi"][l], win["Xlo"][l]
        for name, plane in (("Xhi", hi), ("Xlo", lo)):
            left = np.argwhere(plane == SENTINEL)
            assert not len(left), at + ("%s: arming pattern left in %d halfwords" % (name, len(left)), "(block, stream, unit)", left[:4])
            assert not plane[:, :, width:].any(), at + ("%s: non-zero padded unit" % name, np.argwhere(plane[:, :, width:])[:4])
        assert (np.abs(H[1:]) < 1.0).all(), at + ("|h| >= 1: the scan's clamp applies, the planes are not the split of H",)
        want_hi, want_lo = split_planes(H)
        bad = np.argwhere(hi != want_hi)
        assert not len(bad), at + ("Xhi is not RNE-bf16(H) in %d places" % len(bad), "(block, stream, unit)", bad[:4])
        bad = np.argwhere(lo != want_lo)
        assert not len(bad), at + ("Xlo is not RNE-bf16(H - Xhi) in %d places" % len(bad), "(block, stream, unit)", bad[:4])


def oracle_checks(win, view, ref, width, where=""):
    """H of every (layer, step) and every written block of C against the f64 oracle -> (largest |dH|, largest |dC|); raises
    naming the worst (layer, step) beyond H_C_BOUND[precision]"""
    bound = H_C_BOUND[view["precision"]]
    worst, bad = {"H": 0.0, "C": 0.0}, []
    for l in range(view["depth"]):
        for name, got, want, blocks in (("H", win["H"][l], ref["h"][l], range(1, view["T"] + 1)),
                                        ("C", win["C"][l], ref["c"][l], written_c_blocks(view))):
            for blk in blocks:
                d = np.abs(got[blk][:, :width].astype(np.float64) - want[:, blk - 1])
                e = float(np.where(np.isnan(d), np.inf, d).max())
                worst[name] = max(worst[name], e)
                if not e <= bound:
                    bad.append((name, "layer %d" % l, "step %d" % (blk - 1), "stream %d" % int(np.argmax(d.max(axis=1))), "error %.3g" % e))
    assert not bad, (where, "%d (layer, step) blocks beyond %.3g" % (len(bad), bound), bad[:12])
    return worst["H"], worst["C"]


def p1_products(rows, K, b):
    """rows f32 [M][W], K f32 [W][4W], b f32 [4W] -> (the exact f64 product [M][4W], what the split-precision branches compute)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    exact = rows.astype(np.float64) @ K.astype(np.float64) + b.astype(np.float64)
    return exact, p1_emulation(rows, K, b)


def p1_emulation(rows, K, b, drop=()):
    """hi.hi + b, then + lo.hi, then + hi.lo -- operands split as the planes and KT_hi / KT_lo are, f32 accumulation, f32 result.
    drop: products left out ("lo.hi", "hi.lo": the planted errors of tests/test_forward_view_ref.py)."""
    hi, lo = (bits_f32(p) for p in split_planes(rows))
    k_hi, k_lo = (bits_f32(p) for p in split_planes(K))
    out = hi @ k_hi + b.astype(np.float32)
    if "lo.hi" not in drop:
        out += lo @ k_hi
    if "hi.lo" not in drop:
        out += hi @ k_lo
    return out.astype(np.float32)


def p1_check(win, view, w, width, where=""):
    """P1 against the products of what the scan below left (see the module text) -> dict(layer, emu_max, worst, ratio), or None
    where P1 holds layer 0's gathered rows (no layer below)"""
    l = view["p1_layer"]
    if l < 1:
        return None
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    assert l < L and ((view["ring_mask"] | view["thin_mask"]) >> l) & 1, (where, "p1_layer %d without a product noted for it" % l)
    rows = win["H"][l - 1][1:, :, :width].reshape(T * B, width)
    exact, emu = p1_products(rows, w["K%d" % l], w["b%d" % l])
    got = win["P1"][:, :, :width].reshape(T * B, 4 * width).astype(np.float64)
    assert not win["P1"][:, :, width:].any(), (where, "P1: non-zero padded unit")
    emu_max = float(np.abs(emu.astype(np.float64) - exact).max())
    assert np.isfinite(emu_max) and emu_max > 0.0, (where, "the emulation's own largest error", emu_max)
    d = np.abs(got - exact)
    worst = float(np.where(np.isnan(d), np.inf, d).max())
    r, col = np.unravel_index(np.argmax(np.where(np.isnan(d), np.inf, d)), d.shape)
    assert worst <= FACTOR * emu_max, (where, "P1 of layer %d" % l, "largest error %.4g at (step %d, stream %d, column %d)" % (worst, r // B, r % B, col),
                                       "emulation's %.4g" % emu_max, "ratio %.2f > %.1f" % (worst / emu_max, FACTOR))
    return dict(layer=l, emu_max=emu_max, worst=worst, ratio=worst / emu_max)


def check_window(win, view, w, inp, states_out, ref, width, where=""):
    """every check of this module over one decoded window -> dict(h, c: largest errors against the oracle, p1: `p1_check`'s)"""
    exact_checks(win, view, inp["states"], states_out, width, where)
    h, c = oracle_checks(win, view, ref, width, where)
    return dict(h=h, c=c, p1=p1_check(win, view, w, width, where))
