"""The contract of ONE incremental step (kl_step_batch, kl_step_batch_host), as buffers that show when it is broken, two
references, a checker, a fault catalogue and the case table.  numpy only (no GPU, no torch): tests/test_step_contract_ref.py turns the
checker and the bounds on the numpy model with planted faults and asks the library which route every case takes,
tests/test_step_contract_gpu.py runs the cases on the kernels.

Buffers (build):
  * the pool has more slots than the call uses.  The slots rows start from (`slot_in`, fewer than rows: parents repeat)
    hold random states, |h| < 1 and c ~ N(0, 0.5), non-zero, zero in padded hidden units; every other slot -- the slots
    the call writes (`slot_out`, scattered over the pool), one "trap" slot and a few bystanders -- holds the f32 marker
    0x7fc0beef, a NaN;
  * probs is [n + 64][V] of the marker (the host entry's delivery buffer likewise);
  * idx, ctx, slot_in, slot_out have n entries inside arrays of n + 64: the tail holds valid values, the slot arrays'
    tails point at the trap slot, so that a row read past n computes NaN inside the allocation and nothing faults;
  * every case with two rows or more holds idx 0 and V - 1, ctx 0 and ctx_vocab - 1; no index is out of range.

Model reference (model_layers, model_output): the f64 value of the arithmetic the precision defines, from the rounded
operands.  State rows (f32) are split into bf16 hi + lo by round-to-nearest-even, the weights likewise (U^T, K^T, E as
kl_prepare keeps them); split precision sums a_hi w_hi + a_lo w_hi + a_hi w_lo, bf16 precision a_hi w_hi alone.  Layer
0 adds EK[idx] + sum_n CtxK_n[ctx_n] + b_0 -- f32 tables, here as read back from the device (tests/test_derived_gpu.py
holds them to their definitions) --, layer l > 0 contracts [h_{l-1} new | h_l] against [K_l ; U_l] and adds b_l; the
output layer contracts the new top-layer h AS STORED in f32 against the E planes.  Read off the kernels, route by
route: inc_tile_kernel, inc_cell_kernel (both widths classes, device and kernel-argument indices), the fused and the
plain gather + GEMM ([hi | lo | hi] rows against [hi | hi | lo] weights) and the thin kernel (f32 A: it splits the row
itself) all issue exactly these three MFMA terms, so does every output route -- the model takes no route argument.  The
routes differ in what f32 leaves open: the order of the K sum, the order in which table rows and bias join it (gathered
first where n_ctx != 1), and the gate functions -- expf / tanhf / IEEE division in the GEMM and thin routes, the
hardware's exp2 and reciprocal (1 ulp each) as 1 / (1 + 2^(-x log2 e)) and 2 / (1 + 2^(-2 x log2 e)) - 1 in the tile and
cell kernels.

True reference: oracle.lstm_oracle.step_batch in f64 from the f32 parameters (logical width).

Tolerance of the model comparison (bounds): E32 = the largest deviation from the model of f32 emulations of the same
arithmetic on a sample of the case's rows -- every layer against the model fed the rows the emulation stored below it
(model_layers: `stored`), as the checker feeds it the device's -- numpy float32 accumulation in ascending, descending and 32-blocked k order
with exact bf16 products, f32 gate math in the library form and in the hardware form with both 1-ulp instructions off
by one ulp upwards and downwards.  tol = 8 E32, separately for states (absolute, h and c of all layers) and
probabilities (relative to the model's value; the model's output layer is fed the h the emulation / the device
stored, so this isolates the output layer).  Nothing in it comes from the kernels' results.

check(): the promises in order -- "slots" (every slot not in slot_out bit for bit as before, trap and parents included),
"probs-tail" (rows from n on bit for bit the marker), "finite" (no NaN / Inf in the written slots' 2 L W entries or in
probs[:n]), "padding" (padded hidden units exactly zero), "model" (h, c absolute, probabilities relative, rows sum to
1 within 1e-5), "true" (split precision: 2e-5 on probabilities, 1e-4 on states against the true reference)."""
import contextlib
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests import derived_ref as D
from tests.gemm_contract import bits_to_f32

PREC_BF16, PREC_SPLIT = 1, 3
MARK_F32 = 0x7FC0BEEF
GUARD = 64
CTX_VOCAB, CTX_DIM = 200, 10
PROMISES = ("slots", "probs-tail", "finite", "padding", "model", "true")
TRUE_PROBS, TRUE_STATES = 2e-5, 1e-4          # the project's standing bounds (split precision)
ROW_SUM = 1e-5
TOL_FACTOR = 8                                # tol = TOL_FACTOR * E32; the weakest fault has to reach TOL_FACTOR * tol
SAMPLE_ROWS = 8                               # rows of a case the f32 emulations run on
FAULT_ROWS = 32                               # ... and the fault catalogue

# kl_step_route (include/keraslm_hip.h)
TILES, CELLS, GEMM_FUSED, GEMM_PLAIN, THIN = 1, 2, 3, 4, 5
OUT_FUSED, OUT_THIN, OUT_BIG = 1, 2, 3
IDX_DEVICE, IDX_KERNARG, IDX_PACKED = 1, 2, 3
LAYER_ROUTES = {TILES: "tiles", CELLS: "cells", GEMM_FUSED: "gemm-fused", GEMM_PLAIN: "gemm-plain", THIN: "thin"}
OUT_ROUTES = {OUT_FUSED: "out_softmax", OUT_THIN: "thin GEMM + softmax", OUT_BIG: "big GEMM + softmax"}
IDX_ROUTES = {IDX_DEVICE: "device arrays", IDX_KERNARG: "kernel arguments", IDX_PACKED: "packed copy"}


# ---------------------------------------------------------------- models and cases
@dataclass(frozen=True)
class Model:
    depth: int
    width: int              # logical; 100 and 200 run zero-padded at 128 and 256
    V: int
    n_ctx: int
    scale: float = 1.5      # weights ~ N(0, scale / sqrt(fan-in))

    @property
    def pwidth(self):
        return {100: 128, 200: 256}.get(self.width, self.width)

    @property
    def shape(self):
        return D.Shape(self.depth, self.pwidth, self.V, self.n_ctx, CTX_VOCAB, CTX_DIM)

    @property
    def name(self):
        return "d%dw%dv%dc%d" % (self.depth, self.width, self.V, self.n_ctx)


M64 = Model(2, 64, 50, 1)
M128 = Model(2, 128, 60, 1)
M256 = Model(2, 256, 40, 1)
M512 = Model(2, 512, 256, 1)
M512C2 = Model(2, 512, 230, 2)
M768 = Model(2, 768, 50, 0)
M1024 = Model(2, 1024, 64, 1)
M100 = Model(2, 100, 50, 1)
M200 = Model(2, 200, 50, 1)
M128V = Model(2, 128, 1100, 1)
M512V = Model(2, 512, 300, 1)
M128D1 = Model(1, 128, 40, 1)
M256D3 = Model(3, 256, 40, 2)
MODELS = (M64, M128, M256, M512, M512C2, M768, M1024, M100, M200, M128V, M512V, M128D1, M256D3)
# width 1280: layer 0 (K = 1280) fits inc_cell_kernel's LDS, layer 1 (K = 2560) does not, so below the tile kernel's
# first row count the whole step is the thin kernel's (kl_step_batch used to launch layer 0 and then return KL_ERR_SHAPE)
M1280 = Model(2, 1280, 64, 1)
ALL_MODELS = MODELS + (M1280,)


@dataclass(frozen=True)
class Case:
    model: Model
    n: int
    layers: int                     # the route the case must take: kl_step_route.layers
    out: int = OUT_THIN
    idx: int = IDX_DEVICE
    nmt: tuple = ()                 # cells: row tiles per workgroup, per layer
    gen: int = 0                    # cells: the instantiation for widths 64 / 128
    tile: tuple = (0, 0, 0)         # tiles: rows per tile, px, py
    env: tuple = ()                 # KL_* switches in force when the handle is bound
    ws: bool = True                 # a step workspace is passed
    host: bool = False              # kl_step_batch_host
    by_target: bool = False         # host: the per-target pick instead of whole rows
    head_k: int = 0                 # host: state vectors delivered with the probabilities

    @property
    def name(self):
        s = "%s-n%d" % (self.model.name, self.n)
        if self.host:
            s += "-host%s-k%d" % ("-pick" if self.by_target else "", self.head_k)
        if not self.ws:
            s += "-nows"
        for k, v in self.env:
            s += "-%s=%s" % (k[3:], v)
        return s

    @property
    def route_name(self):
        s = LAYER_ROUTES[self.layers]
        if self.layers == CELLS:
            s += " nmt %s%s" % ("/".join(map(str, self.nmt)), " gen" if self.gen else "")
        if self.layers == TILES:
            s += " %d rows, px %d py %d" % self.tile
        return "%s; %s; %s" % (s, OUT_ROUTES[self.out], IDX_ROUTES[self.idx])


def _cells(m, n, nmt, **kw):
    return Case(m, n, CELLS, nmt=(nmt,) * m.depth if isinstance(nmt, int) else nmt, gen=int(m.pwidth in (64, 128)), **kw)


def _tiles(m, n, rows, px, py, **kw):
    return Case(m, n, TILES, tile=(rows, px, py), **kw)


DEVICE_CASES = (
    # width 64: the 16-unit cell kernel, GEN instantiation, at every row count; no fused output layer at this width
    Case(M64, 1, THIN), _cells(M64, 16, 1), _cells(M64, 129, 2), _cells(M64, 513, 2),
    # width 128
    Case(M128, 15, THIN), _cells(M128, 17, 1), _cells(M128, 33, 1), _cells(M128, 257, 2), _cells(M128, 512, 2, out=OUT_FUSED),
    # width 256: cells below 256 rows, tiles from there on
    _cells(M256, 32, 1), _cells(M256, 255, 2), _tiles(M256, 256, 64, 4, 2), _tiles(M256, 449, 64, 4, 2),
    _tiles(M256, 511, 64, 4, 2),
    # width 512, V = 256: every threshold
    _cells(M512, 16, 1), _cells(M512, 128, 1), _cells(M512, 129, 2), _cells(M512, 255, 2), _tiles(M512, 256, 64, 8, 1),
    _tiles(M512, 257, 64, 8, 1), _tiles(M512, 320, 64, 8, 1), _tiles(M512, 511, 64, 4, 2),
    _tiles(M512, 512, 64, 4, 2, out=OUT_FUSED), _tiles(M512, 513, 64, 8, 1, out=OUT_FUSED),
    # two context variables: layer 0's gate inputs gathered into the workspace first
    _cells(M512C2, 17, 1), _tiles(M512C2, 300, 64, 8, 1),
    # width 768, no context: layer 0 with two row tiles per workgroup, layer 1 (K = 1536) with one
    _cells(M768, 200, (2, 1)), _tiles(M768, 256, 64, 8, 1),
    # width 1024: tiles already from 129 rows; 1030 rows: 128-row tiles, the last of 6 rows
    _cells(M1024, 128, 1), _tiles(M1024, 129, 64, 8, 1), _tiles(M1024, 1030, 128, 8, 1, out=OUT_FUSED),
    # zero-padded widths
    _cells(M100, 33, 1), _cells(M200, 129, 2), _tiles(M200, 257, 64, 8, 1),
    # 1100 characters: no fused output layer; from 256 rows the plain gather + GEMM and the big output GEMM, without a
    # workspace the thin kernel at many rows
    _cells(M128V, 64, 1), Case(M128V, 256, GEMM_PLAIN, out=OUT_BIG), Case(M128V, 256, THIN, ws=False),
    # 300 characters: tiles, but the output layer in two launches
    _tiles(M512V, 512, 64, 4, 2),
    # depth 1 and depth 3
    _cells(M128D1, 16, 1), _cells(M128D1, 129, 2), _cells(M256D3, 33, 1), _tiles(M256D3, 256, 64, 4, 2),
    # the switches
    _tiles(M512, 320, 128, 8, 1, env=(("KL_TILE_ROWS", "128"),)),
    _cells(M512, 300, 2, env=(("KL_INC_TILE", "0"),)),
    Case(M512, 256, GEMM_FUSED, env=(("KL_INC_TILE", "0"), ("KL_INC_SMALL", "0"))),
    _tiles(M512, 512, 64, 4, 2, env=(("KL_OUT_FUSED", "0"),)),
    _cells(M512, 64, 1, out=OUT_FUSED, env=(("KL_OUT_FUSED_MIN", "16"),)),
    Case(M1280, 64, THIN),
)

HOST_CASES = (
    # indices in the kernel arguments: whole rows and the per-target pick alternating, head_k 0 and depth
    _cells(M512, 1, 1, idx=IDX_KERNARG, host=True),
    _cells(M512, 16, 1, idx=IDX_KERNARG, host=True, by_target=True, head_k=2),
    _cells(M128, 17, 1, idx=IDX_KERNARG, host=True, head_k=2),
    _cells(M512, 128, 1, idx=IDX_KERNARG, host=True, by_target=True),
    _cells(M512, 129, 2, idx=IDX_KERNARG, host=True),
    _cells(M512, 256, 2, idx=IDX_KERNARG, host=True, by_target=True, head_k=2),
    _cells(M1024, 128, 1, idx=IDX_KERNARG, host=True, head_k=2),
    # the packed copy and the device-pointer step
    _tiles(M512, 257, 64, 8, 1, idx=IDX_PACKED, host=True, by_target=True),
    _tiles(M1024, 129, 64, 8, 1, idx=IDX_PACKED, host=True, head_k=2),
    _tiles(M256, 449, 64, 4, 2, idx=IDX_PACKED, host=True),
    _cells(M512C2, 17, 1, idx=IDX_PACKED, host=True, by_target=True, head_k=2),
    _cells(M512, 64, 1, idx=IDX_PACKED, host=True, head_k=2, env=(("KL_HOST_KERNARG", "0"),)),
    Case(M1280, 64, THIN, idx=IDX_PACKED, host=True, by_target=True),
)
ALL_CASES = DEVICE_CASES + HOST_CASES


def route_fields(case):
    """the kl_step_route a case's table entry names, as a dict of its fields (nmt / gen: per layer)"""
    L = case.model.depth
    cells = case.layers == CELLS
    return {"layers": case.layers, "out": case.out, "idx": case.idx, "gathered": int(case.model.n_ctx != 1 and case.idx != IDX_KERNARG),
            "depth": L, "tile_rows": case.tile[0], "px": case.tile[1], "py": case.tile[2],
            "nmt": tuple(case.nmt) if cells else (0,) * L, "gen": (case.gen,) * L if cells else (0,) * L}


def route_of(view, depth):
    """the same dict from a kl_step_route structure"""
    return {"layers": view.layers, "out": view.out, "idx": view.idx, "gathered": view.gathered, "depth": view.depth,
            "tile_rows": view.tile_rows, "px": view.px, "py": view.py,
            "nmt": tuple(view.nmt[l] for l in range(depth)), "gen": tuple(view.gen[l] for l in range(depth))}


# the switches of the step's dispatch (api.hip: kl_bind reads them)
STEP_SWITCHES = ("KL_TILE_ROWS", "KL_INC_TILE", "KL_INC_SMALL", "KL_INC_SMALL_MIN", "KL_FUSED_STEP", "KL_OUT_FUSED",
                 "KL_OUT_FUSED_MIN", "KL_HOST_KERNARG")


@contextlib.contextmanager
def switches(env):
    """the KL_* switches of a case, and none of the others, in the environment while a handle is bound"""
    old = {k: os.environ.pop(k, None) for k in STEP_SWITCHES}
    os.environ.update(dict(env))
    try:
        yield
    finally:
        for k in STEP_SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


# ---------------------------------------------------------------- parameters
def _seed(*parts):
    return zlib.crc32(("/".join(str(p) for p in parts)).encode())


def logical_weights(m, seed=0):
    """f32 weights in Keras shapes, every entry many ulps of what a fault would lose: embeddings ~ N(0, 2 / sqrt(W)) and
    N(0, 0.5), K and U ~ N(0, scale / sqrt(fan-in)), biases ~ N(0, 0.3) with the forget gate's at + 1"""
    rng = np.random.default_rng(_seed("weights", m.name, seed))
    W = m.width
    w = {"E": rng.standard_normal((m.V, W)) * (2.0 / np.sqrt(W))}
    for k in range(m.n_ctx):
        w["Ctx%d" % k] = rng.standard_normal((CTX_VOCAB, CTX_DIM)) * 0.5
    for l in range(m.depth):
        rows = W + CTX_DIM * m.n_ctx if l == 0 else W
        w["K%d" % l] = rng.standard_normal((rows, 4 * W)) * (m.scale / np.sqrt(rows))
        w["U%d" % l] = rng.standard_normal((W, 4 * W)) * (m.scale / np.sqrt(W))
        b = rng.standard_normal(4 * W) * 0.3
        b[W:2 * W] += 1.0
        w["b%d" % l] = b
    return {k: v.astype(np.float32) for k, v in w.items()}


def physical_params(m, w):
    """the flat parameter vector at the physical width: hidden units from `width` on are zero in every row, column and
    bias (K0: the context rows sit behind the padded embedding rows)"""
    W, Wp = m.width, m.pwidth
    lay, total = D.layout(m.shape)
    flat = np.zeros(total, dtype=np.float32)
    for name, (off, rows, cols) in lay.items():
        a = w[name]
        out = np.zeros((rows, cols), dtype=np.float32)
        if name.startswith("Ctx"):
            out[:] = a
        elif name == "E":
            out[:, :W] = a
        elif name.startswith("b"):
            for g in range(4):
                out[0, g * Wp:g * Wp + W] = a[g * W:(g + 1) * W]
        else:
            r = np.arange(a.shape[0])
            if name == "K0":
                r = np.where(r < W, r, r + (Wp - W))
            for g in range(4):
                out[r, g * Wp:g * Wp + W] = a[:, g * W:(g + 1) * W]
        flat[off:off + rows * cols] = out.reshape(-1)
    return flat


def _planes(x):
    """f64 hi and lo of an f32 array split as kl_prepare and the kernels split (derived_ref.split)"""
    hi, lo = D.split(x)
    return bits_to_f32(hi).astype(np.float64).reshape(x.shape), bits_to_f32(lo).astype(np.float64).reshape(x.shape)


@dataclass
class Operands:
    """what the model reference reads: per layer the [K_l][4W] planes of [K_l ; U_l] (layer 0: U_0 alone), the E planes
    [V][W], the f32 tables and biases"""
    m: Model
    w_hi: list
    w_lo: list
    e_hi: np.ndarray
    e_lo: np.ndarray
    EK: np.ndarray
    CtxK: list
    b: list


def operands(m, flat, EK, CtxK):
    wp = D.weights(m.shape, flat)
    Wp = m.pwidth
    w_hi, w_lo = [], []
    for l in range(m.depth):
        cat = wp["U%d" % l] if l == 0 else np.concatenate([wp["K%d" % l][:Wp], wp["U%d" % l]], axis=0)
        hi, lo = _planes(np.ascontiguousarray(cat))
        w_hi.append(hi)
        w_lo.append(lo)
    e_hi, e_lo = _planes(wp["E"])
    return Operands(m, w_hi, w_lo, e_hi, e_lo, np.asarray(EK, dtype=np.float32), [np.asarray(c, dtype=np.float32) for c in CtxK],
                    [wp["b%d" % l].reshape(-1) for l in range(m.depth)])


def host_tables(m, flat, prec):
    """EK and CtxK as their definitions give them (derived_ref), rounded to f32: what stands in for the device's tables
    where there is no device"""
    wp = D.weights(m.shape, flat)
    if prec == PREC_SPLIT:
        Wp = m.pwidth
        eh, el = _planes(wp["E"])
        kh, kl = _planes(np.ascontiguousarray(wp["K0"][:Wp]))
        EK = (eh + el) @ kh + eh @ kl
    else:
        EK = D.ek_reference(m.shape, wp, prec)[0]
    return EK.astype(np.float32), [D.ctxk_reference(m.shape, wp, k)[0].astype(np.float32) for k in range(m.n_ctx)]


# ---------------------------------------------------------------- buffers
@dataclass
class Buffers:
    case: Case
    n_slots: int
    pool: np.ndarray            # uint32 [n_slots][2L][Wp]
    probs: np.ndarray           # uint32 [(n + GUARD)][V]
    idx: np.ndarray             # int32 [n + GUARD]
    ctx: np.ndarray             # int32 [n + GUARD][max(n_ctx, 1)]
    slot_in: np.ndarray         # int32 [n + GUARD]
    slot_out: np.ndarray
    target: np.ndarray          # int32 [n] (host, by_target)
    trap: int
    parents: np.ndarray

    def states_in(self):
        """h and c the rows start from: f32 [L][n][Wp] each"""
        L = self.case.model.depth
        s = self.pool.view(np.float32)[self.slot_in[:self.case.n]]
        return s[:, 0::2].transpose(1, 0, 2), s[:, 1::2].transpose(1, 0, 2)


def build(case):
    m, n = case.model, case.n
    rng = np.random.default_rng(_seed("buffers", case.name))
    L, W, Wp, V = m.depth, m.width, m.pwidth, m.V
    P = max(1, (n + 1) // 2)
    n_slots = P + n + 1 + 7
    perm = rng.permutation(n_slots).astype(np.int32)
    parents, outs, trap = perm[:P], perm[P:P + n], int(perm[P + n])
    pool = np.full((n_slots, 2 * L, Wp), MARK_F32, dtype=np.uint32)
    st = np.zeros((P, 2 * L, Wp), dtype=np.float32)
    st[:, 0::2, :W] = rng.uniform(-0.95, 0.95, (P, L, W))
    st[:, 1::2, :W] = rng.standard_normal((P, L, W)) * 0.5
    pool[parents] = st.view(np.uint32)
    slot_in = np.full(n + GUARD, trap, dtype=np.int32)
    slot_in[:n] = parents[rng.integers(0, P, n)]
    if n >= 2:
        slot_in[1] = slot_in[0]                           # a repeated parent in one row tile whatever the draw
    if n >= 3 and slot_in[n - 1] == slot_in[0]:           # ... and the last row on another parent than the first
        slot_in[n - 1] = parents[(int(np.argmax(parents == slot_in[0])) + 1) % P]
    slot_out = np.full(n + GUARD, trap, dtype=np.int32)
    slot_out[:n] = outs
    idx = np.full(n + GUARD, V - 1, dtype=np.int32)
    idx[:n] = rng.integers(0, V, n)
    ctx = np.full((n + GUARD, max(m.n_ctx, 1)), CTX_VOCAB - 1, dtype=np.int32)
    ctx[:n] = rng.integers(0, CTX_VOCAB, (n, ctx.shape[1]))
    idx[n - 1], ctx[n - 1] = V - 1, CTX_VOCAB - 1
    if n >= 2:
        idx[0], ctx[0] = 0, 0
    target = rng.integers(0, V, n).astype(np.int32)
    probs = np.full((n + GUARD, V), MARK_F32, dtype=np.uint32)
    return Buffers(case, n_slots, pool, probs, idx, ctx, slot_in, slot_out, target, trap, parents)


# ---------------------------------------------------------------- the model reference
STATE_FAULTS = ("lo-term", "lo-kstep", "last-8k", "neighbour-parent", "gate-block", "no-b0", "no-ctx")
OUTPUT_FAULTS = ("out-lo-E", "out-column", "out-last-kstep")
FAULTS = STATE_FAULTS + OUTPUT_FAULTS


def applicable_faults(m, n, prec):
    out = []
    for f in FAULTS:
        if f in ("lo-term", "lo-kstep", "out-lo-E") and prec != PREC_SPLIT:
            continue
        if f == "neighbour-parent" and n < 2:
            continue
        if f == "no-ctx" and m.n_ctx == 0:
            continue
        out.append(f)
    return out


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _contract(a32, w_hi, w_lo, prec, fault=None, last_layer=False, m=None):
    """f64 sum over k of the precision's terms; a32: f32 rows [n][K].  The faults sit in the top layer's recurrent half, at
    hidden units the model has (padded units contribute nothing to lose): the last 8 of them, and the last 32-wide k-step
    but one that holds any"""
    a_hi, a_lo = _planes(np.ascontiguousarray(a32, dtype=np.float32))
    K = a32.shape[1]
    if fault in ("last-8k", "lo-kstep") and last_layer:
        h0 = K - m.pwidth                                   # where the recurrent half starts
        k_end = h0 + m.width
        ks = h0 + ((m.width - 1) // 32 - 1) * 32
    if fault == "last-8k" and last_layer:
        a_hi, a_lo = a_hi.copy(), a_lo.copy()
        a_hi[:, k_end - 8:k_end] = 0
        a_lo[:, k_end - 8:k_end] = 0
    if prec != PREC_SPLIT:
        return a_hi @ w_hi
    if fault == "lo-term":
        a_lo = np.zeros_like(a_lo)
    if fault == "lo-kstep" and last_layer:
        a_lo = a_lo.copy()
        a_lo[:, ks:ks + 32] = 0
    return (a_hi + a_lo) @ w_hi + a_hi @ w_lo


def model_layers(op, prec, idx, ctx, h_in, c_in, fault=None, stored=None):
    """new (h, c), f64 [L][n][Wp], of the rows with characters idx [n], contexts ctx [n][n_ctx] and start states h_in, c_in
    (f32 [L][n][Wp]).  The layers above the first read the layer below's new h as stored, in f32: `stored` [L][n][Wp] --
    what a device or an emulation left in the pool -- or, without it, the model's own h rounded to f32.  With `stored`
    every layer is held to the model on its own: in bf16 precision the layer below's h enters through its bf16 rounding
    alone, so an h that is off by one f32 ulp can move a layer's result by 2^-9 of a term, far beyond what f32 leaves
    open; fed the stored rows the comparison of a layer sees that layer's arithmetic and nothing else."""
    m = op.m
    L, Wp, n = m.depth, m.pwidth, len(idx)
    H, C = [], []
    x = None
    for l in range(L):
        h_prev, c_prev = np.asarray(h_in[l], dtype=np.float32), np.asarray(c_in[l], dtype=np.float64)
        if fault == "neighbour-parent" and l == L - 1:       # row 0 with row n - 1's parent (another one: build's draw)
            h_prev, c_prev = h_prev.copy(), c_prev.copy()
            h_prev[0], c_prev[0] = h_in[l][n - 1], c_in[l][n - 1]
        a = h_prev if l == 0 else np.concatenate([x, h_prev], axis=1)
        z = _contract(a, op.w_hi[l], op.w_lo[l], prec, fault, l == L - 1, m)
        if not (fault == "no-b0" and l == 0):
            z = z + op.b[l].astype(np.float64)
        if l == 0:
            z = z + op.EK[idx].astype(np.float64)
            for k in range(m.n_ctx):
                if fault != "no-ctx":
                    z = z + op.CtxK[k][ctx[:, k]].astype(np.float64)
        if fault == "gate-block" and l == L - 1:              # the cell gate's first 16 units from the block next to them
            z = z.copy()
            z[:, 2 * Wp:2 * Wp + 16] = z[:, 2 * Wp + 16:2 * Wp + 32]
        i, f, g, o = _sigmoid(z[:, :Wp]), _sigmoid(z[:, Wp:2 * Wp]), np.tanh(z[:, 2 * Wp:3 * Wp]), _sigmoid(z[:, 3 * Wp:])
        c = f * c_prev + i * g
        h = o * np.tanh(c)
        H.append(h)
        C.append(c)
        x = h.astype(np.float32) if stored is None else np.asarray(stored[l], dtype=np.float32)
    return np.stack(H), np.stack(C)


def model_output(op, prec, h_top32, fault=None):
    """f64 probabilities [n][V] of the output layer over the E planes from top-layer h rows as stored (f32 [n][Wp])"""
    a_hi, a_lo = _planes(np.ascontiguousarray(h_top32, dtype=np.float32))
    e_hi, e_lo = op.e_hi, op.e_lo
    Wp = op.m.pwidth
    if fault == "out-last-kstep":
        a_hi, a_lo = a_hi.copy(), a_lo.copy()
        ks = (op.m.width - 1) // 32 * 32                    # the last k-step that holds hidden units of the model
        a_hi[:, ks:] = 0
        a_lo[:, ks:] = 0
    if prec != PREC_SPLIT:
        logits = a_hi @ e_hi.T
    else:
        if fault == "out-lo-E":
            e_lo = np.zeros_like(e_lo)
        logits = (a_hi + a_lo) @ e_hi.T + a_hi @ e_lo.T
    if fault == "out-column":                                 # character 1 from the embedding row of character 2
        logits = logits.copy()
        logits[:, 1] = logits[:, 2]
    logits = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    return e / e.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------- f32 emulations
def _acc32(a32, w_hi, w_lo, prec, order):
    """float32 accumulation of the same terms (their products are exact in f32: bf16 x bf16), k ascending, descending or
    in blocks of 32 that are summed first"""
    a_hi, a_lo = (p.astype(np.float32) for p in _planes(np.ascontiguousarray(a32, dtype=np.float32)))
    w_hi, w_lo = w_hi.astype(np.float32), w_lo.astype(np.float32)
    n, K = a32.shape
    acc = np.zeros((n, w_hi.shape[1]), dtype=np.float32)

    def add(t, k):
        t += a_hi[:, k, None] * w_hi[k]
        if prec == PREC_SPLIT:
            t += a_lo[:, k, None] * w_hi[k]
            t += a_hi[:, k, None] * w_lo[k]
    if order == "blocked":
        for k0 in range(0, K, 32):
            t = np.zeros_like(acc)
            for k in range(k0, min(k0 + 32, K)):
                add(t, k)
            acc += t
    else:
        for k in (range(K) if order == "ascending" else range(K - 1, -1, -1)):
            add(acc, k)
    return acc


def _ulps(x, d):
    x = np.asarray(x, dtype=np.float32)
    return np.nextafter(x, np.float32(np.inf if d > 0 else -np.inf)) if d else x


def _gates32(gates):
    """(sigmoid, tanh) on float32 arrays.  "lib": 1 / (1 + exp(-x)) and tanh as numpy rounds them; "hw+" / "hw-": the
    tile and cell kernels' form with the two 1-ulp instructions (exp2, reciprocal) both one ulp above / below"""
    one = np.float32(1)
    if gates == "lib":
        return (lambda x: (one / (one + np.exp(-x))).astype(np.float32)), (lambda x: np.tanh(x).astype(np.float32))
    d = 1 if gates == "hw+" else -1

    def rcp1p(x, c):
        e = _ulps(np.exp2((np.float32(c) * x).astype(np.float32)).astype(np.float32), d)
        return _ulps((one / (one + e)).astype(np.float32), d)
    return (lambda x: rcp1p(x, -1.4426950408889634)), (lambda x: (np.float32(2) * rcp1p(x, -2.8853900817779268) - one).astype(np.float32))


EMULATIONS = (("ascending", "lib"), ("descending", "hw+"), ("blocked", "hw-"))


def emulate(op, prec, idx, ctx, h_in, c_in, order, gates):
    """the step in float32: (h, c) f32 [L][n][Wp] and probabilities f32 [n][V]"""
    m = op.m
    L, Wp = m.depth, m.pwidth
    sig, tanh = _gates32(gates)
    H, C = [], []
    x = None
    for l in range(L):
        h_prev, c_prev = np.asarray(h_in[l], dtype=np.float32), np.asarray(c_in[l], dtype=np.float32)
        a = h_prev if l == 0 else np.concatenate([x, h_prev], axis=1)
        init = op.b[l].astype(np.float32)[None, :]
        if l == 0:
            init = op.EK[idx] + init if order != "descending" else init + op.EK[idx]
            for k in range(m.n_ctx):
                init = init + op.CtxK[k][ctx[:, k]]
        z = _acc32(a, op.w_hi[l], op.w_lo[l], prec, order)
        z = (init + z) if order != "blocked" else (z + init)
        i, f, g, o = sig(z[:, :Wp]), sig(z[:, Wp:2 * Wp]), tanh(z[:, 2 * Wp:3 * Wp]), sig(z[:, 3 * Wp:])
        c = (f * c_prev + i * g).astype(np.float32)
        h = (o * tanh(c)).astype(np.float32)
        H.append(h)
        C.append(c)
        x = h
    logits = _acc32(x, op.e_hi.T, op.e_lo.T, prec, order)
    e = np.exp(logits - logits.max(axis=1, keepdims=True)).astype(np.float32)
    s = np.zeros(len(e), dtype=np.float32)
    for v in (range(e.shape[1]) if order != "descending" else range(e.shape[1] - 1, -1, -1)):
        s += e[:, v]
    p = (e * (np.float32(1) / s)[:, None]).astype(np.float32) if gates != "lib" else (e / s[:, None]).astype(np.float32)
    return np.stack(H), np.stack(C), p


# ---------------------------------------------------------------- references and bounds of a case
def _sample(n, k):
    return np.unique(np.linspace(0, n - 1, min(n, k)).round().astype(int))


@dataclass
class Refs:
    op: Operands
    prec: int
    true_probs: np.ndarray      # f64 [n][V]
    true_H: np.ndarray          # f64 [L][n][W] (logical width)
    true_C: np.ndarray
    e32_state: float
    e32_prob: float
    extra: dict = field(default_factory=dict)

    @property
    def tol_state(self):
        return TOL_FACTOR * self.e32_state

    @property
    def tol_prob(self):
        return TOL_FACTOR * self.e32_prob


def e32(op, prec, idx, ctx, h_in, c_in, rows):
    """(E32 of the states, E32 of the probabilities) on the rows `rows` of the call"""
    idx, ctx, h_in, c_in = idx[rows], ctx[rows], h_in[:, rows], c_in[:, rows]
    es = ep = 0.0
    for order, gates in EMULATIONS:
        h, c, p = emulate(op, prec, idx, ctx, h_in, c_in, order, gates)
        H, C = model_layers(op, prec, idx, ctx, h_in, c_in, stored=h)
        es = max(es, float(np.abs(h - H).max()), float(np.abs(c - C).max()))
        pm = model_output(op, prec, h[-1])
        ep = max(ep, float((np.abs(p - pm) / pm).max()))
    return es, ep


def true_reference(m, w, idx, ctx, h_in, c_in):
    """oracle.lstm_oracle.step_batch in f64 from the f32 parameters, at the logical width"""
    from oracle import lstm_oracle as O
    cfg = O.ModelConfig(m.depth, m.width, m.V, m.n_ctx)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = []
    for l in range(m.depth):
        st += [h_in[l][:, :m.width].astype(np.float64), c_in[l][:, :m.width].astype(np.float64)]
    probs, out = O.step_batch(cfg, w64, idx, ctx[:, :m.n_ctx], st)
    return probs, np.stack(out[0::2]), np.stack(out[1::2])


def references(buf, w, op, prec):
    case = buf.case
    n = case.n
    idx, ctx = buf.idx[:n], buf.ctx[:n]
    h_in, c_in = buf.states_in()
    tp, tH, tC = true_reference(case.model, w, idx, ctx, h_in, c_in)
    es, ep = e32(op, prec, idx, ctx, h_in, c_in, _sample(n, SAMPLE_ROWS))
    return Refs(op, prec, tp, tH, tC, es, ep)


def fault_deviations(buf, op, prec):
    """name -> what the checker would see of the model with that fault, in units of the case's tolerance: the deviation
    of its states from the model fed the faulty rows as stored (absolute over h and c), of its probabilities from the
    model's (relative), on the first FAULT_ROWS rows.  Returns the dict and the (E32 state, E32 prob) it was scaled by."""
    case = buf.case
    n = min(case.n, FAULT_ROWS)
    idx, ctx = buf.idx[:n], buf.ctx[:n]
    h_in, c_in = (s[:, :n] for s in buf.states_in())
    es, ep = e32(op, prec, idx, ctx, h_in, c_in, _sample(n, SAMPLE_ROWS))
    H, C = model_layers(op, prec, idx, ctx, h_in, c_in)
    h_top = H[-1].astype(np.float32)
    P = model_output(op, prec, h_top)
    out = {}
    for f in applicable_faults(case.model, n, prec):
        if f in STATE_FAULTS:
            Hf, Cf = model_layers(op, prec, idx, ctx, h_in, c_in, fault=f)
            Hm, Cm = model_layers(op, prec, idx, ctx, h_in, c_in, stored=Hf.astype(np.float32))
            out[f] = max(float(np.abs(Hf - Hm).max()), float(np.abs(Cf - Cm).max())) / (TOL_FACTOR * es)
        else:
            Pf = model_output(op, prec, h_top, fault=f)
            out[f] = float((np.abs(Pf - P) / P).max()) / (TOL_FACTOR * ep)
    return out, (es, ep)


# ---------------------------------------------------------------- the checker
class ContractFailure(AssertionError):
    def __init__(self, promise, message, metrics=None):
        assert promise in PROMISES
        self.promise, self.metrics = promise, metrics or {}
        super().__init__("%s: %s" % (promise, message))


def _where(bad, shape):
    i = np.unravel_index(int(np.argmax(bad)), shape)
    return "%d element(s), first at %s" % (int(bad.sum()), tuple(int(v) for v in i))


def check(buf, refs, pool_after, probs_after, heads=None):
    """pool_after: uint32 like buf.pool; probs_after: uint32 like buf.probs (by_target: its first n words are the picked
    probabilities); heads: f32 [n][head_k * Wp] as delivered (host entry), or None.  Raises ContractFailure with the
    first broken promise, returns the figures of the value comparison."""
    case = buf.case
    m, n = case.model, case.n
    L, W, Wp, V = m.depth, m.width, m.pwidth, m.V
    outs = buf.slot_out[:n]
    pool_after = np.asarray(pool_after).view(np.uint32).reshape(buf.pool.shape)
    probs_after = np.asarray(probs_after).view(np.uint32).reshape(buf.probs.shape)
    # 1 -- nothing but slot_out's slots changes
    keep = np.ones(buf.n_slots, dtype=bool)
    keep[outs] = False
    bad = (pool_after != buf.pool) & keep[:, None, None]
    if bad.any():
        s = int(np.argmax(bad.any(axis=(1, 2))))
        kind = "the trap slot" if s == buf.trap else "a parent slot" if s in set(buf.parents.tolist()) else "a bystander slot"
        raise ContractFailure("slots", "slot %d (%s) written: %s" % (s, kind, _where(bad, bad.shape)))
    # 2 -- nothing behind the n rows of probs
    flat = probs_after.reshape(-1)
    valid = n if case.by_target else n * V
    bad = flat[valid:] != MARK_F32
    if bad.any():
        raise ContractFailure("probs-tail", "%d word(s) behind the %d delivered, first at word %d" % (int(bad.sum()), valid, valid + int(np.argmax(bad))))
    # 3 -- everything that had to be written is a number
    st = pool_after[outs].view(np.float32)
    bad = ~np.isfinite(st)
    if bad.any():
        left = int((pool_after[outs] == MARK_F32).sum())
        raise ContractFailure("finite", "new states (%d of them the marker still): %s (row, vector, unit)" % (left, _where(bad, bad.shape)))
    got_p = flat[:valid].view(np.float32).reshape((n,) if case.by_target else (n, V))
    bad = ~np.isfinite(got_p)
    if bad.any():
        raise ContractFailure("finite", "probabilities: %s" % _where(bad, bad.shape))
    # 4 -- padded hidden units
    if Wp > W:
        bad = st[:, :, W:] != 0
        if bad.any():
            raise ContractFailure("padding", "padded hidden units not zero: %s" % _where(bad, bad.shape))
    # 5 -- the model reference
    got_h, got_c = st[:, 0::2].transpose(1, 0, 2), st[:, 1::2].transpose(1, 0, 2)
    h_in, c_in = buf.states_in()
    H, C = model_layers(refs.op, refs.prec, buf.idx[:n], buf.ctx[:n], h_in, c_in, stored=got_h)
    dh, dc = np.abs(got_h - H), np.abs(got_c - C)
    pm = model_output(refs.op, refs.prec, got_h[-1])
    pt = refs.true_probs
    if case.by_target:
        pm, pt = pm[np.arange(n), buf.target], pt[np.arange(n), buf.target]
    dp = np.abs(got_p - pm) / pm
    metrics = {"state": float(max(dh.max(), dc.max())), "prob_rel": float(dp.max()), "e32_state": refs.e32_state, "e32_prob": refs.e32_prob,
               "state_ratio": float(max(dh.max(), dc.max())) / refs.e32_state, "prob_ratio": float(dp.max()) / refs.e32_prob}
    for name, d in (("h", dh), ("c", dc)):
        if d.max() > refs.tol_state:
            raise ContractFailure("model", "%s off by %.3g (tol %.3g = %d x E32 %.3g): %s (layer, row, unit)"
                                  % (name, d.max(), refs.tol_state, TOL_FACTOR, refs.e32_state, _where(d > refs.tol_state, d.shape)), metrics)
    if dp.max() > refs.tol_prob:
        raise ContractFailure("model", "probabilities off by %.3g relative (tol %.3g = %d x E32 %.3g): %s"
                              % (dp.max(), refs.tol_prob, TOL_FACTOR, refs.e32_prob, _where(dp > refs.tol_prob, dp.shape)), metrics)
    if not case.by_target:
        rs = np.abs(got_p.astype(np.float64).sum(axis=1) - 1.0)
        metrics["row_sum"] = float(rs.max())
        if rs.max() > ROW_SUM:
            raise ContractFailure("model", "row %d sums to 1 %+.3g" % (int(np.argmax(rs)), rs.max()), metrics)
    if heads is not None:
        want = pool_after[outs].reshape(n, -1)[:, :case.head_k * Wp]
        bad = np.asarray(heads).view(np.uint32).reshape(n, -1) != want
        if bad.any():
            raise ContractFailure("model", "delivered head vectors differ from the new slots: %s" % _where(bad, bad.shape), metrics)
    # 6 -- the true reference
    th = float(max(np.abs(got_h[:, :, :W] - refs.true_H).max(), np.abs(got_c[:, :, :W] - refs.true_C).max()))
    tp = float(np.abs(got_p - pt).max())
    metrics["true_state"], metrics["true_prob"] = th, tp
    if refs.prec == PREC_SPLIT:
        if th > TRUE_STATES:
            raise ContractFailure("true", "states off the f64 oracle by %.3g (bound %.3g)" % (th, TRUE_STATES), metrics)
        if tp > TRUE_PROBS:
            raise ContractFailure("true", "probabilities off the f64 oracle by %.3g (bound %.3g)" % (tp, TRUE_PROBS), metrics)
    return metrics


def model_result(buf, refs, fault=None):
    """(pool, probs) as uint32 arrays after a step that computes the model reference (rounded to f32) with `fault`:
    what tests/test_step_contract_ref.py feeds the checker"""
    case = buf.case
    n = case.n
    h_in, c_in = buf.states_in()
    H, C = model_layers(refs.op, refs.prec, buf.idx[:n], buf.ctx[:n], h_in, c_in, fault=fault if fault in STATE_FAULTS else None)
    pool = buf.pool.copy()
    st = np.empty((n, 2 * case.model.depth, case.model.pwidth), dtype=np.float32)
    st[:, 0::2], st[:, 1::2] = H.transpose(1, 0, 2), C.transpose(1, 0, 2)
    pool[buf.slot_out[:n]] = st.view(np.uint32)
    p = model_output(refs.op, refs.prec, st[:, 2 * (case.model.depth - 1)], fault=fault if fault in OUTPUT_FAULTS else None).astype(np.float32)
    probs = buf.probs.copy()
    if case.by_target:
        probs.reshape(-1)[:n] = p[np.arange(n), buf.target].view(np.uint32)
    else:
        probs[:n] = p.view(np.uint32)
    return pool, probs
