"""The gradients of the look-up tables of a training window -- dE and every dCtx_n -- and the embedding regularisers, held to
f64 references of what the kernels stored, as tests/window_grads.py holds dU, dK and db.

Behind the recurrence scans `kl_train_window` builds dE from three parts and each dCtx_n from two (`train_output_layer`,
`table_grads` and `kl_launch_regulariser_grads` of csrc/api.hip).  Given the arrays exactly as the kernels stored them -- the
window decoded at the PADDED width by tests/window_ref.py (`read_window_padded`), now with the output layer's `dlogits`
(`decode_dlogits`, through off_dlogits / ld_dlogits of `kl_test_window_view`) -- every part is a plain product of known
numbers.  CPU only: used by tests/test_table_grads_ref.py (the checker's own sensitivity), tests/test_table_grads_gpu.py (one
case per route) and `check_train_window_gradients` of tests/test_gpu_kernels.py.

References are numpy f64; rows are time-major, r = t * B + b; Wp is the padded width, V the vocabulary, Vp its table rows.

  dE, output part   A = dlogits[:, :V]^T . X_top, X_top = Hd[L-1] where the view has it (off_Hd[L-1] != 0), else blocks 1 .. T of
                    H[L-1].  Exact: columns V .. Vp of dlogits are zero, rows of dummy streams are zero.
  dE, input part    C = bf16(S) . bf16(K0[:Wp])^T, S[v] = the f64 sum of the rows of dZ_0 with idx == v (window_grads.key_sums).
                    The engine rounds S to bf16 before the product, and so does the reference.  A sum within REL (relative) of
                    a bf16 rounding boundary may round either way; the two candidates lie one bf16 step apart,
                    2^-7 |S| / m <= 2^-7 |S|, so such an entry widens the bound of output (v, w) by
                    2^-7 |S[v][j]| |K0bf[w][j]| -- the FULL step, not the half step that the note in tests/window_grads.py
                    finds too small for K0's character rows (that bound stays as it is).  The number of sums near a
                    boundary is reported.
  E, total          ref = A + C + oracle.regulariser_grads evaluated on the f32 table; per entry
                      REL x (max|A| + max|C|) + boundary allowance + 2^-22 x (|A| + |C| + M_reg)
                    REL = 1e-5 is what the same GEMM kernels are held to on bare buffers and in tests/window_grads.py; it applies
                    because the operands are the same stored bf16 numbers.  M_reg = the sum of the magnitudes of the
                    regulariser's terms at the entry (`reg_magnitudes`):
                      characters  0.04 (1 + n_r) |x|, plus 2 (|x| + |mean|) in row 0
                      contexts    0.08 (1 + n_r) |x|, plus 0.2 sum_r |C_r| on rows >= 2, plus 4 (R' |x| + N1 mean|C|) on row 0
                    2^-22 is four f32 ulps: three `+=` into the f32 entry plus the regulariser's own f32 arithmetic.  It is
                    DERIVED from this rounding model, not measured.  Columns W .. Wp of dE: exactly zero.
  dCtx_n            ref = S_n . K0[Wp + n D : Wp + (n + 1) D]^T + the regulariser's f64 gradient; K0 as the f32 parameters (this
                    path is f32 throughout), S_n = the key sums of dZ_0 by ctx[..., n];
                    bound REL x max|ref_data| + 2^-22 x (|ref_data| + M_reg).
  precondition      per array, max|regulariser gradient| <= max|back-propagated part|, from the references' numbers alone: only
                    then does the ONE f32 number per entry that the engine delivers resolve the part under test.  The tests
                    meet it with regulariser-neutral tables (`neutral_tables`): E's rows 1.. of unit norm and row 0 their mean;
                    every Ctx_n with rows 1 .. R-2 unit-norm rows in +/- pairs, row R-1 a copy of row R-2, row 0 zero, all
                    times 1e-3 (with unit-norm context rows not scaled down an f32 restatement of the regulariser kernels was
                    3e-7 off on the body and 6e-6 on row 0, beside REL x max data of 9e-9).  K, U and b are untouched.
                    At 1e-3 the context tables' regulariser gradient is 7e-5; windows of a thousand streams and more
                    back-propagate 1e-5 .. 3e-5 into a context table, and for them the tests scale by 1e-5 instead
                    (tests/test_table_grads_gpu.py has the figures) -- the precondition stays as it is.
                    `check_train_window_gradients` runs with the precondition reported, not asserted, and asserts the exact
                    checks only.

The regulariser kernels on their own (`kl_test_regulariser_grads`, one table per call): `check_regulariser` holds the gradient
to REL x max|ref| + 2^-22 x M_reg, separately over row 0 and over rows >= 1 (row 0 is 1e2 times larger and would hide the
body), and the value to REL (relative).  `restate_f32` states the two kernels in numpy f32 (its `variant`s are the mistakes
tests/test_table_grads_ref.py tells apart); it must stay at or below 0.5 of these bounds on every case of the GPU table
(REGULARISER_CASES, checked on the CPU by tests/test_table_grads_ref.py) -- a case that does not is changed, not the bound.

Known limits: rows of E whose regulariser terms are large under non-neutral tables stay covered only by tests/gradcheck.py;
the 2^-22 allowances come from a rounding model; stream groups are out of scope (the workspace holds the last group only).
The engine delivers ONE number per entry, so a failure cannot measure the parts apart: it names the array, the worst element,
the magnitude of every part there, the route and, as "part", the smallest back-propagated part there that is large enough to
explain the error (at least half of it; a part cannot be wrong by much more than itself), else the regulariser if that is,
else the largest back-propagated part -- a hint at where to read, no more.
"""
import numpy as np

from oracle import lstm_oracle as O
from tests import window_grads as WG

REL = WG.REL
F32_ULPS = 2.0 ** -22
OUT_LOGITS_WS, OUT_LOGITS_W128, OUT_DH_WS, OUT_DE_KMAJOR = 1, 2, 4, 8      # kl_window_view.out_route (include/keraslm_hip.h)


class Precondition(AssertionError):
    """the regularisers' gradient is larger than the part under test (see the module text)"""


def route_text(view):
    """`window_grads.route_text` and what the output layer in front of that stage did"""
    o = view.get("out_route", 0)
    logits = "one kernel (width 512)" if o & OUT_LOGITS_WS else ("one kernel with dH (width 128)" if o & OUT_LOGITS_W128 else "GEMM + softmax")
    dh = "with the logits" if o & OUT_LOGITS_W128 else ("width-512 kernel" if o & OUT_DH_WS else "GEMM")
    return "%s; output layer: logits by %s, dH by %s, dE %s" % (WG.route_text(view), logits, dh,
                                                                "k-major" if o & OUT_DE_KMAJOR else "over dlogits^T")


# ---------------------------------------------------------------------------------------------- tables
def _unit_rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-300)


def neutral_char_table(E):
    """rows 1.. scaled to unit norm, row 0 their mean"""
    out = _unit_rows(E)
    if out.shape[0] > 1:
        out[0] = out[1:].mean(axis=0)
    return out.astype(np.float32)


def neutral_ctx_table(C, scale=1e-3):
    """rows 1 .. R-2: unit-norm rows in +/- pairs (an odd count leaves the last one without a partner), row R-1 a copy of row
    R-2, row 0 zero, everything times `scale`"""
    out = _unit_rows(C)
    R = out.shape[0]
    for r in range(2, R - 1, 2):
        out[r] = -out[r - 1]
    if R >= 3:
        out[R - 1] = out[R - 2]
    out[0] = 0.0
    return (out * scale).astype(np.float32)


def neutral_tables(w, ctx_scale=1e-3):
    """the weights with regulariser-neutral look-up tables (see the module text); K, U and b untouched.  ctx_scale: what the
    context tables are multiplied by -- their regulariser gradient is 0.08 x their entries, the back-propagated part does not
    depend on them, so a window whose back-propagated part is small (many streams: it falls with their number) meets the
    precondition with a smaller scale"""
    out = dict(w)
    out["E"] = neutral_char_table(w["E"])
    for k in w:
        if k.startswith("Ctx"):
            out[k] = neutral_ctx_table(w[k], ctx_scale)
    return out


# ---------------------------------------------------------------------------------------------- the regularisers
def _one_table(X, mode):
    X = np.asarray(X)
    cfg = O.ModelConfig(1, X.shape[1], X.shape[0], mode)
    return cfg, ({"E": X} if mode == 0 else {"E": np.zeros((0, X.shape[1]), dtype=X.dtype), "Ctx0": X})


def reg_magnitudes(X, mode):
    """M_reg [R][D]: the sum of the magnitudes of the regulariser's terms at every entry (mode 0 characters, 1 contexts)"""
    X = np.asarray(X, dtype=np.float64)
    R = X.shape[0]
    n = (X * X).sum(axis=1)
    M = (0.04 if mode == 0 else 0.08) * (1.0 + n)[:, None] * np.abs(X)
    if R < 2:
        return M
    if mode == 0:
        M[0] += 2.0 * (np.abs(X[0]) + np.abs(X[1:].mean(axis=0)))
    else:
        M[2:] += 0.2 * np.abs(X[1:-1]).sum(axis=0)[None]
        M[0] += 4.0 * ((R - 1) * np.abs(X[0]) + n[1:].sum() * np.abs(X[1:]).mean(axis=0))
    return M


def regulariser_ref(X, mode):
    """one f32 table -> (gradient f64 [R][D], value f64, M_reg) from oracle.regulariser_grads / oracle.regularisers"""
    cfg, w = _one_table(X, mode)
    g = O.regulariser_grads(cfg, w)
    return g["E" if mode == 0 else "Ctx0"], float(O.regularisers(cfg, w)), reg_magnitudes(X, mode)


def regulariser_bounds(X, mode):
    """-> (ref gradient, ref value, bound [R][D]): REL x max|ref| + 2^-22 x M_reg, the maximum over row 0 and over rows >= 1
    separately"""
    ref, value, M = regulariser_ref(X, mode)
    bound = F32_ULPS * M
    bound[0] += REL * np.abs(ref[0]).max()
    if ref.shape[0] > 1:
        bound[1:] += REL * np.abs(ref[1:]).max()
    return ref, value, bound


def check_regulariser(X, mode, grad, value, where="", raise_=True):
    """grad [R][D], value: what the kernels (or `restate_f32`) made of table X -> dict(row0, body, value): error / bound;
    raises AssertionError naming the parts beyond their bound, the worst element of each and the shape"""
    ref, ref_value, bound = regulariser_bounds(X, mode)
    over = np.abs(np.asarray(grad, dtype=np.float64) - ref) / np.maximum(bound, 1e-300)
    rep = dict(row0=float(over[0].max()), body=float(over[1:].max()) if ref.shape[0] > 1 else 0.0,
               value=abs(float(value) - ref_value) / max(REL * abs(ref_value), 1e-300))
    bad = []
    for part, rows0, o in (("row 0", 0, over[:1]), ("rows >= 1", 1, over[1:])):
        if o.size and not o.max() <= 1.0:
            r, c = np.unravel_index(np.argmax(np.where(np.isnan(o), np.inf, o)), o.shape)
            r += rows0
            bad.append(("regulariser gradient", part, "element (%d, %d)" % (r, c), "got %.8g" % np.asarray(grad)[r, c], "ref %.8g" % ref[r, c],
                        "bound %.3g" % bound[r, c]))
    if not rep["value"] <= 1.0:
        bad.append(("regulariser value", "got %.9g" % value, "ref %.9g" % ref_value, "bound %.3g" % (REL * abs(ref_value))))
    rep["failed"] = {b[1] if b[0].endswith("gradient") else "value" for b in bad}
    if bad and raise_:
        raise AssertionError((where, "characters" if mode == 0 else "contexts", "table %d x %d" % ref.shape, bad))
    return rep


VARIANTS = ("smoothness from row 1", "s1 with row R-1", "mean over R", "constants swapped", "no row-0 term", "value without smoothness")


def restate_f32(X, mode, variant=None):
    """reg_stats_kernel + reg_apply_kernel of csrc/elementwise.hip in numpy f32 (numpy's summation order, not the device's)
    -> (gradient f32 [R][D], value f32).  `variant`: one of VARIANTS, a mistake such kernels could make."""
    f = np.float32
    X = np.asarray(X, dtype=f)
    R, D = X.shape
    col = X[1:].sum(axis=0, dtype=f)
    mean = col / f(R if variant == "mean over R" else R - 1)
    s1 = col if variant == "s1 with row R-1" else col - X[R - 1]
    s2 = col - X[1]
    nr = (X * X).sum(axis=1, dtype=f)
    N1, N2 = nr[1:].sum(dtype=f), (nr[1:] * nr[1:]).sum(dtype=f)
    c_low = f(0.01 if (mode == 0) != (variant == "constants swapped") else 0.02)
    q = f(1) - nr
    g = (f(-4) * c_low * q)[:, None] * X
    loss = (c_low * q * q).sum(dtype=f)
    Rp = f(R - 1)
    if mode == 0:
        if variant != "no row-0 term":
            u = X[0] - mean
            g[0] += f(2) * u
            loss += (u * u).sum(dtype=f)
    else:
        g[(1 if variant == "smoothness from row 1" else 2):] += f(0.2) * s1
        x = X[0]
        if variant != "no row-0 term":
            g[0] += f(4) * (Rp * x - N1 * mean)
        smooth = f(0) if variant == "value without smoothness" else f(0.2) * s1 * s2
        loss += (smooth + f(2) * (Rp * x * x - f(2) * x * mean * N1 + mean * mean * N2)).sum(dtype=f)
    return g.astype(f), f(loss)


def _table(rule, kind, R, D, zero_from=None):
    """the table of one case of REGULARISER_CASES: `kind` 0.3 / 0.5 = oracle.init_weights' normal rows of that deviation,
    "neutral" = the regulariser-neutral form of the first"""
    rng = np.random.default_rng(1000 * R + D)
    std = 0.3 if kind == "neutral" else kind
    X = (rng.standard_normal((R, D)) * std).astype(np.float32)
    if zero_from is not None:
        X[:, zero_from:] = 0.0
    if kind == "neutral":
        X = neutral_char_table(X) if rule == 0 else neutral_ctx_table(X)
    return X


# (rule, R, D, columns from here on zero, kind of table): the cases of tests/test_table_grads_gpu.py's hook test.
# Characters: two rows (the smallest the launcher runs), three, a usual table, a padded width (100 of 128), one column per
# thread of reg_stats_kernel's first branch with several row groups (512), its edge D == 1024 (one row group), and the
# other branch (1056 columns: the engine takes any multiple of 32).  Contexts: the smallest tables -- no row for the
# smoothness term at R = 2, one at 3, s1 != s2 from 4 on --, an odd count, the model's own 200 x 10.
# Every shape with oracle.init_weights' tables at 0.3 and 0.5 and with a neutral one -- except that the characters' neutral
# tables have at most NEUTRAL_CHAR_ROWS = 17 rows, and none at two rows.  In a neutral character table row 0 IS the mean of
# the others, so its gradient 2 (x - mean) is what the f32 column sum's own rounding leaves of it: about one f32 ulp of a
# ROW's entries whatever R is, against a bound in terms of |mean| ~ |x| / sqrt(R).  The restatement's row 0 reached 0.46 of
# the bound at 50 rows, 0.96 at 256 and 1.36 at 330 (0.27 at 17), so the cases were changed, not the bound; with two rows
# the value is exactly zero and a relative bound says nothing.
NEUTRAL_CHAR_ROWS = 17
_SHAPES = [(0, 2, 64, None), (0, 3, 64, None), (0, 50, 64, None), (0, 60, 128, 100), (0, 256, 512, None), (0, 330, 1024, None),
           (0, 40, 1056, None), (1, 2, 10, None), (1, 3, 10, None), (1, 4, 10, None), (1, 17, 10, None), (1, 200, 10, None)]
REGULARISER_CASES = [s + (k,) for s in _SHAPES for k in (0.3, 0.5)] + \
                    [(0, min(R, NEUTRAL_CHAR_ROWS), D, z, "neutral") for rule, R, D, z in _SHAPES if rule == 0 and R > 2] + \
                    [s + ("neutral",) for s in _SHAPES if s[0] == 1]


def regulariser_case_table(case):
    rule, R, D, zero_from, kind = case
    return _table(rule, kind, R, D, zero_from)


# ---------------------------------------------------------------------------------------------- the window
def table_parts(win, idx, ctx, P):
    """the f64 references of one window: dict(A, C, allowance, near, S, reg = {name: gradient}, M = {name: M_reg},
    ctx = [ref_data per context variable], X_top, masked_top)"""
    view = win["view"]
    L, Wp = view["depth"], view["width"]
    ops = WG.operands(win)
    dl = np.asarray(win["dlogits"], dtype=np.float64)
    V = P["E"].shape[0]
    top = ops[L - 1]
    X_top = top["Hd"] if top["Hd"] is not None else top["Hnext"]
    A = dl[:, :V].T @ X_top
    dz = ops[0]["dZ"]
    S = WG.key_sums(np.asarray(idx).T.reshape(-1), V, dz)
    near = WG.near_bf16_boundary(S)
    K0 = np.asarray(P["K0"])
    K0bf = O.bf16_round(K0[:Wp]).astype(np.float64)
    Cm = O.bf16_round(S).astype(np.float64) @ K0bf.T
    allowance = 2.0 ** -7 * ((np.abs(S) * near) @ np.abs(K0bf).T)
    n_ctx = 0 if ctx is None else np.asarray(ctx).shape[2]
    tabs = {"E": np.asarray(P["E"])}
    for n in range(n_ctx):
        tabs["Ctx%d" % n] = np.asarray(P["Ctx%d" % n])
    reg = O.regulariser_grads(O.ModelConfig(1, Wp, V, n_ctx), tabs)
    M = {name: reg_magnitudes(t, 0 if name == "E" else 1) for name, t in tabs.items()}
    data = []
    for n in range(n_ctx):
        R_, D = tabs["Ctx%d" % n].shape
        Sn = WG.key_sums(np.asarray(ctx)[:, :, n].T.reshape(-1), R_, dz)
        data.append(Sn @ K0[Wp + n * D:Wp + (n + 1) * D].astype(np.float64).T)
    return dict(A=A, C=Cm, allowance=allowance, near=near, S=S, reg=reg, M=M, ctx=data, X_top=X_top, masked_top=top["Hd"] is not None)


def check_table_grads(win, idx, ctx, params, grads, layout, width=None, dummy_from=None, where="", raise_=True, precondition=True):
    """win: `window_ref.read_window_padded`'s dict (with "dlogits" and "view"); idx [B][T], ctx [B][T][n_ctx] or None: the
    window's inputs (all streams the kernels ran); params, grads: the engine's flat physical arrays (or dicts as
    `window_grads.split_flat` gives them); layout: kl_param_layout's; width: the model's own width where the engine padded it;
    dummy_from: the first stream without any target (their dlogits rows must be exactly zero).
    -> {name: dict(ratio, err, bound, at, part, terms, precondition = (max|regulariser|, max|data|), ...)} for E and every
    Ctx_n; raises WG.GradMismatch naming every array beyond its bound -- or, with raise_=False, returns (report, GradMismatch
    or None).  precondition=True: raises `Precondition` where the regularisers hide the part under test; False: reports it."""
    view = win["view"]
    Wp, B = view["width"], view["B"]
    W = Wp if width is None else width
    P = params if isinstance(params, dict) else WG.split_flat(params, layout)
    Gr = grads if isinstance(grads, dict) else WG.split_flat(grads, layout)
    route = route_text(view)
    dl = np.asarray(win["dlogits"])
    V = P["E"].shape[0]
    report, bad = {}, []

    def exact(name, what, nz):
        if nz.any():
            bad.append(("%s %s" % (name, what), name, "non-zero where exactly zero is due", "first at %s" % np.argwhere(nz)[0].tolist(), "route: " + route))
            report.setdefault(name, {})["exact"] = False

    exact("E", "output: dlogits columns >= V", dl[:, V:] != 0)
    if dummy_from is not None:
        exact("E", "output: dlogits rows of dummy streams", dl.reshape(-1, B, dl.shape[1])[:, dummy_from:] != 0)
    exact("E", "padding: columns of padded hidden units", np.asarray(Gr["E"])[:, W:] != 0)
    p = table_parts(win, idx, ctx, P)

    def hold(name, got, terms, ref, bound, reg, **extra):
        got = np.asarray(got, dtype=np.float64)
        over = np.abs(got - ref) / np.maximum(bound, 1e-300)
        ratio = float(np.nanmax(over)) if not np.isnan(over).any() else float("nan")
        r, c = WG._tile(over)
        at = {k: float(np.abs(v[r, c])) for k, v in terms.items()}
        err_at = float(np.abs(got - ref)[r, c])
        enough = {k: v for k, v in at.items() if v >= 0.5 * err_at and k != "regulariser"}
        rest = {k: v for k, v in at.items() if k != "regulariser"}
        part = min(enough, key=enough.get) if enough else ("regulariser" if at["regulariser"] >= 0.5 * err_at else max(rest, key=rest.get))
        data = sum(v for k, v in terms.items() if k != "regulariser")
        rep = dict(ratio=ratio, err=float(np.abs(got - ref)[r, c]), bound=float(bound[r, c]), at=(int(r), int(c)), part=part, terms=at,
                   precondition=(float(np.abs(reg).max()), float(np.abs(data).max())), exact=report.get(name, {}).get("exact", True), **extra)
        report[name] = rep
        if not ratio <= 1.0:
            bad.append(("%s %s" % (name, part), name, "element (%d, %d)" % (r, c), "error %.4g" % rep["err"], "bound %.4g" % rep["bound"],
                        "got %.8g" % got[r, c], "ref %.8g" % ref[r, c], "parts there: " + ", ".join("%s %.4g" % kv for kv in at.items()),
                        "smallest that explains it: " + part, "route: " + route))

    A, Cm = p["A"], p["C"]
    bound = REL * (np.abs(A).max() + np.abs(Cm).max()) + p["allowance"] + F32_ULPS * (np.abs(A) + np.abs(Cm) + p["M"]["E"])
    hold("E", Gr["E"], {"output": A, "input": Cm, "regulariser": p["M"]["E"]}, A + Cm + p["reg"]["E"], bound, p["reg"]["E"],
         near_boundary=int(p["near"].sum()), sums=int((p["S"] != 0).sum()), masked_top=p["masked_top"])
    for n, data in enumerate(p["ctx"]):
        name = "Ctx%d" % n
        bound = REL * np.abs(data).max() + F32_ULPS * (np.abs(data) + p["M"][name])
        hold(name, Gr[name], {"context %d" % n: data, "regulariser": p["M"][name]}, data + p["reg"][name], bound, p["reg"][name])
    hidden = {k: v["precondition"] for k, v in report.items() if not v["precondition"][0] <= v["precondition"][1]}
    if precondition and hidden:
        raise Precondition((where, "max|regulariser gradient| > max|back-propagated part|", hidden))
    err = WG.GradMismatch(bad, where) if bad else None
    if not raise_:
        return report, err
    if err:
        raise err
    return report


def ratio_line(report):
    """'dE 0.12 | dCtx 0.10 0.08 | near n of m': error / bound of the tables' gradients and how many of layer 0's character
    sums lay near a rounding boundary"""
    ctxs = [report[k]["ratio"] for k in sorted(report) if k.startswith("Ctx")]
    return "dE %.2f | dCtx %s | near %d of %d" % (report["E"]["ratio"], " ".join("%.2f" % r for r in ctxs) or "-", report["E"]["near_boundary"],
                                                  report["E"]["sums"])


def precondition_line(report):
    """'E 1.0e-03 <= 5.5e-03 | Ctx0 ...': max|regulariser gradient| against max|back-propagated part| per array"""
    return " | ".join("%s %.1e %s %.1e" % (k, v["precondition"][0], "<=" if v["precondition"][0] <= v["precondition"][1] else ">", v["precondition"][1])
                      for k, v in sorted(report.items()))
