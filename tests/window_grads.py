"""The weight-gradient stage of a training window held to the products of what the scans left in the workspace.

Behind the recurrence scans, `kl_train_window` turns H, the masked outputs Hd and dZ into dU, dK and db of every layer
(the `weight_grads` lambda of csrc/api.hip).  Given those arrays exactly as the kernels stored them -- bf16 numbers, found
through `kl_test_window_view` and decoded by tests/window_ref.py at the PADDED width, every stream included -- each weight
gradient is a plain product of known numbers, and the engine's f32 result can be held to f32-accumulation accuracy instead
of the 1.5e-2 / 3e-2 of tests/gradcheck.py, which has to absorb the bf16 rounding of the whole pass.  CPU only: used by
tests/test_window_grads_ref.py (the checker's own sensitivity), tests/test_window_grads_gpu.py (one case per route of the
stage) and `check_train_window_gradients` of tests/test_gpu_kernels.py.

References are numpy f64 over the decoded values; rows are time-major, r = t * B + b; W is the padded width.

  dU_l              sum_t H_l[block t]^T . dZ_l[t] with blocks 0 .. T-1 of H_l (block 0 = the carried-in output)
  dK_l, l >= 1      X^T . dZ_l, X = Hd[l-1] where the view has it, else blocks 1 .. T of H[l-1]
                    bound for both: every element within REL = 1e-5 x max|ref| of the array -- what test_gemm_tn, test_gemm_an
                    and tests/test_gemm_wide_gpu.py hold the same kernels to on bare buffers; it applies unchanged because
                    the operands are the same bf16 numbers
  db_l, column sum  (wg_db_scan_mask bit l clear: colsum_bf16 over the stored dZ)  the column sums of dZ_l, REL x max|ref|
  db_l, scan sum    (bit set: the backward scan adds its f32 dz BEFORE the bf16 store)  every term differs from the stored one
                    by at most half a bf16 ulp, 2^-9 |x|; as independent errors of variance at most (2^-9 x)^2 / 3, column j is
                    held to SIGMAS = 6 standard deviations, 6 . 2^-9 . sqrt(sum_r dZ[r][j]^2 / 3) + REL x max|ref|.  Derived
                    from the rounding model, not measured.  16 rows missing from such a sum move a column by about
                    4 x its dZ's RMS against a bound of 0.0068 x RMS x sqrt(rows): separated at every shape the tests use
                    (shown at 45 and at 9216 rows by tests/test_window_grads_ref.py).
                    NOTE on the model: bf16 keeps 8 significant bits, so half an ulp of x = m . 2^e (1 <= m < 2) is
                    2^-8 . 2^e = 2^-8 |x| / m -- between 2^-9 |x| and 2^-8 |x|, not at most 2^-9 |x|.  With m spread evenly in the
                    logarithm the errors' true standard deviation is 1.47 x the model's, so the bound stands at 4.1 true
                    standard deviations, not 6 (one column in 24000 beyond it by chance).  The bound is kept as specified;
                    tests/test_window_grads_ref.py draws its clean sums from the TRUE half-ulp and prints where they land
                    (0.95 of the bound at 45 rows).  The scans of this project in fact add the values they STORE (they round
                    first: `dbacc += bf2f(z)`), so on the device their sums land at 0.00 of this bound
  dK_0, context     rows Wp + n . ctx_dim ...: Ctx_n^T . S_n, S_n[c] = the sum of the rows of dZ_0 whose ctx[b][t][n] == c; f32
                    throughout, REL x max|ref| of the product
  dK_0, characters  rows [:Wp]: E_bf16^T . bf16(S), S[v] = the sum of the rows of dZ_0 with idx == v: the engine rounds S to
                    bf16 before the product, and so does the reference.  An entry of S whose f64 value lies within REL
                    (relative) of a bf16 rounding boundary may round either way: each such entry widens the bound of output
                    (w, j) by 2^-8 |E[v][w] . S[v][j]|.  Nothing else beyond REL x max|ref|; the number of entries near a
                    boundary is reported.
                    NOTE on the allowance: the two roundings of S = m . 2^e lie one bf16 step 2^-7 . 2^e = 2^-7 |S| / m apart,
                    which is MORE than 2^-8 |S| for every m < 2: a sum that the engine really rounds the other way than the
                    reference moves its outputs by up to twice the allowance.  Kept as specified, and reported as its own
                    part (CHARACTERS) so that it does not hide the other products
  padding           entries of dU, dK, db in rows and columns of padded hidden units: exactly 0

dE, the context tables' gradients and the regularisers: tests/table_grads.py, through the view's off_dlogits and with
regulariser-neutral tables.  Out of scope: stream groups -- the workspace holds the last group only.

A failure names the array, the layer, the 64 x 64 tile of the worst element and the route the stage took.
"""
import numpy as np

from oracle import lstm_oracle as O

REL = 1e-5
SIGMAS = 6.0
WG_KMAJOR, WG_SCAN_T, WG_TRANSPOSE, WG_SEGSUM, WG_PAIR_CTX = 1, 2, 4, 8, 16      # kl_window_view.wg_route (include/keraslm_hip.h)


CHARACTERS = "K0 characters"      # the part of K0 whose bound allows for sums near a rounding boundary


class GradMismatch(AssertionError):
    """`arrays`: the names of the gradient arrays beyond their bound (a set); `parts`: the same with K0 told apart into
    CHARACTERS and "K0 context n"; `failures`: one tuple per failed check"""

    def __init__(self, failures, where=""):
        super().__init__((where, "%d checks beyond their bound" % len(failures), [f[1:] for f in failures[:8]]))
        self.failures = failures
        self.parts = {f[0] for f in failures}
        self.arrays = {f[1] for f in failures}


def route_text(view):
    r = view.get("wg_route", 0)
    L = view["depth"]
    bits = lambda m: "".join(str((m >> l) & 1) for l in range(L))
    main = "+".join(n for b, n in ((WG_KMAJOR, "k-major"), (WG_SCAN_T, "scan-transposed"), (WG_TRANSPOSE, "transposes")) if r & b) or "?"
    layer0 = "segment sums" if r & WG_SEGSUM else ("one-hot, paired" if r & WG_PAIR_CTX else "one-hot")
    return "%s, pairs %s, db by scan %s, layer 0 %s" % (main, bits(view.get("wg_pair_mask", 0)), bits(view.get("wg_db_scan_mask", 0)), layer0)


def split_flat(flat, layout):
    """the engine's flat parameter-shaped array -> {name: [rows][cols]} by kl_param_layout (physical shapes)"""
    flat = np.asarray(flat)
    return {name: flat[off:off + rows * cols].reshape(rows, cols) for name, off, rows, cols in layout}


def operands(win):
    """`window_ref.read_window_padded`'s dict (or decode_window + decode_hd of an encoded one) -> per layer the time-major
    f64 operands: Hprev [TB][W] (blocks 0 .. T-1), Hnext [TB][W] (blocks 1 .. T), Hd [TB][W] or None, dZ [TB][4W]"""
    out = []
    for l in range(len(win["h"])):
        h, h0, dz = win["h"][l], win["h0"][l], win["dz"][l]
        B, T, W = h.shape
        blocks = np.concatenate([h0[None], h.transpose(1, 0, 2)]).astype(np.float64)      # [T+1][B][W]
        hd = win["hd"][l] if win.get("hd") is not None else None
        out.append(dict(Hprev=blocks[:T].reshape(T * B, W), Hnext=blocks[1:].reshape(T * B, W),
                        Hd=None if hd is None else hd.transpose(1, 0, 2).reshape(T * B, W).astype(np.float64),
                        dZ=dz.transpose(1, 0, 2, 3).reshape(T * B, 4 * W).astype(np.float64)))
    return out


def key_sums(keys, n_keys, dz):
    """S[k] = the sum of the rows of dz whose key is k (keys time-major, one per row)"""
    onehot = np.zeros((n_keys, dz.shape[0]))
    onehot[keys, np.arange(dz.shape[0])] = 1.0
    return onehot @ dz


def near_bf16_boundary(s, rel=REL):
    """where |s - the midpoint of the two bf16 numbers around s| <= rel |s|"""
    _m, e = np.frexp(s)                                    # |s| in [2^(e-1), 2^e): bf16 spacing 2^(e-8)
    ulp = np.ldexp(1.0, e - 8)
    frac = np.abs(s) / ulp
    frac -= np.floor(frac)
    return (np.abs(frac - 0.5) * ulp <= rel * np.abs(s)) & (s != 0)


def character_rows(E, S):
    """E [V][W] f32, S [V][cols] f64 -> (ref, bound, near): E_bf16^T . bf16(S), its bound per element and where S lies near a
    bf16 rounding boundary (see the module text)"""
    near = near_bf16_boundary(S)
    E = O.bf16_round(E).astype(np.float64)
    ref = E.T @ O.bf16_round(S).astype(np.float64)
    return ref, REL * np.abs(ref).max() + 2.0 ** -8 * (np.abs(E).T @ (np.abs(S) * near)), near


def scan_db_bound(dz, ref):
    """the bound of a bias gradient that the backward scan summed before its bf16 store, per column (see the module text)"""
    return SIGMAS * 2.0 ** -9 * np.sqrt((dz * dz).sum(axis=0) / 3.0) + REL * np.abs(ref).max()


def _tile(err_over_bound):
    r, c = np.unravel_index(np.argmax(np.where(np.isnan(err_over_bound), np.inf, err_over_bound)), err_over_bound.shape)
    return int(r), int(c)


def check_window_grads(win, idx, ctx, params, grads, layout, width=None, where="", raise_=True):
    """win: the decoded window at the padded width with "hd" and "view"; idx [B][T], ctx [B][T][n_ctx]: the window's inputs
    (all streams the kernels ran); params, grads: the engine's flat physical arrays (or dicts as `split_flat` gives them);
    layout: kl_param_layout's (name, offset, rows, cols); width: the model's own width where the engine padded it.
    -> {name: dict(ratio, err, bound, ...)}, ratio = the largest error / bound of the array (K0: of its worst part, and
    "parts": the ratio of each); raises GradMismatch naming every array beyond its bound -- or, with raise_=False, returns
    (report, GradMismatch or None)."""
    view = win["view"]
    L, Wp, B, T = view["depth"], view["width"], view["B"], view["T"]
    W = Wp if width is None else width
    P = params if isinstance(params, dict) else split_flat(params, layout)
    Gr = grads if isinstance(grads, dict) else split_flat(grads, layout)
    ops = operands(win)
    idx_tm = np.asarray(idx).T.reshape(-1)
    n_ctx = 0 if ctx is None else np.asarray(ctx).shape[2]
    route = route_text(view)
    report, bad = {}, []

    def hold(name, layer, got, ref, bound, rows0=0, part=None, **extra):
        got = np.asarray(got, dtype=np.float64)
        over = np.abs(got - ref) / np.maximum(bound, 1e-300)
        ratio = float(np.nanmax(over)) if not np.isnan(over).any() else float("nan")
        r, c = _tile(over)
        rep = dict(ratio=ratio, err=float(np.abs(got - ref)[r, c]), bound=float(np.broadcast_to(bound, ref.shape)[r, c]),
                   at=(rows0 + r, c), part=part or name, **extra)
        report.setdefault(name, []).append(rep)
        if not ratio <= 1.0:
            bad.append((part or name, name, "layer %d" % layer, "tile (%d, %d) of 64 x 64" % ((rows0 + r) // 64, c // 64),
                        "element (%d, %d)" % (rows0 + r, c), "error %.4g" % rep["err"], "bound %.4g" % rep["bound"],
                        "got %.6g" % got[r, c], "ref %.6g" % ref[r, c], "route: " + route) + tuple("%s %s" % kv for kv in extra.items()))

    def pads(name, layer, got, rows, part=None):
        """rows / columns of padded hidden units: exactly zero"""
        got = np.asarray(got)
        cols = np.zeros(4 * Wp, dtype=bool)
        for g in range(4):
            cols[g * Wp + W:(g + 1) * Wp] = True
        nz = (got[:, cols] != 0).any() or (rows and (got[W:Wp] != 0).any())
        if nz:
            at = np.argwhere(got[:, cols] != 0)[:1].tolist() or np.argwhere(got[W:Wp] != 0)[:1].tolist()
            bad.append((part or name, name, "layer %d" % layer, "non-zero entry in the padding", at, "route: " + route))
            report.setdefault(name, []).append(dict(ratio=float("inf"), pad=True, part=part or name))

    for l in range(L):
        o = ops[l]
        dz = o["dZ"]
        ref = o["Hprev"].T @ dz
        hold("U%d" % l, l, Gr["U%d" % l], ref, REL * np.abs(ref).max())
        pads("U%d" % l, l, Gr["U%d" % l], True)
        ref = dz.sum(axis=0)[None]
        by_scan = bool((view.get("wg_db_scan_mask", 0) >> l) & 1)
        bound = scan_db_bound(dz, ref)[None] if by_scan else REL * np.abs(ref).max()
        hold("b%d" % l, l, Gr["b%d" % l], ref, bound, by_scan=by_scan)
        pads("b%d" % l, l, Gr["b%d" % l], False)
        name = "K%d" % l
        if l > 0:
            X = ops[l - 1]["Hd"] if ops[l - 1]["Hd"] is not None else ops[l - 1]["Hnext"]
            ref = X.T @ dz
            hold(name, l, Gr[name], ref, REL * np.abs(ref).max(), masked_input=ops[l - 1]["Hd"] is not None)
            pads(name, l, Gr[name], True)
            continue
        # layer 0, the characters' rows: the sums pass through bf16
        V = P["E"].shape[0]
        S = key_sums(idx_tm, V, dz)
        ref, bound, near = character_rows(P["E"], S)
        hold(name, l, Gr[name][:Wp], ref, bound, part=CHARACTERS, near_boundary=int(near.sum()), sums=int((S != 0).sum()))
        pads(name, l, Gr[name][:Wp], True, part=CHARACTERS)
        ctx_dim = (Gr[name].shape[0] - Wp) // max(n_ctx, 1)
        for n in range(n_ctx):
            tab = np.asarray(P["Ctx%d" % n], dtype=np.float64)
            Sn = key_sums(np.asarray(ctx)[:, :, n].T.reshape(-1), tab.shape[0], dz)
            ref = tab.T @ Sn
            rows = slice(Wp + n * ctx_dim, Wp + (n + 1) * ctx_dim)
            hold(name, l, Gr[name][rows], ref, REL * np.abs(ref).max(), rows0=rows.start, part="K0 context %d" % n, context=n)
            pads(name, l, Gr[name][rows], False, part="K0 context %d" % n)
    out = {}
    for name, reps in report.items():
        worst = max(reps, key=lambda r: np.inf if np.isnan(r["ratio"]) else r["ratio"])
        out[name] = dict(worst, near_boundary=sum(r.get("near_boundary", 0) for r in reps), sums=sum(r.get("sums", 0) for r in reps),
                         parts={r["part"]: r["ratio"] for r in reps if not r.get("pad")})
    err = GradMismatch(bad, where) if bad else None
    if not raise_:
        return out, err
    if err:
        raise err
    return out


def ratio_line(report, depth):
    """'U 0.12 0.10 | K (0.30 0.05) 0.11 | b ...': the ratio error / bound per array kind and layer, K0 as (characters,
    worst context variable), then how many of layer 0's character sums lay near a rounding boundary"""
    k0 = report["K0"]["parts"]
    ctxs = [v for k, v in k0.items() if k != CHARACTERS]
    cell = lambda k, l: "(%.2f %.2f)" % (k0[CHARACTERS], max(ctxs) if ctxs else 0.0) if (k, l) == ("K", 0) else "%.2f" % report["%s%d" % (k, l)]["ratio"]
    return " | ".join("%s %s" % (k, " ".join(cell(k, l) for l in range(depth))) for k in "UKb") + \
        " | near a boundary %d of %d sums" % (report["K0"]["near_boundary"], report["K0"]["sums"])
