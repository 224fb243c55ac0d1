"""The table-gradient checker (tests/table_grads.py) without a GPU: a window built from the bf16-storage oracle with
regulariser-neutral tables and laid out as a `kl_window_view` describes it (depth 2, width 100 padded to 128, 30 characters in
32 table rows, two context variables, dropout masks, dummy streams, `dlogits` behind off_dlogits), "engine gradients" from
f32 products of it in the engine's order (dE = output part, += input part, += regulariser; the regularisers by
`table_grads.restate_f32`), and then one corruption at a time, each at the smallest extent a kernel bug would have -- one
16-row block, one key, one row.  Each must fail, on its own array and on no other.  The regulariser kernels' mistakes are told
apart on single tables by `check_regulariser`, as tests/test_table_grads_gpu.py holds the kernels themselves: under neutral
tables the window hardly sees the regularisers (that is what makes the tables neutral), and the value is not a gradient array.

Every corruption of the list was separated; the smallest margin is "S not rounded to bf16", whose worst element lies
at 1.4 x its bound here (run with -s for every figure).  The f32 restatement of the regulariser kernels stays at or below 0.5
of the hook's bounds on every case of the GPU table (the largest: 0.33, row 0 of a neutral character table of 17 rows)."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests import table_grads as TG
from tests import window_grads as WG
from tests import window_ref as R
from tests.gradcheck import cached_weights
from tests.test_window_grads_ref import CTX_DIM, CTX_VOCAB, _f32, _layout

CASE = R._case("tables-small", "none", {}, (2, 100, 30, 20, 9), "", "", n_ctx=2)
WP, VP = 128, 32
EDGE_IDS = (0, 1, CTX_VOCAB - 2, CTX_VOCAB - 1)


def _dlogits(case, w, inp):
    """[B*T][V] time-major: the gradient of the logits of the bf16-storage oracle's window, as it stores it"""
    cfg = O.ModelConfig(case.depth, case.width, case.voc, case.n_ctx)
    L, B, T, V = case.depth, case.B, case.T, case.voc
    st = [inp["states"][:, k] for k in range(2 * L)]
    om = [None] + [inp["masks"][l] for l in range(1, L)]
    probs, _st, _cache = O.forward_window(cfg, w, inp["idx"], inp["ctx"], st, om, keep_cache=True, storage=O.Storage(L))
    tgt = inp["tgt"]
    valid = tgt >= 0
    tsafe = np.where(valid, tgt, 0)
    pt = np.take_along_axis(probs, tsafe[..., None], axis=-1)[..., 0]
    active = valid & (pt >= 1e-7) & (pt <= 1 - 1e-7)
    onehot = np.zeros_like(probs)
    np.put_along_axis(onehot, tsafe[..., None], active[..., None].astype(probs.dtype), axis=-1)
    dlog = (probs * active[..., None] - onehot) / (inp["n_real"] * T)
    return O.bf16_round(dlog.transpose(1, 0, 2).reshape(T * B, V))


def edge_contexts(inp, n_ctx):
    """the context ids of the first real streams overwritten so that 0, 1, R-2 and R-1 all occur where B allows: the rows
    with special regulariser terms and the edges of the sums (shared with tests/test_table_grads_gpu.py)"""
    if n_ctx:
        for k in range(min(len(EDGE_IDS), inp["n_real"])):
            for n in range(n_ctx):
                inp["ctx"][k, :, n] = EDGE_IDS[(k + n) % len(EDGE_IDS)]
    return inp


@pytest.fixture(scope="module")
def window():
    case = CASE
    L, W, V, B, T = case.depth, case.width, case.voc, case.B, case.T
    w = TG.neutral_tables(cached_weights(L, W, V, case.n_ctx, 4, 0.3))
    inp = R.make_inputs(case)
    inp["ctx"] = np.random.default_rng(5).integers(0, CTX_VOCAB, (B, T, case.n_ctx))      # (contexts that change inside the window)
    edge_contexts(inp, case.n_ctx)
    emu = R.references(case, w, inp, O.Storage(L), tag="tables-small-neutral")
    arrs = {k: [a.copy() for a in v] for k, v in emu.items()}
    arrs["h0"] = [O.bf16_round(inp["states"][:, 2 * l]) for l in range(L)]
    arrs["c0"] = [inp["states"][:, 2 * l + 1] for l in range(L)]
    arrs["cT"] = [emu["c"][l][:, -1] for l in range(L)]
    arrs["hd"] = [None] + [O.bf16_round(emu["h"][l] * inp["masks"][l][:, None, :]) for l in range(1, L)]
    view = dict(depth=L, width=WP, B=B, T=T, g_interleaved=0, c_in_cb=0, dh_bf16=0, p_bf16_mask=0, scan2_rows=0,
                wg_route=WG.WG_TRANSPOSE | WG.WG_SEGSUM, wg_pair_mask=0, wg_db_scan_mask=0, out_route=TG.OUT_LOGITS_W128)
    off = 256
    for key, size in (("off_H", (T + 1) * B * WP * 2), ("off_C", (T + 1) * B * WP * 4), ("off_Cb", (T + 1) * B * WP * 2),
                      ("off_G", T * B * 4 * WP * 2), ("off_dZ", T * B * 4 * WP * 2), ("off_Hd", T * B * WP * 2)):
        view[key] = [off + l * size for l in range(L)]
        off += L * size
    view["off_Hd"][0] = 0
    view["off_dlogits"], view["ld_dlogits"] = off, VP
    ws = R.encode_window(arrs, view, fill=0)
    R.encode_dlogits(ws, view, _dlogits(case, w, inp))
    win = R.decode_window(ws, view)
    win["hd"] = R.decode_hd(ws, view)
    win["dlogits"] = R.decode_dlogits(ws, view)
    win["view"] = view
    assert win["dlogits"].shape == (B * T, VP) and win["dlogits"][:, :V].any() and not win["dlogits"][:, V:].any()
    layout, n_params = _layout(L, WP, V, case.n_ctx)
    params = np.zeros(n_params, dtype=np.float32)
    P = WG.split_flat(params, layout)
    P["E"][:, :W] = w["E"]
    for n in range(case.n_ctx):
        P["Ctx%d" % n][:] = w["Ctx%d" % n]
    K0 = P["K0"].reshape(-1, 4, WP)      # (gate blocks of the padded width; padded units: zeros)
    K0[:W, :, :W] = w["K0"][:W].reshape(W, 4, W)
    K0[WP:, :, :W] = w["K0"][W:].reshape(-1, 4, W)
    out = dict(win=win, inp=inp, params=params, P=P, layout=layout, n_params=n_params, ops=WG.operands(win))
    out["grads"] = _engine(out)
    return out


def _engine(window, kind=None):
    """what a correct engine delivers -- f32 products, the three parts of dE added one after the other --, or with `kind`
    one thing wrong; -> the flat gradient array"""
    win, inp, P, ops = window["win"], window["inp"], window["P"], window["ops"]
    B, T, V, W = CASE.B, CASE.T, CASE.voc, CASE.width
    flat = np.zeros(window["n_params"], dtype=np.float32)
    G = WG.split_flat(flat, window["layout"])
    dl = _f32(win["dlogits"]).copy()
    top = ops[-1]
    X = _f32(top["Hd"])
    rows = np.ones(B * T, dtype=bool)
    if kind == "H blocks 0..T-1 as the top operand":
        X = X.copy()
        blk = slice(3 * B, 3 * B + 16)      # one 16-row block: step 3, streams 0 .. 15
        X[blk] = _f32(ops[-1]["Hd"])[2 * B:2 * B + 16]
    elif kind == "unmasked top outputs":
        X = X.copy()
        X[3 * B:3 * B + 16] = _f32(top["Hnext"])[3 * B:3 * B + 16]
    elif kind == "dlogits without its last 16 rows":
        rows[-16:] = False
        assert dl[-16:].any()      # (streams 4 .. 7 of the last step are real ones)
    elif kind == "non-zero dlogits column >= V":
        dl[5 * B + 2, V + 1] = 2.0 ** -20      # (the product does not read it: columns [:V] only)
    G["E"][:] = dl[rows][:, :V].T @ X[rows]
    # layer 0 through the tables
    dz = _f32(ops[0]["dZ"])
    idx_tm = inp["idx"].T.reshape(-1)
    S = _f32(WG.key_sums(idx_tm, V, dz))
    if kind == "one character's sum missing":
        v = int(idx_tm[0])
        S[v] = 0
    Sb = S if kind == "S not rounded to bf16" else O.bf16_round(S)
    G["E"][:] += Sb @ O.bf16_round(P["K0"][:WP]).T
    G["E"][:] += TG.restate_f32(P["E"], 0)[0]
    for n in range(CASE.n_ctx):
        keys = inp["ctx"][:, :, n].T.reshape(-1)
        Sn = _f32(WG.key_sums(keys, CTX_VOCAB, dz))
        krows = slice(WP + n * CTX_DIM, WP + (n + 1) * CTX_DIM)
        if kind == "dCtx_1 with the K0 rows of variable 0" and n == 1:
            krows = slice(WP, WP + CTX_DIM)
        if kind == "dCtx_0 without context id R-1" and n == 0:
            assert Sn[CTX_VOCAB - 1].any()
            Sn[CTX_VOCAB - 1] = 0
        if kind == "dCtx_0 through the other stride convention" and n == 0:
            Sn = np.ascontiguousarray(Sn.reshape(Sn.shape[1], Sn.shape[0]).T)      # element [col][r] at r + col * R instead of r * N + col
        G["Ctx%d" % n][:] = Sn @ P["K0"][krows].T
        G["Ctx%d" % n][:] += TG.restate_f32(P["Ctx%d" % n], 1)[0]
    return flat


def _check(window, grads, win=None, **kw):
    inp = window["inp"]
    return TG.check_table_grads(win or window["win"], inp["idx"], inp["ctx"], window["params"], grads, window["layout"], width=CASE.width,
                                dummy_from=inp["n_real"], where="ref", **kw)


def test_clean_window_passes(window):
    rep = _check(window, window["grads"])
    print("ratios:", TG.ratio_line(rep), "| precondition:", TG.precondition_line(rep))
    assert set(rep) == {"E", "Ctx0", "Ctx1"}
    assert all(v["ratio"] < 0.5 for v in rep.values()), rep      # (f32 products of 180 rows: far inside)
    assert rep["E"]["masked_top"] and rep["E"]["sums"] > 0
    inp = window["inp"]
    assert all(np.isin(EDGE_IDS, inp["ctx"][:inp["n_real"], :, n]).all() for n in range(CASE.n_ctx))
    assert TG.route_text(window["win"]["view"]).endswith("output layer: logits by one kernel with dH (width 128), dH by with the logits, "
                                                         "dE over dlogits^T")


WINDOW_KINDS = {"H blocks 0..T-1 as the top operand": "E", "unmasked top outputs": "E", "dlogits without its last 16 rows": "E",
                "non-zero dlogits column >= V": "E", "one character's sum missing": "E", "S not rounded to bf16": "E",
                "dCtx_1 with the K0 rows of variable 0": "Ctx1", "dCtx_0 without context id R-1": "Ctx0",
                "dCtx_0 through the other stride convention": "Ctx0"}


@pytest.mark.parametrize("kind", list(WINDOW_KINDS))
def test_one_corruption_fails_on_its_array(window, kind):
    name = WINDOW_KINDS[kind]
    flat = _engine(window, kind)
    win = window["win"]
    if kind.startswith("non-zero dlogits"):
        win = dict(win, dlogits=win["dlogits"].copy())
        win["dlogits"][5 * CASE.B + 2, CASE.voc + 1] = 2.0 ** -20
    rep, err = _check(window, flat, win=win, raise_=False)
    assert err is not None, (kind, rep[name])
    print("%-45s %s ratio %.3g (%s)" % (kind, name, rep[name]["ratio"], ", ".join(sorted(err.parts))))
    assert err.arrays == {name}, (kind, err.arrays)
    text = str(err)
    assert "route: transposes" in text and "output layer: logits by one kernel with dH" in text
    if kind.startswith("non-zero dlogits"):
        assert err.parts == {"E output: dlogits columns >= V"} and rep["E"]["ratio"] < 0.5
    else:
        assert "element (" in text and "smallest that explains it: " in text
    if name.startswith("Ctx") and "stride" not in kind:
        assert err.parts == {"%s context %s" % (name, name[3])}


def test_exact_checks(window):
    """dlogits rows of a dummy stream and dE's padded columns must be exactly zero; a view from before the fields has no dlogits"""
    win = dict(window["win"], dlogits=window["win"]["dlogits"].copy())
    win["dlogits"][2 * CASE.B + CASE.B - 1, 3] = 2.0 ** -30
    _rep, err = _check(window, window["grads"], win=win, raise_=False)
    assert err is not None and err.parts == {"E output: dlogits rows of dummy streams"}
    flat = window["grads"].copy()
    WG.split_flat(flat, window["layout"])["E"][4, CASE.width] = 1e-30
    _rep, err = _check(window, flat, raise_=False)
    assert err is not None and err.parts == {"E padding: columns of padded hidden units"}
    old = {k: v for k, v in window["win"]["view"].items() if k not in ("out_route", "off_dlogits", "ld_dlogits")}
    import torch
    ws = torch.zeros(R.window_bytes(old), dtype=torch.uint8)
    assert R.decode_dlogits(ws, old) is None and len(R.decode_window(ws, old)["h"]) == CASE.depth
    assert TG.route_text(old).endswith("dE over dlogits^T")


def test_precondition_is_asserted_from_the_references(window):
    """the usual tables of the same model: the regularisers' gradient is 1e2 .. 1e5 times the part under test"""
    w = cached_weights(CASE.depth, CASE.width, CASE.voc, CASE.n_ctx, 4, 0.3)
    params = window["params"].copy()
    P = WG.split_flat(params, window["layout"])
    P["E"][:, :CASE.width] = w["E"]
    P["Ctx0"][:] = w["Ctx0"]
    inp = window["inp"]
    args = (window["win"], inp["idx"], inp["ctx"], params, window["grads"], window["layout"])
    with pytest.raises(TG.Precondition) as err:
        TG.check_table_grads(*args, width=CASE.width)
    assert set(err.value.args[0][2]) == {"E", "Ctx0"}
    rep, _err = TG.check_table_grads(*args, width=CASE.width, raise_=False, precondition=False)
    print("precondition:", TG.precondition_line(rep))
    assert rep["E"]["precondition"][0] > 10 * rep["E"]["precondition"][1]


def test_neutral_tables():
    w = cached_weights(2, 100, 30, 2, 4, 0.3)
    n = TG.neutral_tables(w)
    assert all(n[k] is w[k] for k in w if k[0] in "KUb")
    E = n["E"].astype(np.float64)
    assert np.allclose((E[1:] ** 2).sum(axis=1), 1.0, atol=1e-6) and np.allclose(E[0], E[1:].mean(axis=0), atol=1e-8)
    for k in ("Ctx0", "Ctx1"):
        C = n[k].astype(np.float64)
        assert not C[0].any() and np.array_equal(C[-1], C[-2]) and np.array_equal(C[1:-1:2], -C[2:-1:2])
        assert np.allclose((C[1:] ** 2).sum(axis=1), 1e-6, rtol=1e-5)
        g = O.regulariser_grads(O.ModelConfig(1, 10, 0, 1), {"E": np.zeros((0, 10)), "Ctx0": n[k]})["Ctx0"]
        assert np.abs(g).max() < 1e-4      # (init_weights' table at 0.3: 1e2)


@pytest.mark.parametrize("case", TG.REGULARISER_CASES, ids=lambda c: "%s-%dx%d-%s" % ("ctx" if c[0] else "char", c[1], c[2], c[4]))
def test_f32_restatement_stays_below_half_the_bounds(case):
    X = TG.regulariser_case_table(case)
    grad, value = TG.restate_f32(X, case[0])
    rep = TG.check_regulariser(X, case[0], grad, value, where=case)
    print(case, "row 0 %.3f | rows >= 1 %.3f | value %.3f" % (rep["row0"], rep["body"], rep["value"]))
    assert max(rep["row0"], rep["body"], rep["value"]) <= 0.5, rep


# variant -> per rule (None: the rule has no such term) the parts of `check_regulariser` that MUST fail and those that may:
# the statistics (mean, s1) feed both the gradient and the value, so a wrong one may show in both; a mistake in the apply pass
# shows in one.  FINDING: the characters' VALUE does not separate "mean over R" at 60 rows (0.42 of its bound: the mean, 0.04,
# enters through (x - mean)^2 beside x of 0.3); row 0 of the gradient does, at 214 x its bound.
_ALL = {"row 0", "rows >= 1", "value"}
REG_KINDS = {"smoothness from row 1": (None, ({"rows >= 1"}, {"rows >= 1"})), "s1 with row R-1": (None, ({"rows >= 1", "value"},) * 2),
             "mean over R": (({"row 0"}, {"row 0", "value"}), ({"row 0", "value"},) * 2),
             "constants swapped": ((_ALL, _ALL), (_ALL, _ALL)),
             "no row-0 term": (({"row 0", "value"},) * 2, ({"row 0"}, {"row 0"})), "value without smoothness": (None, ({"value"}, {"value"}))}


@pytest.mark.parametrize("variant", TG.VARIANTS)
def test_one_regulariser_mistake_fails_on_its_part(variant):
    """on oracle.init_weights' tables at 0.3 (60 x 128 with a padded width, 200 x 10) and on the smallest context table with all
    terms (4 x 10): the parts the mistake reaches fail and no other"""
    for rule, want in enumerate(REG_KINDS[variant]):
        if want is None:
            continue
        for case in ((0, 60, 128, 100, 0.3),) if rule == 0 else ((1, 200, 10, None, 0.3), (1, 4, 10, None, 0.3)):
            X = TG.regulariser_case_table(case)
            grad, value = TG.restate_f32(X, rule, variant)
            rep = TG.check_regulariser(X, rule, grad, value, raise_=False)
            print("%-26s %s row 0 %.3g | rows >= 1 %.3g | value %.3g" % (variant, case[:3], rep["row0"], rep["body"], rep["value"]))
            assert want[0] <= rep["failed"] <= want[1], (variant, case, rep)
            with pytest.raises(AssertionError, match="regulariser"):
                TG.check_regulariser(X, rule, grad, value)
