"""The weight-gradient checker (tests/window_grads.py) without a GPU: a window built from the bf16-storage oracle and laid out
as a `kl_window_view` describes it (depth 3, width 100 padded to 128, two context variables, dropout masks, dummy streams),
"engine gradients" from f32 products of it, and then one corruption at a time of the kinds this stage can produce -- each
must fail, and on exactly the array it belongs to.  This is the evidence that the bounds of tests/window_grads.py are tight
enough for what tests/test_window_grads_gpu.py relies on them for.

The scan-summed bias bound separates 16 missing rows at 200 rows here and, on synthetic dZ, at 45 and at 9216 rows (the
smallest and the largest row counts of the GPU cases whose scans sum db): no shape is left out."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests import window_grads as WG
from tests import window_ref as R
from tests.gradcheck import cached_weights

CASE = R._case("grads-small", "none", {}, (3, 100, 30, 40, 5), "", "", n_ctx=2)
WP = 128
CTX_VOCAB, CTX_DIM = 200, 10
DB_BY_SCAN = 0b010      # layer 1's bias gradient as a backward scan sums it, the others as column sums


def _layout(L, Wp, V, n_ctx):
    out, off = [], 0
    shapes = [("E", V, Wp)] + [("Ctx%d" % n, CTX_VOCAB, CTX_DIM) for n in range(n_ctx)]
    for l in range(L):
        shapes += [("K%d" % l, Wp + (n_ctx * CTX_DIM if l == 0 else 0), 4 * Wp), ("U%d" % l, Wp, 4 * Wp), ("b%d" % l, 1, 4 * Wp)]
    for name, rows, cols in shapes:
        out.append((name, off, rows, cols))
        off += rows * cols
    return out, off


@pytest.fixture(scope="module")
def window():
    """the decoded window, its inputs, the physical parameters, the layout and the clean f32 "engine gradients\""""
    case = CASE
    L, W, V, B, T = case.depth, case.width, case.voc, case.B, case.T
    w = cached_weights(L, W, V, case.n_ctx, 4, 0.3)
    inp = R.make_inputs(case)
    inp["ctx"] = np.random.default_rng(5).integers(0, CTX_VOCAB, (B, T, case.n_ctx))      # (contexts that change inside the window)
    emu = R.references(case, w, inp, O.Storage(L))
    arrs = {k: [a.copy() for a in v] for k, v in emu.items()}
    arrs["h0"] = [O.bf16_round(inp["states"][:, 2 * l]) for l in range(L)]
    arrs["c0"] = [inp["states"][:, 2 * l + 1] for l in range(L)]
    arrs["cT"] = [emu["c"][l][:, -1] for l in range(L)]
    arrs["hd"] = [None] + [O.bf16_round(emu["h"][l] * inp["masks"][l][:, None, :]) for l in range(1, L)]
    view = dict(depth=L, width=WP, B=B, T=T, g_interleaved=0, c_in_cb=0, dh_bf16=0, p_bf16_mask=0, scan2_rows=0,
                wg_route=WG.WG_TRANSPOSE | WG.WG_SEGSUM, wg_pair_mask=0, wg_db_scan_mask=DB_BY_SCAN)
    off = 256
    for key, size in (("off_H", (T + 1) * B * WP * 2), ("off_C", (T + 1) * B * WP * 4), ("off_Cb", (T + 1) * B * WP * 2),
                      ("off_G", T * B * 4 * WP * 2), ("off_dZ", T * B * 4 * WP * 2), ("off_Hd", T * B * WP * 2)):
        view[key] = [off + l * size for l in range(L)]
        off += L * size
    view["off_Hd"][0] = 0
    ws = R.encode_window(arrs, view, fill=0)      # (padded units: zeros, as the engine's zero weights leave them)
    win = R.decode_window(ws, view)
    win["hd"] = R.decode_hd(ws, view)
    win["view"] = view
    assert win["hd"][0] is None and np.array_equal(win["hd"][2][:, :, :W], arrs["hd"][2]) and not win["hd"][2][:, :, W:].any()
    layout, n_params = _layout(L, WP, V, case.n_ctx)
    params = np.zeros(n_params, dtype=np.float32)
    P = WG.split_flat(params, layout)
    P["E"][:, :W] = w["E"]
    for n in range(case.n_ctx):
        P["Ctx%d" % n][:] = w["Ctx%d" % n]
    return dict(win=win, inp=inp, params=params, layout=layout, ops=WG.operands(win), grads=_products(win, inp, P, layout, n_params))


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _unrounded(dz, rng):
    """f32 values that the stored bf16 dz could have been rounded from: uniformly within half a bf16 ulp of each (the TRUE
    half-ulp, 2^-8 . 2^e for |x| in [2^e, 2^(e+1)) -- see the note in tests/window_grads.py)"""
    _m, e = np.frexp(dz)
    return _f32(dz + rng.uniform(-1.0, 1.0, dz.shape) * 0.999 * np.ldexp(1.0, e - 9) * (dz != 0))


def _products(win, inp, P, layout, n_params):
    """what a correct engine delivers: every product with f32 accumulation"""
    ops = WG.operands(win)
    rng = np.random.default_rng(9)
    flat = np.zeros(n_params, dtype=np.float32)
    G = WG.split_flat(flat, layout)
    for l, o in enumerate(ops):
        dz = _f32(o["dZ"])
        G["U%d" % l][:] = _f32(o["Hprev"]).T @ dz
        G["b%d" % l][0] = _unrounded(o["dZ"], rng).sum(axis=0) if (DB_BY_SCAN >> l) & 1 else dz.sum(axis=0)
        if l > 0:
            X = ops[l - 1]["Hd"] if ops[l - 1]["Hd"] is not None else ops[l - 1]["Hnext"]
            G["K%d" % l][:] = _f32(X).T @ dz
    dz = _f32(ops[0]["dZ"])
    S = _f32(WG.key_sums(inp["idx"].T.reshape(-1), P["E"].shape[0], dz))
    G["K0"][:WP] = O.bf16_round(P["E"]).T @ O.bf16_round(S)
    for n in range(inp["ctx"].shape[2]):
        Sn = _f32(WG.key_sums(inp["ctx"][:, :, n].T.reshape(-1), CTX_VOCAB, dz))
        G["K0"][WP + n * CTX_DIM:WP + (n + 1) * CTX_DIM] = P["Ctx%d" % n].T @ Sn
    return flat


def _check(window, grads):
    return WG.check_window_grads(window["win"], window["inp"]["idx"], window["inp"]["ctx"], window["params"], grads,
                                 window["layout"], width=CASE.width, where="ref")


def test_clean_products_pass(window):
    rep = _check(window, window["grads"])
    print("ratios:", WG.ratio_line(rep, CASE.depth))
    assert set(rep) == {"%s%d" % (k, l) for k in "UKb" for l in range(CASE.depth)}
    assert all(v["ratio"] < 0.5 for k, v in rep.items() if k != "b1"), rep      # (f32 products of 200 rows: far inside)
    assert rep["b1"]["by_scan"] and not rep["b0"]["by_scan"]
    assert rep["K2"]["masked_input"]


def _real_rows(window, first, count):
    """`count` consecutive time-major rows from `first` on that all belong to real streams"""
    B, n_real = CASE.B, window["inp"]["n_real"]
    rows = np.arange(first, first + count)
    assert (rows % B < n_real).all()
    return rows


def _corrupt(window, kind):
    ops = window["ops"]
    flat = window["grads"].copy()
    G = WG.split_flat(flat, window["layout"])
    W, B = CASE.width, CASE.B
    keep = np.ones(ops[0]["dZ"].shape[0], dtype=bool)
    if kind.startswith("32 rows"):
        keep[np.r_[_real_rows(window, B, 24), _real_rows(window, 2 * B, 8)]] = False      # (rows 40 .. 71 minus the dummy streams' zeros)
        keep[B:B + 32] = False
    if kind == "32 rows of dU":
        G["U1"][:] = _f32(ops[1]["Hprev"][keep]).T @ _f32(ops[1]["dZ"][keep])
        return flat, "U1"
    if kind == "32 rows of dK":
        G["K2"][:] = _f32(ops[1]["Hd"][keep]).T @ _f32(ops[2]["dZ"][keep])
        return flat, "K2"
    if kind == "32 rows of the character sums":
        dz = _f32(ops[0]["dZ"][keep])
        S = _f32(WG.key_sums(window["inp"]["idx"].T.reshape(-1)[keep], CASE.voc, dz))
        E = WG.split_flat(window["params"], window["layout"])["E"]
        G["K0"][:WP] = O.bf16_round(E).T @ O.bf16_round(S)
        return flat, "K0"
    if kind == "32 rows of a context sum":
        dz = _f32(ops[0]["dZ"][keep])
        Sn = _f32(WG.key_sums(window["inp"]["ctx"][:, :, 1].T.reshape(-1)[keep], CTX_VOCAB, dz))
        G["K0"][WP + CTX_DIM:WP + 2 * CTX_DIM] = WG.split_flat(window["params"], window["layout"])["Ctx1"].T @ Sn
        return flat, "K0"
    if kind == "tile from the neighbouring layer's dZ":
        G["U1"][0:64, 64:128] = _f32(ops[1]["Hprev"][:, 0:64]).T @ _f32(ops[2]["dZ"][:, 64:128])
        return flat, "U1"
    if kind == "H blocks 1..T for dU":
        G["U0"][:] = _f32(ops[0]["Hnext"]).T @ _f32(ops[0]["dZ"])
        return flat, "U0"
    if kind == "H where Hd is due":
        G["K2"][:] = _f32(ops[1]["Hnext"]).T @ _f32(ops[2]["dZ"])
        return flat, "K2"
    if kind == "16 rows of a scan-summed db":
        keep[_real_rows(window, 3 * B, 16)] = False
        G["b1"][0] = _unrounded(ops[1]["dZ"][keep], np.random.default_rng(9)).sum(axis=0)
        return flat, "b1"
    if kind == "16 rows of a column-summed db":
        keep[_real_rows(window, 3 * B, 16)] = False
        G["b2"][0] = _f32(ops[2]["dZ"][keep]).sum(axis=0)
        return flat, "b2"
    if kind == "twice the product":
        G["U2"][:] *= 2
        return flat, "U2"
    if kind == "twice the bias sum":
        G["b1"][:] *= 2
        return flat, "b1"
    if kind == "non-zero pad column":
        G["K1"][3, 2 * WP + W] = 1e-30
        return flat, "K1"
    if kind == "non-zero pad row":
        G["U0"][W + 1, 5] = -1e-30
        return flat, "U0"
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["32 rows of dU", "32 rows of dK", "32 rows of the character sums", "32 rows of a context sum",
                                  "tile from the neighbouring layer's dZ", "H blocks 1..T for dU", "H where Hd is due",
                                  "16 rows of a scan-summed db", "16 rows of a column-summed db", "twice the product",
                                  "twice the bias sum", "non-zero pad column", "non-zero pad row"])
def test_one_corruption_fails_on_its_array(window, kind):
    flat, name = _corrupt(window, kind)
    with pytest.raises(WG.GradMismatch) as err:
        _check(window, flat)
    assert err.value.arrays == {name}, (kind, err.value.arrays)
    text = str(err.value)
    assert "layer %s" % name[1] in text and "route: transposes" in text and ("tile (" in text or "padding" in text)
    if kind.startswith("tile"):
        assert "tile (0, 1) of 64 x 64" in text


@pytest.mark.parametrize("rows", [45, 9216])
def test_scan_db_bound_separates_16_rows(rows):
    """synthetic dZ of the GPU cases' smallest and largest row counts whose scans sum db: the rounding model's sum passes at
    the bound (the largest of 512 columns is printed), 16 missing rows fail in most columns"""
    rng = np.random.default_rng(rows)
    dz = O.bf16_round(rng.standard_normal((rows, 512)) * 1e-3).astype(np.float64)
    ref = dz.sum(axis=0)
    bound = WG.scan_db_bound(dz, ref)
    got = _unrounded(dz, rng).sum(axis=0, dtype=np.float64)
    ratio = np.abs(got - ref) / bound
    print("rows %d: clean ratio max %.3f" % (rows, ratio.max()))
    assert ratio.max() <= 1.0
    missing = _unrounded(dz[16:], rng).sum(axis=0, dtype=np.float64)
    over = np.abs(missing - ref) / bound
    assert (over > 1).mean() > 0.5 and over.max() > 4, (over.max(), (over > 1).mean())


def test_near_boundary_entries():
    """bf16 numbers lie 2^-7 apart in [1, 2): 1 + 2^-8 is a boundary; the test is relative to the value"""
    s = np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 5e-6, 1.0 + 2.0 ** -8 - 2e-5, 1.0, 0.0, -(3.0 + 2.0 ** -7) * 2.0 ** -20, 1.5 + 2.0 ** -8 + 1.4e-5])
    assert WG.near_bf16_boundary(s).tolist() == [True, True, False, False, False, True, True]


def test_allowance_of_a_sum_near_a_boundary():
    """a character sum within 1e-5 of a bf16 boundary gets an allowance of 2^-8 |E S| per output, a sum away from a boundary
    none"""
    rng = np.random.default_rng(2)
    V, W, cols = 30, 16, 8
    E = O.bf16_round(rng.standard_normal((V, W)) * 0.3)
    S = rng.standard_normal((V, cols)) * 1e-3
    S[3, 2] = (1.0 + 2.0 ** -8) * 2.0 ** -10 * (1.0 + 3e-6)      # just above the boundary between 2^-10 and 2^-10 (1 + 2^-7)
    ref, bound, near = WG.character_rows(E, S)
    assert near.sum() == 1 and near[3, 2]
    Sb = O.bf16_round(S).astype(np.float64)
    assert Sb[3, 2] == 2.0 ** -10 * (1.0 + 2.0 ** -7)
    inside = lambda: (np.abs(E.astype(np.float64).T @ Sb - ref) <= bound).all()
    assert inside()
    # the allowance per flagged entry is 2^-8 |E S|: half the step to the other rounding at this S (see the note in the
    # module text of tests/window_grads.py) -- so the other rounding is NOT accepted, and neither is anything further away
    Sb[3, 2] = 2.0 ** -10 * (1.0 + 2.0 ** -8)
    assert inside()
    Sb[3, 2] = 2.0 ** -10
    assert not inside()
    Sb = O.bf16_round(S).astype(np.float64)
    Sb[4, 1] += np.sign(Sb[4, 1]) * 2.0 ** (np.frexp(Sb[4, 1])[1] - 8)      # an entry away from any boundary, one bf16 step off
    assert not near[4, 1] and not inside()
