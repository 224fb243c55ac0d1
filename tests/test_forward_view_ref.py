"""tests/forward_view.py on the CPU: its decoders round-trip, its checker raises on one planted error of each kind, and its
cases -- decided from the oracle alone -- keep |h| < 1 (so that the planes must be the split of H) and give the P1
emulation an error of its own to measure against.  No GPU, no library: the arrays are laid out by `encode_forward`."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests import forward_view as F

DEPTH, WIDTH, WP, VOC, B, T = 3, 100, 128, 30, 5, 4


def _weights(depth, width, voc, n_ctx):
    from tests.gradcheck import cached_weights
    return cached_weights(depth, width, voc, n_ctx, 4, 0.5)


@pytest.fixture(scope="module")
def window():
    """a correct window as fwd_split_layers would leave it, from the f32 oracle: width 100 padded to 128, P1 = layer 2's gate inputs"""
    case = F._case("synthetic", (DEPTH, WIDTH, VOC, 1, B, T), F.LAYERS, thin=0b110, p1_layer=2)
    w = _weights(DEPTH, WIDTH, VOC, 1)
    inp = F.make_inputs(case)
    cfg = O.ModelConfig(DEPTH, WIDTH, VOC, 1)
    st = [inp["states"][:, k] for k in range(2 * DEPTH)]
    _p, st_out, cache = O.forward_window(cfg, dict(w), inp["idx"], inp["ctx"], st, keep_cache=True)
    view = F.synthetic_view(DEPTH, WP, B, T)
    view["thin_mask"] = 0b110
    pad = lambda a: np.pad(np.asarray(a, dtype=np.float32), [(0, 0)] * (a.ndim - 1) + [(0, WP - WIDTH)])
    H = [pad(np.concatenate([inp["states"][None, :, 2 * l], cache["hpre"][l].transpose(1, 0, 2)])) for l in range(DEPTH)]
    C = [pad(np.concatenate([inp["states"][None, :, 2 * l + 1], cache["c"][l].transpose(1, 0, 2)])) for l in range(DEPTH)]
    planes = [F.split_planes(h) for h in H]
    rows = H[1][1:, :, :WIDTH].reshape(T * B, WIDTH)
    P1 = pad(F.p1_emulation(rows, w["K2"], w["b2"]).reshape(T * B, 4, WIDTH))
    arrs = dict(H=H, C=C, Xhi=[p[0] for p in planes], Xlo=[p[1] for p in planes], P1=P1)
    ref = F.references(case, w, inp)
    return dict(case=case, w=w, inp=inp, view=view, arrs=arrs, ref=ref, states_out=np.stack(st_out, axis=1).astype(np.float32))


def _check(window, arrs, view=None):
    view = view or window["view"]
    win = F.decode_forward(F.encode_forward(arrs, view), view)
    return F.check_window(win, view, window["w"], window["inp"], window["states_out"], window["ref"], WIDTH, where="planted")


def _planted(window, **changed):
    arrs = {k: ([a.copy() for a in v] if isinstance(v, list) else v.copy()) for k, v in window["arrs"].items()}
    for k, fn in changed.items():
        fn(arrs[k])
    return arrs


def test_decoders_round_trip_through_a_filled_workspace(window):
    view, arrs = window["view"], window["arrs"]
    ws = F.encode_forward(arrs, view)
    win = F.decode_forward(ws, view)
    for l in range(DEPTH):
        for k in ("H", "C"):
            assert np.array_equal(win[k][l].view(np.uint32), arrs[k][l].view(np.uint32))
        for k in ("Xhi", "Xlo"):
            assert np.array_equal(win[k][l], arrs[k][l])
    assert np.array_equal(win["P1"].view(np.uint32), arrs["P1"].view(np.uint32))
    # every byte outside the arrays is still the fill: nothing was written beside them
    mask = np.ones(ws.size, dtype=bool)
    n = (T + 1) * B * WP
    mask[view["off_P1"]:view["off_P1"] + T * B * 4 * WP * 4] = False
    for l in range(DEPTH):
        for k, size in (("off_H", 4), ("off_C", 4), ("off_Xhi", 2), ("off_Xlo", 2)):
            mask[view[k][l]:view[k][l] + n * size] = False
    assert mask.any() and (ws[mask] == 0xFF).all()
    # a view without planes decodes none
    bare = F.synthetic_view(DEPTH, WP, B, T, planes=False, family=F.WAVEFRONT, c_every_step=1)
    assert F.decode_forward(F.encode_forward(arrs, bare), bare)["Xhi"] is None


def test_view_dict_reads_the_ctypes_struct():
    from ocrd_keraslm_amd.lib import hipabi
    v = hipabi.KlForwardView()
    v.depth, v.width, v.B, v.T, v.family, v.p1_layer, v.off_P1 = 2, 128, 3, 4, F.FUSED, -1, 0
    v.off_H[1], v.off_Xlo[1] = 4096, 8192
    d = F.view_dict(v)
    assert (d["family"], d["p1_layer"], d["off_H"], d["off_Xlo"]) == (F.FUSED, -1, [0, 4096], [0, 8192])
    assert (hipabi.KL_FWD_SPLIT_PAIRS, hipabi.KL_FWD_SPLIT_LAYERS, hipabi.KL_FWD_SPLIT_FUSED, hipabi.KL_FWD_WAVEFRONT) == \
        (F.PAIRS, F.LAYERS, F.FUSED, F.WAVEFRONT)
    assert (hipabi.KL_FWD_HANDOFF_NONE, hipabi.KL_FWD_HANDOFF_SENTINELS, hipabi.KL_FWD_HANDOFF_COUNTERS) == (F.NONE, F.SENTINELS, F.COUNTERS)


def test_the_correct_window_passes(window):
    rep = _check(window, window["arrs"])
    assert rep["h"] < 1e-5 and rep["c"] < 1e-5          # (the f32 oracle against the f64 one)
    assert rep["p1"]["layer"] == 2 and rep["p1"]["ratio"] == 1.0      # (P1 is the emulation itself)


def _wrong_tile(H):
    H[1][2, :, :16] += 3e-4      # a middle layer, a middle step, 16 units; planes recomputed below: only the oracle check sees it


def test_a_wrong_h_tile_in_a_middle_layer_and_step(window):
    arrs = _planted(window, H=_wrong_tile)
    planes = [F.split_planes(h) for h in arrs["H"]]
    arrs["Xhi"], arrs["Xlo"] = [p[0] for p in planes], [p[1] for p in planes]
    with pytest.raises(AssertionError, match=r"'H', 'layer 1', 'step 1'"):
        _check(window, arrs)


def test_hi_and_lo_swapped(window):
    arrs = _planted(window)
    arrs["Xhi"][1], arrs["Xlo"][1] = arrs["Xlo"][1], arrs["Xhi"][1]
    with pytest.raises(AssertionError, match="Xhi is not RNE-bf16"):
        _check(window, arrs)


def test_lo_rounded_toward_zero(window):
    def truncate(lo_planes):
        H = window["arrs"]["H"][2]
        hi = F.bits_f32(F.bf16_bits(H))
        lo_planes[2][...] = ((H - hi).view(np.uint32) >> 16).astype(np.uint16)
    arrs = _planted(window, Xlo=truncate)
    assert (arrs["Xlo"][2] != window["arrs"]["Xlo"][2]).any()
    with pytest.raises(AssertionError, match=r"Xlo is not RNE-bf16\(H - Xhi\)"):
        _check(window, arrs)


def test_a_sentinel_left(window):
    def leave(planes):
        planes[0][T, B - 1, 6:8] = F.SENTINEL      # one armed dword of the last block's last stream
    with pytest.raises(AssertionError, match="arming pattern left in 2 halfwords"):
        _check(window, _planted(window, Xhi=leave))
    with pytest.raises(AssertionError, match="Xlo: arming pattern left"):
        _check(window, _planted(window, Xlo=leave))


def test_a_non_zero_padded_unit(window):
    def plant_f32(a):
        a[1][2, 1, WIDTH + 3] = 1e-30

    def plant_u16(a):
        a[1][2, 1, WP - 1] = 1
    for name, plant, msg in (("H", plant_f32, "H: non-zero padded unit"), ("Xhi", plant_u16, "Xhi: non-zero padded unit"),
                             ("Xlo", plant_u16, "Xlo: non-zero padded unit")):
        with pytest.raises(AssertionError, match=msg):
            _check(window, _planted(window, **{name: plant}))

    def plant_c(a):
        a[1][T, 1, WIDTH] = 1e-30      # (block T: written by every family)
    with pytest.raises(AssertionError, match="C: non-zero padded unit"):
        _check(window, _planted(window, C=plant_c))


def test_p1_without_the_lo_hi_product(window):
    w = window["w"]
    rows = window["arrs"]["H"][1][1:, :, :WIDTH].reshape(T * B, WIDTH)
    for drop in ("lo.hi", "hi.lo"):
        def plant(P1, drop=drop):
            P1[:, :, :WIDTH] = F.p1_emulation(rows, w["K2"], w["b2"], drop=(drop,)).reshape(T * B, 4, WIDTH)
        with pytest.raises(AssertionError, match=r"P1 of layer 2.*ratio [0-9.]+ > 2"):
            _check(window, _planted(window, P1=plant))


def test_a_c_block_t_that_is_not_the_state(window):
    def plant(C):
        C[2][T, 0, 0] = np.nextafter(C[2][T, 0, 0], np.float32(2.0))      # one ulp
    with pytest.raises(AssertionError, match="C block T is not the carried-out state"):
        _check(window, _planted(window, C=plant))
    # ... and a middle block of C is looked at exactly where the view says it was written
    def middle(C):
        C[0][2, 0, 0] += 1.0
    arrs = _planted(window, C=middle)
    _check(window, arrs)
    every = dict(window["view"], c_every_step=1)
    with pytest.raises(AssertionError, match=r"'C', 'layer 0', 'step 1'"):
        _check(window, arrs, view=every)


def test_case_tables_are_consistent():
    names = [c.name for c in F.CASES]
    assert len(set(names)) == len(names) == 16
    for c in F.CASES + F.OLD_SHAPES:
        Wp = F.physical_width(c.width)
        n_rb = (c.B + 15) // 16
        split = c.precision == F.PREC_SPLIT
        assert bool(c.planes) == (c.family != F.WAVEFRONT)
        assert (c.ring | c.thin) == 0 or c.family == F.LAYERS
        if c.family == F.LAYERS:      # fwd_split_layers' own arithmetic: every layer above the first takes one of the two branches
            assert split and Wp == 1024 and n_rb <= 16
            above = (1 << c.depth) - 2
            assert (c.ring if c.B * c.T >= 2048 else c.thin) == above and (c.thin if c.B * c.T >= 2048 else c.ring) == 0
            assert c.p1_layer == c.depth - 1
        if c.family == F.PAIRS:
            assert split and Wp == 1024 and n_rb <= 2 and c.depth <= 4
    rows = {c.name: c.B * c.T for c in F.CASES}
    assert rows["thin-2047-rows"] == 2047 and rows["ring-2048-rows"] == 2048


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_gpu_cases_from_the_oracle_alone(case):
    """|h| < 1 everywhere (the planes are then the split of H itself), and where P1 will hold a product, its emulation has an
    error of its own to hold the kernel to: non-zero and finite.  (The f32 oracle: a bound on |h| needs no more.)"""
    w = _weights(case.depth, case.width, case.voc, case.n_ctx)
    inp = F.make_inputs(case)
    cfg = O.ModelConfig(case.depth, case.width, case.voc, case.n_ctx)
    st = [inp["states"][:, k] for k in range(2 * case.depth)]
    assert all(np.abs(st[2 * l]).max() < 1.0 for l in range(case.depth))
    _p, _st, cache = O.forward_window(cfg, dict(w), inp["idx"], inp["ctx"], st, keep_cache=True)
    for l in range(case.depth):
        assert np.abs(cache["hpre"][l]).max() < 1.0, (case.name, l)
    if case.p1_layer >= 1:
        l = case.p1_layer
        rows = np.ascontiguousarray(cache["hpre"][l - 1].transpose(1, 0, 2)).reshape(case.B * case.T, case.width)
        exact, emu = F.p1_products(rows, w["K%d" % l], w["b%d" % l])
        err = float(np.abs(emu - exact).max())
        assert np.isfinite(err) and 0.0 < err < 1e-3, err
