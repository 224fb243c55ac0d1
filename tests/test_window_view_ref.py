"""The tile check of the training window's intermediates (tests/window_ref.py) without a GPU: the oracle's new arguments
leave its default results untouched, the layout decoders round-trip, the checker catches one wrong tile of every kind, and
the inputs of every GPU case (tests/test_window_intermediates_gpu.py) keep the floor out of the way -- decided from the f64
oracle alone."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests import window_ref as R
from tests.gradcheck import cached_weights

SMALL = R._case("small", "none", {}, (2, 128, 40, 40, 5), "", "")


def _weights(case):
    return cached_weights(case.depth, case.width, case.voc, case.n_ctx, 4, 0.3)


def test_no_rounding_requested_is_the_oracle_bit_for_bit():
    """storage=None, keep_dz and an explicit count of B*T change nothing, and the dz handed back is the dz the bias
    gradients were summed from"""
    case = SMALL
    cfg = O.ModelConfig(case.depth, case.width, case.voc, case.n_ctx)
    w = {k: v.astype(np.float64) for k, v in _weights(case).items()}
    inp = R.make_inputs(case)
    st = [inp["states"][:, k].astype(np.float64) for k in range(2 * case.depth)]
    om = [None] + [inp["masks"][l].astype(np.float64) for l in range(1, case.depth)]
    p0, s0, c0 = O.forward_window(cfg, w, inp["idx"], inp["ctx"], st, om, keep_cache=True)
    p1, s1, c1 = O.forward_window(cfg, w, inp["idx"], inp["ctx"], st, om, keep_cache=True, storage=None)
    assert np.array_equal(p0, p1) and all(np.array_equal(a, b) for a, b in zip(s0, s1))
    g0 = O.backward_window(cfg, w, inp["idx"], inp["ctx"], inp["tgt"], p0, c0, om)
    g1, dz = O.backward_window(cfg, w, inp["idx"], inp["ctx"], inp["tgt"], p1, c1, om, keep_dz=True, storage=None,
                               count=case.B * case.T)
    assert set(g0) == set(g1) and all(np.array_equal(g0[k], g1[k]) for k in g0)
    for l in range(case.depth):
        assert dz[l].shape == (case.B, case.T, 4, case.width)
        assert np.array_equal(dz[l].reshape(-1, 4 * case.width).sum(axis=0), g0["b%d" % l])
    # ... and the storage rounding does something: bf16 numbers where the HIP path stores bf16
    p2, _s, c2 = O.forward_window(cfg, w, inp["idx"], inp["ctx"], st, om, keep_cache=True, storage=O.Storage(case.depth))
    for name in ("hpre", "gates"):
        a = c2[name][0]
        assert np.array_equal(a, O.bf16_round(a)) and not np.array_equal(a, c0[name][0])


@pytest.mark.parametrize("interleaved,cb,width,n", [(0, 0, 128, 40), (1, 1, 128, 40), (1, 0, 100, 33), (0, 1, 100, 24)])
def test_layout_decoders_round_trip(interleaved, cb, width, n):
    """canonical arrays -> a workspace as the view describes it -> the same arrays, with gate-interleaved G, bf16 cell
    states, a padded width (100 of 128) and padded streams (n of 40); everything around them is 0xFF bytes"""
    L, Wp, B, T = 2, 128, 40, 3
    rng = np.random.default_rng(3)
    bf = lambda shape: O.bf16_round(rng.standard_normal(shape).astype(np.float32))
    arrs = dict(h=[bf((n, T, width)) for _ in range(L)], gates=[bf((n, T, 4, width)) for _ in range(L)],
                dz=[bf((n, T, 4, width)) for _ in range(L)], h0=[bf((n, width)) for _ in range(L)],
                c0=[rng.standard_normal((n, width)).astype(np.float32) for _ in range(L)],
                cT=[rng.standard_normal((n, width)).astype(np.float32) for _ in range(L)])
    arrs["c"] = [bf((n, T, width)) if cb else rng.standard_normal((n, T, width)).astype(np.float32) for _ in range(L)]
    if not cb:
        for l in range(L):
            arrs["c"][l][:, -1] = arrs["cT"][l]      # (block T is one array)
    arrs["hd"] = [None, bf((n, T, width))]           # (the masked outputs: layer 0 has none)
    view = dict(depth=L, width=Wp, B=B, T=T, g_interleaved=interleaved, c_in_cb=cb, dh_bf16=0, p_bf16_mask=0, scan2_rows=0)
    off, offs = 0, {}
    for key, size in (("off_H", (T + 1) * B * Wp * 2), ("off_C", (T + 1) * B * Wp * 4), ("off_G", T * B * 4 * Wp * 2),
                      ("off_dZ", T * B * 4 * Wp * 2), ("off_Cb", (T + 1) * B * Wp * 2), ("off_Hd", T * B * Wp * 2)):
        offs[key] = []
        for _l in range(L):
            off = (off + 255) // 256 * 256 + 256
            offs[key].append(off)
            off += size
    offs["off_Hd"][0] = 0
    view.update(offs)
    ws = R.encode_window(arrs, view)
    got = R.decode_window(ws, view, width=width, n=n)
    for key in ("h", "c", "gates", "dz", "h0", "c0", "cT"):
        for l in range(L):
            assert np.array_equal(got[key][l], arrs[key][l]), (key, l)
    hd = R.decode_hd(ws, view, width=width, n=n)
    assert hd[0] is None and np.array_equal(hd[1], arrs["hd"][1])
    assert R.decode_hd(ws, {k: v for k, v in view.items() if k != "off_Hd"}) == [None] * L      # (a view from before the field)
    # the bytes really lie as the header says: gate g of unit u of stream b at step t
    import torch
    t, b, g, u, l = 1, n - 1, 2, width - 1, 1
    G = ws[view["off_G"][l]:view["off_G"][l] + T * B * 4 * Wp * 2].view(torch.bfloat16)
    at = (t * B + b) * 4 * Wp + (u * 4 + g if interleaved else g * Wp + u)
    assert float(G[at]) == arrs["gates"][l][b, t, g, u]
    t, b, u, l = 2, n - 1, width - 1, 1      # the masked output of unit u of stream b at step t: row t * B + b, no block 0
    Hd = ws[view["off_Hd"][l]:view["off_Hd"][l] + T * B * Wp * 2].view(torch.bfloat16)
    assert float(Hd[(t * B + b) * Wp + u]) == arrs["hd"][l][b, t, u]
    # rows and columns beyond the trimmed ones are the fill: the finite check sees them when it is given all of them
    full = width == Wp and n == B
    assert got["finite"] == dict(h=full, gates=full, dz=full, cb=full or not cb)


def test_view_struct_and_dict():
    """the fields from before the weight-gradient stage was added keep their offsets (the scalars in front, the five offset
    arrays from byte 64 on), the new ones took four of the reserved words and the end of the struct; the output layer's took
    one more reserved word (out_route) and two words behind off_Hd; `view_dict` carries all"""
    import ctypes as C
    from ocrd_keraslm_amd.lib import hipabi
    V = hipabi.KlWindowView
    scalars = ["depth", "width", "B", "T", "g_interleaved", "c_in_cb", "dh_bf16", "p_bf16_mask", "scan2_rows", "wg_route", "wg_pair_mask",
               "wg_db_scan_mask", "out_route", "reserved"]
    assert [getattr(V, k).offset for k in scalars] == [4 * i for i in range(len(scalars))]
    arrays = ["off_H", "off_C", "off_Cb", "off_G", "off_dZ", "off_Hd"]
    assert [getattr(V, k).offset for k in arrays] == [64 + 128 * i for i in range(6)]
    assert (V.off_dlogits.offset, V.ld_dlogits.offset, C.sizeof(V)) == (64 + 128 * 6, 64 + 128 * 6 + 8, 64 + 128 * 6 + 16)
    assert V.reserved.size == 12 and V.reserved.offset + V.reserved.size == 64
    assert (hipabi.KL_OUT_LOGITS_WS, hipabi.KL_OUT_LOGITS_W128, hipabi.KL_OUT_DH_WS, hipabi.KL_OUT_DE_KMAJOR) == (1, 2, 4, 8)
    assert (hipabi.KL_WG_KMAJOR, hipabi.KL_WG_SCAN_T, hipabi.KL_WG_TRANSPOSE, hipabi.KL_WG_SEGSUM, hipabi.KL_WG_PAIR_CTX) == (1, 2, 4, 8, 16)
    v = V(depth=3, width=128, B=40, T=5, p_bf16_mask=5, wg_route=hipabi.KL_WG_TRANSPOSE | hipabi.KL_WG_SEGSUM, wg_pair_mask=4,
          wg_db_scan_mask=6, out_route=hipabi.KL_OUT_LOGITS_WS | hipabi.KL_OUT_DH_WS | hipabi.KL_OUT_DE_KMAJOR, off_dlogits=123456, ld_dlogits=352)
    for l in range(3):
        v.off_H[l], v.off_Hd[l] = 1000 + l, 7000 * l
    d = R.view_dict(v)
    assert (d["depth"], d["p_bf16_mask"], d["wg_route"], d["wg_pair_mask"], d["wg_db_scan_mask"]) == (3, 5, 12, 4, 6)
    assert d["off_H"] == [1000, 1001, 1002] and d["off_Hd"] == [0, 7000, 14000] and len(d["off_dZ"]) == 3
    from tests import window_grads as WG
    assert (WG.WG_KMAJOR, WG.WG_SCAN_T, WG.WG_TRANSPOSE, WG.WG_SEGSUM, WG.WG_PAIR_CTX) == (1, 2, 4, 8, 16)
    assert WG.route_text(d) == "transposes, pairs 001, db by scan 011, layer 0 segment sums"
    from tests import table_grads as TG
    assert (d["out_route"], d["off_dlogits"], d["ld_dlogits"]) == (13, 123456, 352)
    assert (TG.OUT_LOGITS_WS, TG.OUT_LOGITS_W128, TG.OUT_DH_WS, TG.OUT_DE_KMAJOR) == (1, 2, 4, 8)
    assert TG.route_text(d) == WG.route_text(d) + "; output layer: logits by one kernel (width 512), dH by width-512 kernel, dE k-major"
    assert TG.route_text(dict(d, out_route=2)).endswith("logits by one kernel with dH (width 128), dH by with the logits, dE over dlogits^T")
    assert TG.route_text(dict(d, out_route=0)).endswith("logits by GEMM + softmax, dH by GEMM, dE over dlogits^T")


def test_dlogits_round_trip():
    """[B*T][V] -> bf16 rows of ld_dlogits behind off_dlogits -> the same numbers, zeros in the padded columns, and nothing
    else of the workspace touched; a view from before the fields decodes to None (as off_Hd's does, above)"""
    L, Wp, B, T, V, Vp = 1, 32, 5, 3, 30, 32
    view = dict(depth=L, width=Wp, B=B, T=T, g_interleaved=0, c_in_cb=0, dh_bf16=0, p_bf16_mask=0, scan2_rows=0)
    off = 0
    for key, size in (("off_H", (T + 1) * B * Wp * 2), ("off_C", (T + 1) * B * Wp * 4), ("off_Cb", (T + 1) * B * Wp * 2),
                      ("off_G", T * B * 4 * Wp * 2), ("off_dZ", T * B * 4 * Wp * 2)):
        view[key] = [off]
        off += size
    assert R.decode_dlogits(None, view) is None
    before = R.window_bytes(view)
    view["off_dlogits"], view["ld_dlogits"] = off + 64, Vp
    assert R.window_bytes(view) == off + 64 + B * T * Vp * 2 > before
    import torch
    ws = torch.zeros(R.window_bytes(view), dtype=torch.uint8)
    dl = O.bf16_round(np.random.default_rng(1).standard_normal((B * T, V)).astype(np.float32) * 1e-3)
    R.encode_dlogits(ws, view, dl)
    got = R.decode_dlogits(ws, view)
    assert got.shape == (B * T, Vp) and np.array_equal(got[:, :V], dl) and not got[:, V:].any() and not ws[:off + 64].any()
    t, b, v = 2, 4, 29      # the bytes lie as the header says: row t * B + b, column v of ld_dlogits
    assert float(ws[off + 64:].view(torch.bfloat16)[(t * B + b) * Vp + v]) == dl[t * B + b, v]


@pytest.fixture(scope="module")
def small_refs():
    inp = R.make_inputs(SMALL)
    w = _weights(SMALL)
    return inp, R.references(SMALL, w, inp), R.references(SMALL, w, inp, O.Storage(SMALL.depth))


def _copy(emu):
    return {k: [a.copy() for a in v] for k, v in emu.items()}


def test_checker_passes_the_emulation(small_refs):
    inp, r64, emu = small_refs
    rep = R.check_tiles(emu, r64, emu, inp["n_real"])
    assert all(abs(v["ratio"] - 1.0) < 1e-12 for v in rep.values())


@pytest.mark.parametrize("name", R.ARRAYS)
@pytest.mark.parametrize("kind", ["next step", "swapped blocks", "sentinels"])
def test_checker_catches_one_wrong_tile(small_refs, name, kind):
    """synthetic kernel output = the emulation with ONE tile (two for the swap) of one array wrong"""
    inp, r64, emu = small_refs
    got = _copy(emu)
    l, t = 1, 2
    a = got[name][l]
    if kind == "next step":
        a[0:16, t] = a[0:16, t + 1]
    elif kind == "swapped blocks":
        a[0:16, t], a[16:32, t] = a[16:32, t].copy(), a[0:16, t].copy()
    else:
        a[0:16, t] = np.frombuffer(np.full(1, 0xFFFF0000, dtype=np.uint32).tobytes(), dtype=np.float32)[0]      # bf16 0xFFFF
    with pytest.raises(AssertionError) as err:
        R.check_tiles(got, r64, emu, inp["n_real"])
    text = str(err.value)
    assert "'%s', 'layer %d', 'step %d', 'block 0'" % (name, l, t) in text
    assert ("2 tiles" if kind == "swapped blocks" else "1 tiles") in text


def test_checker_catches_a_dropped_cell_gradient(small_refs):
    inp, r64, emu = small_refs
    got = _copy(emu)
    l, t, blk = 0, 1, 0
    got["dz"][l][blk * 16:(blk + 1) * 16, t] = R.zero_dc_tile(emu, l, t, blk)
    with pytest.raises(AssertionError) as err:
        R.check_tiles(got, r64, emu, inp["n_real"])
    assert "'dz', 'layer %d', 'step %d', 'block %d'" % (l, t, blk) in str(err.value) and "1 tiles" in str(err.value)


def test_exact_checks_catch_a_sentinel_and_a_dummy_stream_gradient(small_refs):
    import torch
    inp, _r64, emu = small_refs
    case = SMALL
    L, W, B, T = case.depth, case.width, case.B, case.T
    st_in = inp["states"]
    st_out = np.stack([a for l in range(L) for a in (emu["h"][l][:, -1], emu["c"][l][:, -1])], axis=1)
    arrs = dict(emu, h0=[O.bf16_round(st_in[:, 2 * l]) for l in range(L)], c0=[st_in[:, 2 * l + 1] for l in range(L)],
                cT=[emu["c"][l][:, -1] for l in range(L)])
    view = dict(depth=L, width=W, B=B, T=T, g_interleaved=0, c_in_cb=0, dh_bf16=0, p_bf16_mask=0, scan2_rows=0)
    off = 0
    for key, size in (("off_H", (T + 1) * B * W * 2), ("off_C", (T + 1) * B * W * 4), ("off_Cb", (T + 1) * B * W * 2),
                      ("off_G", T * B * 4 * W * 2), ("off_dZ", T * B * 4 * W * 2)):
        view[key] = [off + l * size for l in range(L)]
        off += L * size
    ws = R.encode_window(arrs, view)
    R.exact_checks(R.decode_window(ws, view), st_in, st_out, inp["n_real"])
    bad = ws.clone()
    bad[view["off_dZ"][1] + 2 * (1 * B + 3) * 4 * W:][:32] = 0xFF      # 16 halfwords of step 1, stream 3
    with pytest.raises(AssertionError, match="NaN"):
        R.exact_checks(R.decode_window(bad, view), st_in, st_out, inp["n_real"])
    bad = ws.clone()
    bad[view["off_dZ"][0] + 2 * (2 * B + B - 1) * 4 * W + 1] = 0x3C      # one halfword of the last (dummy) stream
    with pytest.raises(AssertionError, match="dummy"):
        R.exact_checks(R.decode_window(bad, view), st_in, st_out, inp["n_real"])
    bad = ws.clone()
    bad[view["off_C"][0] + 5] ^= 1      # one bit of the carried-in cell state
    with pytest.raises(AssertionError, match="C block 0"):
        R.exact_checks(R.decode_window(bad, view), st_in, st_out, inp["n_real"])


def _input_sets():
    seen, out = set(), []
    for case in R.CASES + [R.REPLAY_A, R.REPLAY_B, R.CONSECUTIVE]:
        key = (case[3:9], case.last_only)
        if key not in seen:
            seen.add(key)
            out.append(case)
    return out


@pytest.mark.parametrize("case", _input_sets(), ids=lambda c: c.name)
def test_floor_share_of_the_gpu_cases(case):
    """at most 5 % of the non-dummy tiles of any array and layer may be measured against the floor instead of their own norm
    (none is, at the chosen inputs), and every case has an all-dummy block and a half-dummy one where it has the rows"""
    inp = R.make_inputs(case)
    n_real, B = inp["n_real"], case.B
    assert (inp["tgt"][n_real:] == -2).all() and (inp["tgt"][:n_real] >= -1).all()
    if B > 16:
        assert n_real % 16 == 8 and len(R.dummy_blocks(B, n_real)) == 1
    share = R.floor_share(R.references(case, _weights(case), inp), n_real, B)
    print(case.name, "largest floor share %.4f" % max(share.values()))
    assert max(share.values()) <= R.FLOOR_SHARE_MAX, share


def _group_cases():
    from tests import train_groups
    return train_groups.CASES


@pytest.mark.parametrize("gc", _group_cases(), ids=lambda g: g.name)
def test_floor_and_near_tie_share_of_the_group_cases(gc):
    """the inputs of tests/test_train_groups_gpu.py, from the oracle alone: the plan cuts and pads each batch as the case says;
    in the SECOND window (carried states: here the f64 oracle's) of every checked group at most 5 % of the non-dummy tiles are
    measured against the floor, and at most 5 % of the real positions have their two largest probabilities within 1e-2 of
    each other (the allowance of the accuracy check); at most 15 % of the targets had to be moved away from the loss clip"""
    from ocrd_keraslm_amd.lib.engine import HipLM, physical_width
    from tests import train_groups as G
    c = gc.case
    lm = HipLM.__new__(HipLM)
    lm.pwidth, lm.pad_streams, lm.plan_override, lm.max_streams_per_launch = physical_width(c.width), True, gc.plan_override, gc.max_streams
    parts = lm._stream_groups(c.B, c.T)
    assert [(b0, b1, lm._padded_streams(b1 - b0, c.T)) for b0, b1 in parts] == [tuple(g) for g in gc.groups]
    w = G.weights(gc)
    first = G.batch_inputs(gc, seed=21)
    inp = G.batch_inputs(gc, seed=22, states=G.carried_states(gc, w, first))
    groups, replaced = G.settle_batch(gc, w, inp)
    assert replaced <= 0.15 * c.B * c.T, replaced
    for i in gc.checked:
        g, case, ginp, fw = groups[i]
        n = g.b1 - g.b0
        assert (ginp["tgt"][n:] == -2).all() and not ginp["states"][n:].any() and np.array_equal(ginp["tgt"][:n], inp["tgt"][g.b0:g.b1])
        ref = G.group_oracle(case, fw, ginp)
        share = R.floor_share(ref["ref64"], n, g.Bp)
        print(gc.name, tuple(g), "largest floor share %.4f, near ties %.4f, CE %.3f, accuracy %.4f, targets moved in the batch %d"
              % (max(share.values()), ref["near_ties"], ref["ce"], ref["acc"], replaced))
        assert max(share.values()) <= R.FLOOR_SHARE_MAX, share
        assert ref["near_ties"] <= G.NEAR_TIE_MAX, ref["near_ties"]
