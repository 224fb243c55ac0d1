"""What the engine does ABOVE the kernels of a training window -- HipLM.train_window / forward_window with _stream_groups,
_padded_streams, _pad_group, _unpad_states: a batch cut into stream groups, the last one padded with dummy streams, every
group run with kl_set_loss_rows, gradients / loss / accuracy composed as size-weighted sums, the regulariser taken once, a
padded group's states carried through a side buffer, its keep-masks extended -- held to f64 references GROUP BY GROUP,
through the test hook HipLM.group_hook.  Cases, inputs and references: tests/train_groups.py.

Every case runs two consecutive windows with pad_streams on (the engine makes the dummy streams) and checks the SECOND: a
replayed graph whose side buffer has been used before.  Per checked group, against the reference of the group's own streams
plus the engine's dummies:
  1. tests/window_ref.py's exact checks over all Bp rows (so the dummy rows' carried-in H and C blocks are exactly zero in
     the second window too), lm.states[b0:b1] = the group's carried-out block bit for bit, no row outside [b0, b1) touched;
  2. every tile of H, C, G, dZ within twice the bf16-storage emulation's largest tile error; floor share <= 5 %;
  3. the weight gradients (tests/window_grads.py, its own bounds) and the tables' exact zeros (tests/table_grads.py) on the
     GROUP's gradients, `_part_grads`;
  4. `_part_loss`: CE within 2 % of the f64 CE of the real streams, the regulariser within 1e-5, no time-out flag, accuracy
     within the share of near ties (<= 5 %, from the oracle alone).
On the batch: lm.grads and loss_acc[0:2] against the f64 sum of the captured parts (4 k u sum |w_i part_i|, exact zeros kept),
loss_acc[2] = group 0's regulariser bit for bit, and -- a belt -- the composed gradients against the f64 oracle of the whole
batch at rel 2e-2 / maxn 4e-2 (tests/gradcheck.py).  A third, traced window names the kernels every group ran on.
test_validation_groups runs the two-group case through forward_window(..., want_probs=False).

Observed on an MI355X (largest ratio error / bound; the bounds are 2.00 for the tiles h, c, gates, dz and 1.00 elsewhere;
"K0" = layer 0's character and context rows, "comp" = the composed gradients and loss_acc[0:2] against the f64 sum of the
parts, "batch" = worst relative L2 error of a composed gradient array against the whole batch's oracle, bound 0.02).  The
emulation's own largest tile error was 0.0071 .. 0.0110 (bound for it 0.1), the floor in force for no tile, near ties
1.8 .. 3.5 % of a group's positions (cap 5 %), the accuracies equal to the oracle's but for 2 positions of regtile-pad's 9000;
7 tests in 14.5 s, the longest (3000 -> 3072 streams x 3 steps: the oracle and its emulation dominate) 4.4 s.

  group                    kernels (forward, backward)   h     c     gates dz    dU    K0           dK1   db    CE    comp        batch
  pad-one 1040 as 1536     wide2, wide2                  1.00  1.00  1.00  1.01  0.02  (0.01 0.04)  0.02  0.00  0.00  -           0.0065
  two-groups 1024          wide2, wide2                  1.00  1.00  1.00  0.94  0.02  (0.01 0.04)  0.01  0.00  0.00  0.29  0.18  0.0063
  two-groups 520 as 1024   wide2, wide2                  1.00  1.00  1.00  1.00  0.02  (0.01 0.05)  0.02  0.00  0.00
  regtile-pad 3000 as 3072 fwd8, regtile                 1.00  1.00  1.00  0.97  0.02  (0.01 0.04)  0.02  0.00  0.00  -           0.0061
  w1024 588 as 640         w32, w32                      1.00  1.00  1.00  0.97  0.03  (0.01 0.04)  0.03  0.00  0.00  0.26  0.13  0.0056
  w128-ragged 64 (three)   w128 multi, w128 multi        1.00  1.00  1.00  1.09  0.03  (0.01 0.03)  0.03  0.00  0.01  0.20  0.08  0.0079
  w128-ragged 8            w128 multi, w128 multi        1.00  1.00  1.00  0.97  0.01  (0.01 0.01)  0.01  0.00  0.01
  validation 1024 / 520    -                             CE within 0.0002 of 7.58 / 7.39 (bound 0.15), accuracies equal, comp 0.13

Hand-made faults, each run once on a scratch copy against this module: the regulariser added per group (fails: "the
regulariser is added once", every multi-group case), weight Bp / B for a padded group (fails: the composition, every padded
case), the side buffer's dummy rows not re-zeroed (fails: "H block 0", every padded case), the keep-masks not extended -- run
in bounds, as the unextended array at the start of a zero buffer of the extended size -- (fails: hundreds of dZ tiles, every
padded case).  (Run with -s for the ROUTE / LOSS / RATIOS / COMPOSITION / KERNELS lines.)
"""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests import gradcheck
from tests import table_grads as TG
from tests import train_groups as G
from tests import window_grads as WG
from tests import window_ref as R

pytestmark = pytest.mark.gpu

CE_REL = 2e-2          # the bf16 training path's loss bar (tests/test_full_size_training.py)
STATES_ABS = 3e-2      # ... and its bar for carried states


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _engine(gc):
    from ocrd_keraslm_amd.lib import hipabi
    from ocrd_keraslm_amd.lib.engine import HipLM
    c = gc.case
    w = G.weights(gc)
    lm = HipLM(c.depth, c.width, c.voc, c.n_ctx)
    assert lm.pad_streams and lm.group_hook is None and lm.pwidth == c.width
    lm.plan_override, lm.max_streams_per_launch = gc.plan_override, gc.max_streams
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    parts = lm._stream_groups(c.B, c.T)
    assert [(b0, b1, lm._padded_streams(b1 - b0, c.T)) for b0, b1 in parts] == [tuple(g) for g in gc.groups]
    return w, lm


class _Capture(object):
    """the group hook: what the engine holds of group i before it is folded into the batch's results"""

    def __init__(self, lm, gc, train):
        self.lm, self.gc, self.train, self.groups = lm, gc, train, []

    def __call__(self, i, b0, b1, Bp):
        lm = self.lm
        lm.torch.cuda.synchronize()
        host = lambda t: t.detach().cpu().numpy().copy()
        rec = dict(i=i, g=G.Group(b0, b1, Bp), loss=host(lm._part_loss), states=host(lm.states),
                   side=host(lm._pad_states[Bp]) if Bp != b1 - b0 else None)
        if self.train:
            rec["grads"] = host(lm._part_grads)
            if i in self.gc.checked:
                rec["win"] = R.read_window_padded(lm)
        self.groups.append(rec)


def _check_states(rec, before, ginp, ref, B, where):
    """-> the carried-out states of all Bp rows of the group; rows outside the group untouched, the side buffer copied back"""
    g = rec["g"]
    n = g.b1 - g.b0
    outside = np.ones(B, dtype=bool)
    outside[g.b0:g.b1] = False
    assert np.array_equal(_bits(rec["states"][outside]), _bits(before[outside])), (where, "a row outside the group changed")
    if rec["side"] is None:
        out = rec["states"][g.b0:g.b1]
    else:
        out = rec["side"]
        assert out.shape[0] == g.Bp
        assert np.array_equal(_bits(rec["states"][g.b0:g.b1]), _bits(out[:n])), (where, "lm.states is not the side buffer's real rows")
    err = float(np.abs(out[:n] - ref["states_out"]).max())
    assert err < STATES_ABS, (where, "carried-out states against the oracle", err)
    return out


def _check_loss(rec, ref, reg, where):
    """-> (CE error / bound, accuracy difference / allowance)"""
    l = rec["loss"]
    assert ref["near_ties"] <= G.NEAR_TIE_MAX, (where, ref["near_ties"])
    ce_bound = CE_REL * max(1.0, ref["ce"])
    print("LOSS | %s | CE %.6f oracle %.6f bound %.4f | accuracy %.6f oracle %.6f near ties %.4f | regulariser %.8g oracle %.8g | flag %g"
          % (where, l[0], ref["ce"], ce_bound, l[1], ref["acc"], ref["near_ties"], l[2], -1.0 if reg is None else reg, l[3]))
    assert abs(l[0] - ref["ce"]) < ce_bound, (where, "CE", l[0], ref["ce"])
    assert abs(l[1] - ref["acc"]) <= ref["near_ties"], (where, "accuracy", l[1], ref["acc"], ref["near_ties"])
    assert l[3] == 0, (where, "time-out flag", l[3])
    if reg is None:
        assert l[2] == 0, (where, "a validation window has no regulariser", l[2])
    else:
        assert abs(l[2] - reg) <= TG.REL * abs(reg), (where, "regulariser", l[2], reg)
    return abs(l[0] - ref["ce"]) / ce_bound, abs(l[1] - ref["acc"]) / max(ref["near_ties"], 1e-300)


def _check_group(gc, w, lm, rec, grp, ref, before, params, reg):
    g, case, ginp, _fw = grp
    c = gc.case
    n = g.b1 - g.b0
    where = case.name
    assert tuple(rec["g"]) == tuple(g), (where, rec["g"])
    st_out = _check_states(rec, before, ginp, ref, c.B, where)
    if rec["i"] not in gc.checked:
        return
    win = rec["win"]
    info, view = win["info"], win["view"]
    assert (info["B"], info["T"], info["first"], info["n"], info["groups"]) == (g.Bp, c.T, g.b0, n, len(gc.groups)), (where, info)
    route = (bool(view["scan2_rows"]), view["wg_route"], view["wg_pair_mask"], view["wg_db_scan_mask"])
    text = TG.route_text(view)
    print("ROUTE | %s | scan2_rows %d | %s" % (where, view["scan2_rows"], text))
    assert route == gc.route[rec["i"]], (where, route, gc.route[rec["i"]], text)
    # 1. no tolerance (ginp's states: the group's carried-in rows, then zeros for the dummy streams)
    R.exact_checks(win, ginp["states"], st_out, n, where=where)
    # 2. the tiles
    share = R.floor_share(ref["ref64"], n, g.Bp)
    assert max(share.values()) <= R.FLOOR_SHARE_MAX, (where, share)
    storage = R.storage_of(view)
    emu = R.references(case, w, ginp, storage, tag=where)
    rep = R.check_tiles(win, ref["ref64"], emu, n, where=where)
    worst = {name: max(v["ratio"] for (a, _l), v in rep.items() if a == name) for name in R.ARRAYS}
    # 3. the group's own gradients
    wrep, werr = WG.check_window_grads(win, ginp["idx"], ginp["ctx"], params, rec["grads"], lm.layout, width=lm.width, where=where, raise_=False)
    trep, terr = TG.check_table_grads(win, ginp["idx"], ginp["ctx"], params, rec["grads"], lm.layout, width=lm.width, dummy_from=n,
                                      where=where, raise_=False, precondition=False)
    # 4. the group's own loss
    ce_ratio, acc_ratio = _check_loss(rec, ref, reg, where)
    print("RATIOS | %s | %d streams as %d | h %.2f | c %.2f | gates %.2f | dz %.2f | emu max %.4f | floor share %.3f | %s | CE %.2f | accuracy %.2f"
          % (where, n, g.Bp, worst["h"], worst["c"], worst["gates"], worst["dz"], max(v["emu_max"] for v in rep.values()),
             max(share.values()), WG.ratio_line(wrep, c.depth), ce_ratio, acc_ratio))
    if werr is not None:
        raise werr
    inexact = [f for f in (terr.failures if terr is not None else []) if "non-zero where exactly zero is due" in f]
    if inexact:
        raise WG.GradMismatch(inexact, where)


@pytest.mark.parametrize("gc", G.CASES, ids=lambda g: g.name)
def test_train_groups(gc):
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    c = gc.case
    w, lm = _engine(gc)
    first = G.batch_inputs(gc, seed=21)
    lm.set_states(first["states"])
    lm.loss_acc.zero_()
    lm.train_window(first["idx"], first["ctx"], first["tgt"], first["masks"])
    lm.read_loss()      # (raises if a hand-off timed out; zeroes the sums)
    before = lm.states.detach().cpu().numpy().copy()
    inp = G.batch_inputs(gc, seed=22, states=before)
    groups, moved = G.settle_batch(gc, w, inp)
    cap = _Capture(lm, gc, train=True)
    lm.group_hook = cap
    try:
        lm.train_window(inp["idx"], inp["ctx"], inp["tgt"], inp["masks"])
    finally:
        lm.group_hook = None
    torch.cuda.synchronize()
    total, grads = lm.loss_acc.detach().cpu().numpy().copy(), lm.grads.detach().cpu().numpy().copy()
    assert [r["i"] for r in cap.groups] == list(range(len(gc.groups)))
    assert np.array_equal(_bits(lm.states.detach().cpu().numpy()), _bits(cap.groups[-1]["states"]))
    # the groups
    cfg = O.ModelConfig(c.depth, c.width, c.voc, c.n_ctx)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    reg = O.regularisers(cfg, w64)
    params = lm.params.detach().cpu().numpy()
    g_batch = None
    for rec, grp in zip(cap.groups, groups):
        ref = G.group_oracle(grp[1], grp[3], grp[2])
        _check_group(gc, w, lm, rec, grp, ref, before, params, reg)
        before = rec["states"]
        share = (grp[0].b1 - grp[0].b0) / c.B
        g_batch = {k: share * v for k, v in ref["g_data"].items()} if g_batch is None else {k: g_batch[k] + share * v for k, v in ref["g_data"].items()}
        rec.pop("win", None)
    # the composition
    sizes = [g.b1 - g.b0 for g in gc.groups]
    comp_g = G.check_composition([r["grads"] for r in cap.groups], sizes, grads, where=(gc.name, "grads"))
    comp_l = G.check_composition([r["loss"][:2] for r in cap.groups], sizes, total[:2], where=(gc.name, "loss_acc[0:2]"))
    assert np.array_equal(_bits(total[2:3]), _bits(cap.groups[0]["loss"][2:3])), (gc.name, "the regulariser is added once", total[2], cap.groups[0]["loss"][2])
    assert total[3] == 0
    table = gradcheck.assert_gradients(lm.layout, lm._unflatten(grads), g_batch, O.regulariser_grads(cfg, w64), rel=2e-2, maxn=4e-2, where=gc.name)
    print("COMPOSITION | %s | %d groups | grads %.3f | loss_acc[0:2] %.3f | targets moved %d of %d | whole batch against the oracle: worst rel L2 %.4f, max-norm %.4f"
          % (gc.name, len(sizes), comp_g, comp_l, moved, c.B * c.T, max(e["rel_l2"] for e in table.values()),
             max(e["max_over_maxnorm"] for e in table.values())))
    # which kernels the groups ran on: a third window, traced (a traced window is not replayed as a graph)
    names = []

    def kernels(i, b0, b1, Bp):
        torch.cuda.synchronize()
        names.append([lm.lib.kl_trace_kernel_name(lm.handle, k).decode() for k in (0, 1)])

    hipabi.check(lm.lib.kl_trace_enable(lm.handle, 1))
    lm.group_hook = kernels
    try:
        lm.train_window(inp["idx"], inp["ctx"], inp["tgt"], inp["masks"])
        torch.cuda.synchronize()
    finally:
        lm.group_hook = None
        hipabi.check(lm.lib.kl_trace_enable(lm.handle, 0))
    lm.read_loss()
    print("KERNELS | %s | %s" % (gc.name, names))
    assert len(names) == len(gc.groups)
    for i in gc.checked:
        assert names[i][0] in c.fwd and names[i][1] in c.bwd, (gc.name, i, names[i], c.fwd, c.bwd)


def test_validation_groups():
    """the two-group case through forward_window(idx, ctx, tgt, want_probs=False): a validation window on the training forward,
    grouped and padded like a training batch.  Second of two windows; per group CE and accuracy against the oracle (no
    dropout), the states' placement, loss_acc[0:2] by the composition rule, no regulariser"""
    import torch
    gc = G.VALIDATION
    c = gc.case
    w, lm = _engine(gc)
    first = G.batch_inputs(gc, seed=21)
    lm.set_states(first["states"])
    lm.loss_acc.zero_()
    assert lm.forward_window(first["idx"], first["ctx"], first["tgt"], want_probs=False) is None
    lm.read_loss()
    before = lm.states.detach().cpu().numpy().copy()
    inp = G.batch_inputs(gc, seed=22, states=before)
    groups, _moved = G.settle_batch(gc, w, inp, dropout=False)
    cap = _Capture(lm, gc, train=False)
    lm.group_hook = cap
    try:
        lm.forward_window(inp["idx"], inp["ctx"], inp["tgt"], want_probs=False)
    finally:
        lm.group_hook = None
    torch.cuda.synchronize()
    total = lm.loss_acc.detach().cpu().numpy().copy()
    assert [tuple(r["g"]) for r in cap.groups] == [tuple(g) for g in gc.groups]
    assert np.array_equal(_bits(lm.states.detach().cpu().numpy()), _bits(cap.groups[-1]["states"]))
    for rec, grp in zip(cap.groups, groups):
        g, case, ginp, fw = grp
        ref = G.group_oracle(case, fw, ginp, backward=False)
        _check_states(rec, before, ginp, ref, c.B, case.name)
        _check_loss(rec, ref, None, case.name + " (validation)")
        before = rec["states"]
    comp = G.check_composition([r["loss"][:2] for r in cap.groups], [g.b1 - g.b0 for g in gc.groups], total[:2], where="validation")
    assert total[2] == 0 and total[3] == 0, total
    print("COMPOSITION | validation | loss_acc[0:2] %.3f" % comp)
