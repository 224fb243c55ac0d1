"""Every recurrence scan of the training window held to the oracle per TILE (one layer x one step x 16 streams) on what it
leaves in the workspace -- the outputs H, the cell states C / Cb, the gate activations G and the gate gradients dZ of every
step and layer --, found through kl_test_window_view (HipLM.window_view) and decoded by tests/window_ref.py, where the
bounds are explained: twice the largest tile error of the bf16-storage oracle, no number fixed in advance, plus the checks
without tolerance (no sentinel left, dummy streams' dZ exactly zero, blocks 0 and T = the carried-in / carried-out state).

Each case forces one kernel family with the switches of tests/test_gpu_kernels.py and asserts both kernel names; each runs
with dropout masks, a padded tail, an all-dummy 16-row block and a half-dummy one (kl_set_loss_rows), one case in the stateless
window mode.  Stream groups and the engine's own dummy streams: tests/test_train_groups_gpu.py, group by group.

Observed on an MI355X (largest ratio kernel tile error / the emulation's largest tile error over the family's cases and
layers; the bound is 2.00).  The emulation's own largest tile error was 0.0046 .. 0.0070 (bound for it: 0.1), the floor was
in force for no tile of any case (share 0.000, cap 0.05); 24 cases + view / replay / consecutive windows = 27 tests in 45 s,
the longest case (3072 streams x 5 steps, the oracle and its emulation dominate) 5.7 s.

  family                                    h     c     gates  dz
  thin fused scans                          1.00  1.00  1.00   1.01
  launch per step                           1.00  1.00  1.00   1.01
  padded width (100 -> 128)                 1.00  1.00  1.00   1.02
  wide, first generation (+ consecutive)    1.00  1.00  1.00   1.01
  second generation (+ replay)              1.00  1.00  1.00   1.00
  second generation, prefetch variant       1.00  1.00  1.00   0.99
  second generation, f32 exchange           1.00  1.00  1.00   1.00
  second generation, register-tile backward 1.00  1.00  1.00   1.01
  eight-wave forward                        1.00  1.00  1.00   1.00
  eight-wave forward, counter form          1.00  1.00  1.00   1.00
  eight-wave forward, table mode            1.00  1.00  1.00   1.00
  width 1024                                1.00  1.00  1.00   0.99
  width 128, multi (+ stateless mode)       1.06  1.00  1.00   1.01
  width 128, single                         1.00  1.00  1.00   1.01
  width 128, unfused                        1.00  1.00  1.00   1.01

(The kernels land on the emulation's own errors: they round where it rounds.  Run with -s for the per-case lines.)
"""
import pytest

from tests import window_ref as R

pytestmark = pytest.mark.gpu


def _engine(case, monkeypatch):
    from ocrd_keraslm_amd.lib import hipabi
    from ocrd_keraslm_amd.lib.engine import HipLM
    from tests.gradcheck import cached_weights
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)      # (read when the engine is created)
    w = cached_weights(case.depth, case.width, case.voc, case.n_ctx, 4, 0.3)
    lm = HipLM(case.depth, case.width, case.voc, case.n_ctx)
    lm.pad_streams = False            # (the cases bring their own dummy streams)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    if case.last_only:
        lm.set_window_mode(True)
    return w, lm


def _train(lm, inp, names=None):
    """one window with the means over the real streams; names: (forward, backward) kernels that must have run"""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lm.loss_acc.zero_()
    if names:
        hipabi.check(lm.lib.kl_trace_enable(lm.handle, 1))
    hipabi.check(lm.lib.kl_set_loss_rows(lm.handle, inp["n_real"]))
    try:
        lm.train_window(inp["idx"], inp["ctx"], inp["tgt"], inp["masks"])
    finally:
        hipabi.check(lm.lib.kl_set_loss_rows(lm.handle, 0))
    torch.cuda.synchronize()
    if names:
        got = [lm.lib.kl_trace_kernel_name(lm.handle, k).decode() for k in (0, 1)]
        hipabi.check(lm.lib.kl_trace_enable(lm.handle, 0))
        assert got[0] in names[0] and got[1] in names[1], (got, names)
    lm.read_loss()      # (raises if a hand-off timed out)


def _check(case, w, lm, inp, tag=None):
    win = R.read_window(lm)
    info = win["info"]
    assert (info["B"], info["T"], info["n"], info["groups"]) == (case.B, case.T, case.B, 1), info
    R.exact_checks(win, inp["states"], lm.get_states(), inp["n_real"], where=case.name)
    storage = R.storage_of(win["view"])
    ref64 = R.references(case, w, inp, tag=tag)
    share = R.floor_share(ref64, inp["n_real"], case.B)
    assert max(share.values()) <= R.FLOOR_SHARE_MAX, share
    emu = R.references(case, w, inp, storage, tag=tag)
    rep = R.check_tiles(win, ref64, emu, inp["n_real"], where=case.name)
    worst = {name: max(v["ratio"] for (a, _l), v in rep.items() if a == name) for name in R.ARRAYS}
    print("RATIOS | %s | %s | %s | p_bf16 %s dh_bf16 %d cb %d | h %.2f | c %.2f | gates %.2f | dz %.2f | emu max %.4f | floor share %.3f"
          % (case.name, case.family, " ".join("%s=%s" % kv for kv in case.env.items()) or "defaults", storage.p_bf16,
             storage.dh_bf16, storage.c_bf16, worst["h"], worst["c"], worst["gates"], worst["dz"],
             max(v["emu_max"] for v in rep.values()), max(share.values())))
    return rep


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_window_intermediates(monkeypatch, case):
    w, lm = _engine(case, monkeypatch)
    inp = R.make_inputs(case)
    lm.set_states(inp["states"])
    _train(lm, inp, names=(case.fwd, case.bwd))
    _check(case, w, lm, inp)


def test_view_needs_a_training_window(monkeypatch):
    import ctypes as C
    from ocrd_keraslm_amd.lib import hipabi
    case = R.CASES[0]
    _w, lm = _engine(case, monkeypatch)
    with pytest.raises(hipabi.KlError):
        lm.window_view()
    ws = lm._workspace(case.B, case.T, True)
    view = hipabi.KlWindowView()
    assert lm.lib.kl_test_window_view(lm.handle, case.B, case.T, C.c_void_p(ws.data_ptr()), C.byref(view)) == 3      # KL_ERR_STATE


def test_window_intermediates_after_replay(monkeypatch):
    """shape A, shape B, then A again on one engine, one workspace and the same state buffers: A's second window is a replayed
    graph (nothing is traced here, so windows are captured) behind a window of another shape -- sentinels re-armed, the
    flag epoch moved on, and the view must still describe A"""
    A, Bc = R.REPLAY_A, R.REPLAY_B
    w, lm = _engine(A, monkeypatch)
    big = max(lm.lib.kl_window_workspace_bytes(lm.handle, c.B, c.T, 1) for c in (A, Bc))
    ws = lm.torch.empty(big, dtype=lm.torch.uint8, device=lm.device)
    lm._workspace = lambda B, T, training: ws
    lm._ws = ws
    states = {}
    for case, seed in ((A, 21), (Bc, 21), (A, 22)):
        inp = R.make_inputs(case, seed=seed)
        if case.B in states:
            lm.states = states[case.B]      # (the same buffer: its address is part of the captured graph's key)
        lm.set_states(inp["states"])
        states[case.B] = lm.states
        _train(lm, inp)
    _check(A, w, lm, inp, tag="replay-A-2")


def test_window_intermediates_consecutive_windows(monkeypatch):
    """two windows on carried state; the second one (a replayed graph, starting from what the first left) is checked"""
    case = R.CONSECUTIVE
    w, lm = _engine(case, monkeypatch)
    inp = R.make_inputs(case, seed=21)
    lm.set_states(inp["states"])
    _train(lm, inp)
    carried = lm.get_states()
    inp = R.make_inputs(case, seed=22, states=carried)
    _train(lm, inp)
    _check(case, w, lm, inp, tag="consecutive-2")
