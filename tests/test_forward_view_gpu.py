"""Every scan family of the INFERENCE-layout window (split-precision kl_forward_window, kl_rate_window: the rating, rate_best
and correction paths) held to the oracle per layer and step on what it leaves in the workspace -- H, C, the (hi, lo) planes
and the gate inputs P1 --, found through kl_test_forward_view (HipLM.forward_view) and decoded and checked by
tests/forward_view.py, where the checks and their bounds are explained.

Each case first asserts what the view says about the route -- the family that finished the window, the families that launched
and handed it on, the layers whose gate inputs came from the ring products / the thin GEMM, the hand-off --, so a case that no
longer reaches its branch fails instead of passing on another one; then all checks run over two consecutive windows carrying
state (the second a replayed graph).  The stream counts assume 256 compute units (asserted).

Observed on an MI355X (256 CUs), the larger of the two windows: largest |H - oracle| and |C - oracle| over every (layer, step)
(bound 1e-4 in split precision, 3e-2 in bf16), largest probability error (bound 2e-5; bf16 1e-2), and the ratio of the kernel's
largest P1 error to the emulation's (bound 2.00; the emulation's own largest error was 0.9e-6 .. 2.6e-6).  16 cases + view
errors + rate-window view + the five old shapes = 23 tests in 19 s, the longest case 2.3 s (weights and the f64 oracle dominate).

  case                               family (passed)        gate inputs of layers >= 1   H        C        probs    P1 ratio
  pairs                              SPLIT_PAIRS            in the scan                  3.0e-06  5.7e-06  6.0e-06  -
  pair-and-single                    SPLIT_PAIRS            in the scan                  3.0e-06  5.5e-06  7.6e-06  -
  pairs-hand-on                      SPLIT_LAYERS (PAIRS)   thin GEMM, layers 1..4       3.2e-06  5.2e-06  5.3e-06  1.000
  split8-off                         SPLIT_LAYERS           thin GEMM                    3.0e-06  5.7e-06  6.2e-06  1.000
  thin-2047-rows                     SPLIT_LAYERS           thin GEMM                    4.0e-06  6.2e-06  6.6e-06  1.010
  ring-2048-rows                     SPLIT_LAYERS           ring products                3.8e-06  6.5e-06  7.5e-06  1.000
  ring-ragged-two-contexts           SPLIT_LAYERS           ring products                4.0e-06  6.1e-06  6.6e-06  1.000
  ring-16-row-blocks-p1-reused       SPLIT_LAYERS           ring products, layers 1, 2   3.5e-06  6.4e-06  9.4e-06  1.004
  ring-partial-row-block-no-context  SPLIT_LAYERS           ring products                4.9e-06  8.4e-06  9.8e-06  1.004
  beyond-16-row-blocks               WAVEFRONT (FUSED)      per step                     2.9e-06  5.3e-06  1.2e-05  -
  fused-sentinels                    SPLIT_FUSED            in the scan                  3.0e-06  5.3e-06  4.6e-06  -
  fused-counters                     SPLIT_FUSED            in the scan                  3.0e-06  5.2e-06  4.9e-06  -
  padded-width                       SPLIT_FUSED            in the scan                  1.9e-06  2.9e-06  9.3e-07  -
  deeper-than-maxl                   WAVEFRONT              per step                     2.9e-06  4.3e-06  1.2e-06  -
  scan-off                           WAVEFRONT              per step                     2.5e-06  4.4e-06  1.2e-06  -
  bf16-inference-workspace           WAVEFRONT              per step                     1.4e-03  2.5e-03  8.7e-04  -

The old width-1024 shapes (F.OLD_SHAPES): 4 x 1024 at 2 streams, 3 x 1024 at 20, 2 x 1024 at 5 -- SPLIT_PAIRS; 1 x 1024 at 65 --
SPLIT_LAYERS with no layer above the first; 2 x 1024 at 40 x 4 -- SPLIT_LAYERS, thin GEMM.  None had reached the ring products or
the hand-on after launched pairs.  When this module first ran, fused-counters failed the plane check (Xlo differed from
RNE-bf16(H - Xhi) in 1501 of 102400 halfwords of layer 0): lstm_scan_fwd_split_kernel's subtraction had been contracted with the
product that makes h; fixed in the kernel.  Run with -s for the per-window lines.
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import forward_view as F

pytestmark = pytest.mark.gpu

PROBS_BOUND = {F.PREC_SPLIT: F.PROBS_BOUND, F.PREC_BF16: 1e-2}      # (bf16: the bound of test_validation_windows_bf16)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _engine(case, monkeypatch):
    from ocrd_keraslm_amd.lib.engine import HipLM
    from tests.gradcheck import cached_weights
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)      # (read when the engine is created)
    w = cached_weights(case.depth, case.width, case.voc, case.n_ctx, 4, 0.5)
    lm = HipLM(case.depth, case.width, case.voc, case.n_ctx)
    cus = lm.torch.cuda.get_device_properties(lm.device).multi_processor_count
    assert cus >= 256, "the cases were chosen for 256 compute units (the scans' grid plan clamps there); %d here" % cus
    assert lm.pwidth == F.physical_width(case.width)
    lm.set_weights(w, case.precision)
    return w, lm


class Runner(object):
    """windows of one case on one engine, carrying state: through HipLM.forward_window, or (case.abi) through kl_forward_window
    on an inference-size workspace of the test's own"""

    def __init__(self, lm, case, inp):
        self.lm, self.case = lm, case
        torch = lm.torch
        if case.abi:
            self.states = torch.zeros((case.B, 2 * case.depth, lm.pwidth), dtype=torch.float32, device=lm.device)
            self.states[:, :, :lm.width] = torch.from_numpy(inp["states"]).to(lm.device)
            n = lm.lib.kl_window_workspace_bytes(lm.handle, case.B, case.T, 0)
            self.ws = torch.empty(n, dtype=torch.uint8, device=lm.device)
            self.probs = torch.empty((case.B, case.T, case.voc), dtype=torch.float32, device=lm.device)
        else:
            assert lm._rating_groups(case.B) == [(0, case.B)]
            lm.set_states(inp["states"])

    def window(self, inp):
        """-> (probabilities [B][T][V], carried-out states [B][2L][width], view dict, workspace)"""
        lm, case = self.lm, self.case
        lm.loss_acc.zero_()
        if case.abi:
            from ocrd_keraslm_amd.lib import hipabi
            with lm._launch():
                x = lm._dev_i32(inp["idx"])
                z = lm._dev_i32(inp["ctx"]) if lm.n_ctx else None
                hipabi.check(lm.lib.kl_forward_window(lm.handle, case.B, case.T, _ptr(x), _ptr(z), None, _ptr(self.states), _ptr(self.probs),
                                                      _ptr(lm.loss_acc), _ptr(self.ws), self.ws.numel(), lm._stream()), "kl_forward_window")
            lm.torch.cuda.synchronize()
            assert float(lm.loss_acc[3].item()) == 0.0, "a scan hand-off timed out"
            probs, states = self.probs.cpu().numpy(), self.states[:, :, :lm.width].cpu().numpy()
            view, ws = lm.forward_view(case.B, case.T, self.ws)
        else:
            probs = lm.forward_window(inp["idx"], inp["ctx"], inp["tgt"]).cpu().numpy()      # (raises if a hand-off timed out)
            states = lm.get_states()
            view, ws = lm.forward_view()
        return probs, states, F.view_dict(view), ws


def _assert_route(case, vd, lm):
    got = dict(family=F.FAMILY_NAMES.get(vd["family"], vd["family"]), passed=vd["passed_mask"], ring=vd["ring_mask"], thin=vd["thin_mask"],
               handoff=vd["handoff"], planes=F.has_planes(vd), p1_layer=vd["p1_layer"], c_every_step=vd["c_every_step"])
    want = dict(family=F.FAMILY_NAMES[case.family], passed=case.passed, ring=case.ring, thin=case.thin, handoff=case.handoff,
                planes=bool(case.planes), p1_layer=case.p1_layer, c_every_step=1 if case.family == F.WAVEFRONT else 0)
    assert got == want, (case.name, "the window did not take the route the case exists for", got, want)
    assert (vd["depth"], vd["width"], vd["B"], vd["T"], vd["precision"]) == (case.depth, lm.pwidth, case.B, case.T, case.precision)


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_forward_view(monkeypatch, case):
    t0 = time.time()
    w, lm = _engine(case, monkeypatch)
    inp = F.make_inputs(case, seed=31)
    run = Runner(lm, case, inp)
    worst = dict(h=0.0, c=0.0, probs=0.0, ratio=None, emu=None)
    for win_no in range(2):
        probs, states_out, vd, ws = run.window(inp)
        _assert_route(case, vd, lm)
        ref = F.references(case, w, inp, tag=None if win_no == 0 else case.name + "-2")
        where = "%s, window %d" % (case.name, win_no)
        rep = F.check_window(F.decode_forward(ws, vd), vd, w, inp, states_out, ref, case.width, where=where)
        e_probs = float(np.abs(probs - ref["probs"]).max())
        worst.update(h=max(worst["h"], rep["h"]), c=max(worst["c"], rep["c"]), probs=max(worst["probs"], e_probs))
        if rep["p1"]:
            worst["ratio"], worst["emu"] = max(worst["ratio"] or 0.0, rep["p1"]["ratio"]), rep["p1"]["emu_max"]
        print("FORWARD_VIEW | %s | window %d | %s passed %d ring %s thin %s handoff %d p1_layer %d | H %.3g | C %.3g | probs %.3g | P1 %s"
              % (case.name, win_no, F.FAMILY_NAMES[vd["family"]], vd["passed_mask"], bin(vd["ring_mask"]), bin(vd["thin_mask"]), vd["handoff"],
                 vd["p1_layer"], rep["h"], rep["c"], e_probs,
                 "layer %(layer)d ratio %(ratio).3f emu %(emu_max).3g worst %(worst).3g" % rep["p1"] if rep["p1"] else "-"))
        assert e_probs <= PROBS_BOUND[case.precision], (where, "probabilities", e_probs)
        inp = F.make_inputs(case, seed=32, states=states_out)
    print("FORWARD_VIEW_CASE | %s | %.1f s | H %.3g | C %.3g | probs %.3g | ratio %s"
          % (case.name, time.time() - t0, worst["h"], worst["c"], worst["probs"], "%.3f" % worst["ratio"] if worst["ratio"] else "-"))


def test_view_needs_a_window_of_that_shape(monkeypatch):
    from ocrd_keraslm_amd.lib import hipabi
    case = next(c for c in F.CASES if c.name == "padded-width")
    _w, lm = _engine(case, monkeypatch)
    with pytest.raises(hipabi.KlError):
        lm.forward_view()
    ws = lm._workspace(case.B, case.T, False)
    view = hipabi.KlForwardView()
    ask = lambda B, T: lm.lib.kl_test_forward_view(lm.handle, B, T, _ptr(ws), C.byref(view))
    assert ask(case.B, case.T) == 3      # KL_ERR_STATE: nothing has run
    inp = F.make_inputs(case)
    lm.set_states(inp["states"])
    lm.forward_window(inp["idx"], inp["ctx"])
    assert lm._workspace(case.B, case.T, False).data_ptr() == ws.data_ptr()
    assert ask(case.B, case.T) == 0 and view.family == F.FUSED
    assert ask(case.B, case.T + 1) == 3 and ask(case.B + 1, case.T) == 3      # another shape on the same workspace
    other = lm.torch.empty(ws.numel(), dtype=lm.torch.uint8, device=lm.device)
    assert lm.lib.kl_test_forward_view(lm.handle, case.B, case.T, _ptr(other), C.byref(view)) == 3      # another workspace
    lm.prepare(hipabi.KL_PREC_BF16)
    assert ask(case.B, case.T) == 3      # another precision: its window has not run


def test_rate_window_view_is_forward_window_view(monkeypatch):
    """kl_rate_window carves the same window at the start of its workspace: the same route, the same offsets and -- from the same
    state and inputs -- the same bits in H, the planes and P1 (the ring case)"""
    case = F.RING_CASE
    _w, lm = _engine(case, monkeypatch)
    inp = F.make_inputs(case)
    lm.set_states(inp["states"])
    lm.forward_window(inp["idx"], inp["ctx"])
    v_fwd, ws_fwd = lm.forward_view()
    vd_fwd = F.view_dict(v_fwd)
    _assert_route(case, vd_fwd, lm)
    a = F.decode_forward(ws_fwd, vd_fwd)
    st_fwd = lm.get_states()
    lm.set_states(inp["states"])
    lm.rate_window(inp["idx"], inp["ctx"], inp["tgt"])
    lm.rate_status_check()
    v_rate, ws_rate = lm.forward_view()
    assert ws_rate.data_ptr() != ws_fwd.data_ptr()
    vd_rate = F.view_dict(v_rate)
    assert vd_rate == vd_fwd
    b = F.decode_forward(ws_rate, vd_rate)
    assert np.array_equal(lm.get_states().view(np.uint32), st_fwd.view(np.uint32))
    for l in range(case.depth):
        assert np.array_equal(a["H"][l].view(np.uint32), b["H"][l].view(np.uint32)), ("H", l)
        assert np.array_equal(a["C"][l][[0, case.T]].view(np.uint32), b["C"][l][[0, case.T]].view(np.uint32)), ("C", l)
        assert np.array_equal(a["Xhi"][l], b["Xhi"][l]) and np.array_equal(a["Xlo"][l], b["Xlo"][l]), ("planes", l)
    assert np.array_equal(a["P1"].view(np.uint32), b["P1"].view(np.uint32))


@pytest.mark.parametrize("case", F.OLD_SHAPES, ids=lambda c: c.name)
def test_old_width_1024_shapes_stay_below_the_ring_branch(monkeypatch, case):
    """the width-1024 split-precision shapes of test_forward_window_parity and test_rate_window_is_forward_window_picked: the
    route each takes (pairs, one layer, or the thin GEMM) -- none of them the ring products"""
    _w, lm = _engine(case, monkeypatch)
    inp = F.make_inputs(case)
    lm.set_states(inp["states"])
    lm.forward_window(inp["idx"], inp["ctx"])
    vd = F.view_dict(lm.forward_view()[0])
    print("FORWARD_VIEW_OLD | %s | %s passed %d ring %s thin %s" % (case.name, F.FAMILY_NAMES[vd["family"]], vd["passed_mask"],
                                                                     bin(vd["ring_mask"]), bin(vd["thin_mask"])))
    _assert_route(case, vd, lm)
    assert vd["ring_mask"] == 0
