"""The weight-gradient stage of kl_train_window -- dU, dK, db of every layer, layer 0's table route included -- held to the
f64 products of what the scans left in the workspace (tests/window_grads.py: 1e-5 of the array's largest entry for every
product, the rounding model's bound for a bias gradient that a backward scan summed, exact zeros in the padding), one case
per ROUTE of the stage, each at the smallest shape that takes the route, each asserting the route through the view's
wg_route / wg_pair_mask / wg_db_scan_mask.  Inputs as in tests/test_window_intermediates_gpu.py: dropout masks, a padded
tail, an all-dummy 16-row block and a half-dummy one.  Every product is checked in full (the f64 references take 0.1 - 0.9 s
per case).  The gemm-level switches (KL_GEMM_WIDE, KL_GEMM_LONG, ...) are read once per process and not toggled here:
tests/test_gemm_wide_gpu.py covers them.  Stream groups (every group's own gradients): tests/test_train_groups_gpu.py.

Layer 0's character rows (E_bf16^T . bf16(S)) are asserted by a test of their own, test_window_grads_characters, from the
same run: their allowance for sums near a bf16 rounding boundary is half of what a sum that really rounds the other way
needs (see the note in tests/window_grads.py), and a failure there must not hide the other products.

Observed on an MI355X (largest ratio error / bound per kind of array over the case's layers; the bound is 1.00; "K0 chars" and
"K0 ctx" are layer 0's character and context rows, "near" the character sums within 1e-5 of a bf16 rounding boundary out of all
non-zero ones -- sums of a few dozen bf16 numbers are short binary fractions and often lie exactly ON a boundary, where the
engine's f32 sum is exact too and rounds as the reference does).  30 tests in 6.2 s, the longest 1.0 s.

  case                 route                                      dU    K0 chars  K0 ctx  dK>=1  db    near
  kmajor-pairs         k-major, pair, segment sums                0.03  0.01      0.04    0.02   0.00  918 / 131071
  kmajor-single        k-major, single launches, segment sums     0.02  0.01      0.04    0.01   0.00  918 / 131071
  bt864-wide1          scan-transposed, segment sums              0.06  0.01      0.03    0.04   0.00  5342 / 131068
  bt864-gemm-an-off    scan-transposed, segment sums              0.06  0.01      0.03    0.04   0.00  5342 / 131068
  thin-256             transposes (45 -> 48 rows), column sums    0.01  0.00      0.01    0.01   0.00  554 / 22527
  thin-128             transposes, depth 3, two context tables    0.02  0.00      0.01    0.02   0.00  1048 / 12797
  w128-multi-ragged    transposes (165 -> 168 rows), depth 4      0.03  0.00      0.01    0.02   0.00  1141 / 14847
  padded-width         transposes, width 100 -> 128               0.01  0.00      0.01    0.01   0.00  1514 / 14397
  w1024-ragged         transposes, width 1024                     0.02  0.00      0.02    0.02   0.00  16595 / 151523
  onehot-v64           k-major, pair, one-hot                     0.03  0.01      0.04    0.01   0.00  918 / 131071
  onehot-v128-paired   k-major, pair, one-hot with context pair   0.03  0.01      0.03    0.02   0.00  3240 / 262143
  onehot-v128-single   k-major, single launches, one-hot          0.03  0.01      0.03    0.02   0.00  3240 / 262143
  segsum-cutoff        k-major, pair, one-hot (352 x 200 buckets) 0.02  0.12      0.05    0.02   0.00  25949 / 675818
  regtile-db           k-major, pair, register-tile backward scan 0.03  0.01      0.05    0.02   0.00  562 / 131072
  consecutive-2        k-major, pair, segment sums                0.02  0.01      0.04    0.01   0.00  955 / 131072
  replay-A-2           k-major, pair, segment sums                0.02  0.01      0.05    0.02   0.00  887 / 131071

(db 0.00 also where a backward scan summed it -- all cases but thin-256 and thin-128: the scans' sums agree with the column sums
of the STORED dZ to within 0.5 % of the rounding model's bound, i.e. they add the values they store.  Run with -s for the lines.)
"""
import numpy as np
import pytest

from tests import window_grads as WG
from tests import window_ref as R
from tests.test_window_intermediates_gpu import _engine, _train

pytestmark = pytest.mark.gpu

KM, ST, TR, SEG, PCTX = WG.WG_KMAJOR, WG.WG_SCAN_T, WG.WG_TRANSPOSE, WG.WG_SEGSUM, WG.WG_PAIR_CTX
_W2, _F8, _RT = R._W2, R._F8, R._RT
_WIDE1 = {"KL_WIDE_FWD_MIN": "1", "KL_SCAN2": "0"}


def _case(name, env, shape, route, pairs, db_scan, n_ctx=1, names=None):
    return R._case(name, "", env, shape, *(names or ("", "")), n_ctx=n_ctx), route, pairs, db_scan


# (case, wg_route, wg_pair_mask, wg_db_scan_mask) -- the route each shape and switch must take
CASES = [
    # K-major plan, dU / dK pairs on the 256 x 256 tile; and one launch per product
    _case("kmajor-pairs", {}, (2, 512, 64, 1024, 4), KM | SEG, 0b10, 0b11),
    _case("kmajor-single", {"KL_FUSE_WG": "0"}, (2, 512, 64, 1024, 4), KM | SEG, 0, 0b11),
    # B*T = 864 = 27 x 32: no multiple of the K-major kernels' 64-row k-step, so the plan does not apply and the products
    # contract over the transposed outputs of the first-generation wide scans (HTf + B, ldtf = (T+1) B) -- with and without
    # KL_GEMM_AN=0, which forces the same route
    _case("bt864-wide1", _WIDE1, (2, 512, 64, 144, 6), ST | SEG, 0, 0b11),
    _case("bt864-gemm-an-off", dict(_WIDE1, KL_GEMM_AN="0"), (2, 512, 64, 144, 6), ST | SEG, 0, 0b11),
    # explicit transposes into buffers padded from B*T = 45 to 48 rows
    _case("thin-256", {}, (2, 256, 40, 5, 9), TR | SEG, 0, 0),
    # depth 3: layer 2 reads the masked outputs of layer 1 (off_Hd); the second context table by a one-hot product
    _case("thin-128", {"KL_W128": "0"}, (3, 128, 30, 20, 6), TR | SEG, 0, 0, n_ctx=2),
    # depth 4, every db from the multi-layer scan; B*T = 165 padded to 168
    _case("w128-multi-ragged", {"KL_W128_MIN": "1"}, (4, 128, 30, 33, 5), TR | SEG, 0, 0b1111),
    # width 100 padded to 128: rows and columns of the padding exactly zero
    _case("padded-width", {}, (2, 100, 50, 24, 9), TR | SEG, 0, 0b11),
    _case("w1024-ragged", {"KL_W32_MIN_RB": "1"}, (2, 1024, 40, 40, 4), TR | SEG, 0, 0b11),
    # layer 0 by one-hot products: 64 characters pad to 64 table rows, no multiple of 128, so the first context variable's
    # product cannot share the characters' launch; with 128 characters it does, and with KL_FUSE_WG=0 it does not
    _case("onehot-v64", {"KL_SEGSUM": "0"}, (2, 512, 64, 1024, 4), KM, 0b10, 0b11),
    _case("onehot-v128-paired", {"KL_SEGSUM": "0"}, (2, 512, 128, 1024, 4), KM | PCTX, 0b10, 0b11),
    _case("onehot-v128-single", {"KL_SEGSUM": "0", "KL_FUSE_WG": "0"}, (2, 512, 128, 1024, 4), KM, 0, 0b11),
    # 330 characters (352 table rows) x 200 context values: more buckets than the segment sums take
    _case("segsum-cutoff", {}, (2, 512, 330, 1024, 4), KM, 0b10, 0b11),
    # db summed by the register-tile backward scan: it needs six 16-row blocks per workgroup and step (3072 streams) and
    # three steps -- T = 3 still selects it
    _case("regtile-db", {}, (2, 512, 64, 3072, 3), KM | SEG, 0b10, 0b11, names=((_W2, _F8), _RT)),
]
CONSECUTIVE = CASES[0]
REPLAY_A = CASES[0]
REPLAY_B = _case("replay-B", {}, (2, 512, 64, 2048, 3), KM | SEG, 0b10, 0b11)

_results = {}


def _grads_of(entry, w, lm, inp):
    """-> (line, report, GradMismatch or None) for the window that just ran on lm"""
    case, route, pairs, db_scan = entry
    win = R.read_window_padded(lm)
    info, view = win["info"], win["view"]
    assert (info["B"], info["T"], info["n"], info["groups"]) == (case.B, case.T, case.B, 1), info
    text = WG.route_text(view)
    assert (view["wg_route"], view["wg_pair_mask"], view["wg_db_scan_mask"]) == (route, pairs, db_scan), (case.name, text, view)
    masked = [bool(o) for o in view["off_Hd"]]
    assert masked == [l > 0 for l in range(case.depth)], view["off_Hd"]
    report, err = WG.check_window_grads(win, inp["idx"], inp["ctx"], lm.params.detach().cpu().numpy(),
                                        lm.grads.detach().cpu().numpy(), lm.layout, width=lm.width, where=case.name, raise_=False)
    line = "WG RATIOS | %s | %s | %s | %s" % (case.name, " ".join("%s=%s" % kv for kv in case.env.items()) or "defaults", text,
                                            WG.ratio_line(report, case.depth))
    return line, report, err


def _result(entry, monkeypatch):
    case = entry[0]
    if case.name not in _results:
        w, lm = _engine(case, monkeypatch)
        inp = R.make_inputs(case)
        lm.set_states(inp["states"])
        _train(lm, inp, names=(case.fwd, case.bwd) if case.bwd != ("",) else None)
        _results[case.name] = _grads_of(entry, w, lm, inp)
    return _results[case.name]


def _assert_products(line, err):
    print(line)
    if err is not None and err.parts - {WG.CHARACTERS}:
        raise WG.GradMismatch([f for f in err.failures if f[0] != WG.CHARACTERS], line)


def _assert_characters(line, err):
    print(line)
    if err is not None and WG.CHARACTERS in err.parts:
        raise WG.GradMismatch([f for f in err.failures if f[0] == WG.CHARACTERS], line)


@pytest.mark.parametrize("entry", CASES, ids=lambda e: e[0].name)
def test_window_grads(monkeypatch, entry):
    line, _report, err = _result(entry, monkeypatch)
    _assert_products(line, err)


@pytest.mark.parametrize("entry", CASES, ids=lambda e: e[0].name)
def test_window_grads_characters(monkeypatch, entry):
    """layer 0's character rows of the same runs (see the module text)"""
    line, _report, err = _result(entry, monkeypatch)
    _assert_characters(line, err)


def test_window_grads_consecutive_windows(monkeypatch):
    """two windows on one engine, the second a replayed graph on carried state: its gradients are the products of ITS arrays,
    nothing of the first window's sums remains (the check sees a leftover of 1e-5 of an array's largest entry)"""
    entry = CONSECUTIVE
    case = entry[0]
    w, lm = _engine(case, monkeypatch)
    inp = R.make_inputs(case, seed=21)
    lm.set_states(inp["states"])
    _train(lm, inp)
    first = lm.grads.detach().cpu().numpy().copy()
    inp = R.make_inputs(case, seed=22, states=lm.get_states())
    _train(lm, inp)
    assert not np.array_equal(first, lm.grads.detach().cpu().numpy())
    line, _report, err = _grads_of(entry, w, lm, inp)
    _assert_products(line.replace(case.name, "consecutive-2", 1), err)
    _assert_characters(line.replace(case.name, "consecutive-2 (characters)", 1), err)


def test_window_grads_after_replay(monkeypatch):
    """shape A, shape B, then A again on one engine, one workspace and the same state buffers (as
    test_window_intermediates_after_replay): A's second window is a replayed graph behind a window of another shape, and both
    its gradients and what the view says about its route must be A's"""
    A, Bc = REPLAY_A, REPLAY_B
    w, lm = _engine(A[0], monkeypatch)
    big = max(lm.lib.kl_window_workspace_bytes(lm.handle, e[0].B, e[0].T, 1) for e in (A, Bc))
    ws = lm.torch.empty(big, dtype=lm.torch.uint8, device=lm.device)
    lm._workspace = lambda B, T, training: ws
    lm._ws = ws
    states = {}
    for entry, seed in ((A, 21), (Bc, 21), (A, 22)):
        case = entry[0]
        inp = R.make_inputs(case, seed=seed)
        if case.B in states:
            lm.states = states[case.B]      # (the same buffer: its address is part of the captured graph's key)
        lm.set_states(inp["states"])
        states[case.B] = lm.states
        _train(lm, inp)
    line, _report, err = _grads_of(A, w, lm, inp)
    _assert_products(line.replace(A[0].name, "replay-A-2", 1), err)
    _assert_characters(line.replace(A[0].name, "replay-A-2 (characters)", 1), err)
