"""The look-up tables' gradients of kl_train_window -- dE (output layer, layer 0's character sums, regulariser) and every dCtx_n
(context sums, regulariser) -- held to the f64 references of what the kernels left in the workspace (tests/table_grads.py:
1e-5 of the largest back-propagated entry plus four f32 ulps of what shares the entry, exact zeros where they are due), and the
regulariser kernels on caller buffers (kl_test_regulariser_grads) against the oracle's gradient and value.

Windows: `_engine` and `_train` of tests/test_window_intermediates_gpu.py with the tables replaced by regulariser-neutral ones
(`table_grads.neutral_tables`: only then does the f32 total resolve the back-propagated part -- the precondition is asserted
from the references' numbers), inputs by `window_ref.make_inputs` with the context ids of the first real streams overwritten
so that ids 0, 1, R-2 and R-1 all occur.  Every case asserts the route it is there for, through wg_route and out_route of the
view, before it checks numbers:
  * all of tests/test_window_grads_gpu.py's CASES (layer 0's routes: segment sums, one-hot products, the context pair, the
    bucket cutoff, explicit transposes with B*T 45 -> 48 and 165 -> 168, two context tables, width 100 -> 128, V = 330 -> 352),
    whose output layers are GEMM + softmax (widths 256 .. 1024) or the width-128 kernel that also delivers dH;
  * `last-only` of window_ref.CASES: dlogits non-zero at t = T - 1 only;
  * out-ws-kmajor   (2, 512, 256, 2048, 4): B*T = 8192, so logits_ce_ws, dh_ws and the K-major dE all apply (V = Vp = 256);
  * out-v256-gemm   (2, 512, 256, 144, 6), first-generation wide scans: V = 256 through GEMM + softmax_ce and dlogits^T;
  * no-context      (2, 128, 40, 20, 9) without context variables;
  * onehot-two-ctx  (3, 128, 30, 20, 6), KL_SEGSUM=0: both context tables by one-hot products, i.e. the transposed strides
    of ctx_grad_c_kernel (with segment sums variable 0 is row-major);
  * the second of two consecutive windows on one workspace (padded-width's shape), and a replayed graph behind a window of
    another shape (kmajor-pairs behind 2048 streams x 3 steps).

The regulariser hook: `table_grads.REGULARISER_CASES` (why the characters' neutral tables have at most 17 rows is told there);
gX is pre-filled to prove `+=`, loss_acc[0], [1] and [3] must come back untouched.  reg_stats_kernel's `D > 1024` branch is
reached by the 40 x 1056 table (the engine takes any width that is a multiple of 32).

Observed on an MI355X (error / bound, the bound is 1.00; "near": layer 0's character sums within 1e-5 of a bf16 rounding
boundary out of the non-zero ones; run with -s for the lines):

  case                 weight-gradient route, layer 0     output layer                         dE    dCtx       near
  kmajor-pairs         k-major, segment sums              GEMMs + softmax, dlogits^T           0.26  0.01       780 / 131072
  kmajor-single        k-major, segment sums              GEMMs + softmax, dlogits^T           0.26  0.01       780 / 131072
  bt864-wide1          scan-transposed, segment sums      GEMMs + softmax, dlogits^T           0.07  0.02       4526 / 131069
  bt864-gemm-an-off    scan-transposed, segment sums      GEMMs + softmax, dlogits^T           0.07  0.02       4526 / 131069
  thin-256             transposes, segment sums           GEMMs + softmax, dlogits^T           0.02  0.01       570 / 22528
  thin-128             transposes, segment sums           width-128 kernel, dlogits^T          0.03  0.01 0.01  927 / 12800
  w128-multi-ragged    transposes, segment sums           width-128 kernel, dlogits^T          0.06  0.01       1031 / 14846
  padded-width         transposes, segment sums           width-128 kernel, dlogits^T          0.05  0.01       1518 / 14398
  w1024-ragged         transposes, segment sums           GEMMs + softmax, dlogits^T           0.01  0.02       15001 / 151521
  onehot-v64           k-major, one-hot                   GEMMs + softmax, dlogits^T           0.26  0.01       780 / 131072
  onehot-v128-paired   k-major, one-hot, paired           GEMMs + softmax, dlogits^T           0.31  0.01       2889 / 262144
  onehot-v128-single   k-major, one-hot                   GEMMs + softmax, dlogits^T           0.31  0.01       2889 / 262144
  segsum-cutoff        k-major, one-hot                   GEMMs + softmax, dlogits^T           0.28  0.01       23157 / 675823
  regtile-db           k-major, segment sums              GEMMs + softmax, dlogits^T           0.35  0.01       559 / 131072
  last-only            transposes, segment sums           width-128 kernel, dlogits^T          0.01  0.01       2253 / 26617
  out-ws-kmajor        k-major, segment sums              width-512 kernels, k-major dE        0.57  0.01       5906 / 524287
  out-v256-gemm        scan-transposed, segment sums      GEMMs + softmax, dlogits^T           0.20  0.01       51051 / 489358
  no-context           transposes, segment sums           width-128 kernel, dlogits^T          0.05  -          1908 / 15867
  onehot-two-ctx       transposes, one-hot                width-128 kernel, dlogits^T          0.04  0.01 0.01  910 / 12799
  consecutive-2        transposes, segment sums           width-128 kernel, dlogits^T          0.18  0.01       1370 / 15597
  replay-A-2           k-major, segment sums              GEMMs + softmax, dlogits^T           0.31  0.01       723 / 131072

  rule         tables     cases  row 0   rows >= 1  value
  characters   0.3 / 0.5  14     0.01    0.02       0.03
  characters   neutral    6      0.33    0.13       0.01
  contexts     0.3 / 0.5  10     0.01    0.10       0.01
  contexts     neutral    5      0.01    0.02       0.01

(57 tests in 5.8 s, the longest 0.9 s.  dE is the only part above 0.5: 0.57 where 8192 rows are contracted, 0.26 .. 0.35 at
4096 .. 9216 rows, 0.07 .. 0.20 at 864 rows, 0.06 or less up to 216 rows except the second of two consecutive windows (0.18,
whose largest entry is a fifth of the first window's).  The margin goes to the f32 accumulation of the output-layer product
over the B*T rows and its split-K partial sums, against a bound of 1e-5 of the LARGEST entry whatever the number of rows --
read from the growth with the row count, not measured part by part.  A neutral character table's row 0 is the regulariser's
own cancellation, see tests/table_grads.py; everything else of the regulariser kernels lies at 0.13 or below.  The
regulariser VALUE lands at 0.03 of its 1e-5 relative bound or below, which is why `check_train_window_gradients` now holds
it to that instead of 1e-3.)
"""
import ctypes as C

import numpy as np
import pytest

from tests import table_grads as TG
from tests import window_grads as WG
from tests import window_ref as R
from tests.test_table_grads_ref import edge_contexts
from tests.test_window_grads_gpu import CASES as WG_CASES
from tests.test_window_intermediates_gpu import _engine, _train

pytestmark = pytest.mark.gpu

KM, ST, TR, SEG, PCTX = WG.WG_KMAJOR, WG.WG_SCAN_T, WG.WG_TRANSPOSE, WG.WG_SEGSUM, WG.WG_PAIR_CTX
WS, W128, DHWS, DEKM = TG.OUT_LOGITS_WS, TG.OUT_LOGITS_W128, TG.OUT_DH_WS, TG.OUT_DE_KMAJOR
_WIDE1 = {"KL_WIDE_FWD_MIN": "1", "KL_SCAN2": "0"}


def _out_route_of(case):
    """the output layer of tests/test_window_grads_gpu.py's cases: none has V = 256, so neither of the width-512 kernels
    applies and dE is never K-major (that takes a whole number of 256-row tiles of characters); at (padded) width 128 the one
    kernel that also delivers dH"""
    return W128 if case.width <= 128 else 0


# The context tables' scale.  With `neutral_tables`' 1e-3 their regulariser gradient is 6.7e-5 .. 7.4e-5.  Measured on the
# MI355X with that scale, max|back-propagated part| of dCtx_0 was 5.0e-4 .. 2.9e-3 in the cases of 20 .. 40 streams, 9.0e-5
# and 9.3e-5 at 144 streams, 1.7e-4 at width 1024 -- precondition met --, but 3.8e-5 at depth 4 with 33 streams
# (w128-multi-ragged), 1.8e-5 .. 2.3e-5 at 1024 streams, 1.3e-5 at 2048 and 9.4e-6 at 3072: the mean over more positions
# leaves less per context id.  Those cases scale by 1e-5 (regulariser gradient 7e-7); the precondition is asserted as it is.
SMALL_CTX = 1e-5
_SMALL_CTX_CASES = {"kmajor-pairs", "kmajor-single", "w128-multi-ragged", "onehot-v64", "onehot-v128-paired", "onehot-v128-single",
                    "segsum-cutoff", "regtile-db", "out-ws-kmajor"}


def _entry(name, env, shape, wg_route, out_route, n_ctx=1):
    return R._case(name, "", env, shape, "", "", n_ctx=n_ctx), wg_route, out_route


# (case, wg_route, out_route)
CASES = [(e[0], e[1], _out_route_of(e[0])) for e in WG_CASES] + \
        [(next(c for c in R.CASES if c.name == "last-only"), TR | SEG, W128),
         _entry("out-ws-kmajor", {}, (2, 512, 256, 2048, 4), KM | SEG, WS | DHWS | DEKM),
         _entry("out-v256-gemm", _WIDE1, (2, 512, 256, 144, 6), ST | SEG, 0),
         _entry("no-context", {}, (2, 128, 40, 20, 9), TR | SEG, W128, n_ctx=0),
         _entry("onehot-two-ctx", {"KL_SEGSUM": "0"}, (3, 128, 30, 20, 6), TR, W128, n_ctx=2)]
BY_NAME = {e[0].name: e for e in CASES}
# (the second of two windows starts from the state the first left, which is smaller than the drawn one, and so are its
#  gradients: at 1024 streams E's back-propagated part, 5.3e-4, fell below the regularisers' 6.2e-4.  24 streams leave 1e-2.)
CONSECUTIVE = BY_NAME["padded-width"]
REPLAY_A = BY_NAME["kmajor-pairs"]
REPLAY_B = _entry("replay-B", {}, (2, 512, 64, 2048, 3), KM | SEG, 0)


def _neutral_engine(case, monkeypatch):
    from ocrd_keraslm_amd.lib import hipabi
    w, lm = _engine(case, monkeypatch)
    w = TG.neutral_tables(w, SMALL_CTX if case.name in _SMALL_CTX_CASES else 1e-3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    return w, lm


def _inputs(case, **kw):
    return edge_contexts(R.make_inputs(case, **kw), case.n_ctx)


def _check(entry, lm, inp, name=None):
    case, wg_route, out_route = entry
    win = R.read_window_padded(lm)
    info, view = win["info"], win["view"]
    assert (info["B"], info["T"], info["n"], info["groups"]) == (case.B, case.T, case.B, 1), info
    text = TG.route_text(view)
    assert (view["wg_route"], view["out_route"]) == (wg_route, out_route), (case.name, text, view)
    assert view["ld_dlogits"] == -(-case.voc // 32) * 32 and win["dlogits"].shape == (case.B * case.T, view["ld_dlogits"])
    if case.last_only:
        assert not win["dlogits"].reshape(case.T, case.B, -1)[:-1].any() and win["dlogits"].any()
    report, err = TG.check_table_grads(win, inp["idx"], inp["ctx"] if case.n_ctx else None, lm.params.detach().cpu().numpy(),
                                       lm.grads.detach().cpu().numpy(), lm.layout, width=lm.width, dummy_from=inp["n_real"],
                                       where=name or case.name, raise_=False, precondition=False)
    print("TABLE RATIOS | %s | %s | %s | %s | precondition %s" % (name or case.name, " ".join("%s=%s" % kv for kv in case.env.items()) or "defaults",
                                                               text, TG.ratio_line(report), TG.precondition_line(report)))
    hidden = {k: v["precondition"] for k, v in report.items() if not v["precondition"][0] <= v["precondition"][1]}
    assert not hidden, (name or case.name, "max|regulariser gradient| > max|back-propagated part|", hidden)
    if err is not None:
        raise err
    return report


@pytest.mark.parametrize("entry", CASES, ids=lambda e: e[0].name)
def test_table_grads(monkeypatch, entry):
    case = entry[0]
    _w, lm = _neutral_engine(case, monkeypatch)
    inp = _inputs(case)
    lm.set_states(inp["states"])
    _train(lm, inp)
    _check(entry, lm, inp)


def test_table_grads_consecutive_windows(monkeypatch):
    """two windows on one engine and one workspace, the second a replayed graph on carried state: its table gradients are made
    of ITS dlogits and sums, nothing of the first window's remains"""
    entry = CONSECUTIVE
    case = entry[0]
    _w, lm = _neutral_engine(case, monkeypatch)
    inp = _inputs(case, seed=21)
    lm.set_states(inp["states"])
    _train(lm, inp)
    first = R.read_window_padded(lm)["dlogits"].copy()
    inp = _inputs(case, seed=22, states=lm.get_states())
    _train(lm, inp)
    assert not np.array_equal(first, R.read_window_padded(lm)["dlogits"])
    _check(entry, lm, inp, name="consecutive-2")


def test_table_grads_after_replay(monkeypatch):
    """shape A, shape B, then A again on one engine, one workspace and the same state buffers (as
    test_window_grads_after_replay): A's second window is a replayed graph, and out_route must still be A's"""
    A, Bc = REPLAY_A, REPLAY_B
    _w, lm = _neutral_engine(A[0], monkeypatch)
    big = max(lm.lib.kl_window_workspace_bytes(lm.handle, e[0].B, e[0].T, 1) for e in (A, Bc))
    ws = lm.torch.empty(big, dtype=lm.torch.uint8, device=lm.device)
    lm._workspace = lambda B, T, training: ws
    lm._ws = ws
    states = {}
    for entry, seed in ((A, 21), (Bc, 21), (A, 22)):
        case = entry[0]
        inp = _inputs(case, seed=seed)
        if case.B in states:
            lm.states = states[case.B]      # (the same buffer: its address is part of the captured graph's key)
        lm.set_states(inp["states"])
        states[case.B] = lm.states
        _train(lm, inp)
    _check(A, lm, inp, name="replay-A-2")


def _hook(X, mode, fill):
    """kl_test_regulariser_grads on table X -> (gradient = gX after - before, loss_acc after, return code)"""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    R_, D = X.shape
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    g = torch.from_numpy(fill).to(dev)
    acc = torch.tensor([3.0, 5.0, 0.0, 7.0], dtype=torch.float32, device=dev)
    scratch = torch.full((3 * D + R_ + 8,), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.kl_test_regulariser_grads(p(x), R_, D, mode, p(g), p(acc), p(scratch), C.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    return g.cpu().numpy(), acc.cpu().numpy(), rc


@pytest.mark.parametrize("case", TG.REGULARISER_CASES, ids=lambda c: "%s-%dx%d-%s" % ("ctx" if c[0] else "char", c[1], c[2], c[4]))
def test_regulariser_hook(case):
    mode = case[0]
    X = TG.regulariser_case_table(case)
    # gX comes in non-zero everywhere, at 2^-13 .. 2^-12 of the gradient it is going to receive: the kernel's `+=` then rounds
    # once more, by at most 2^-24 of the entry -- a quarter of the four f32 ulps that the bound grants the entry's terms
    ref, _value, _bound = TG.regulariser_bounds(X, mode)
    rng = np.random.default_rng(7)
    fill = (rng.uniform(0.5, 1.0, X.shape) * np.maximum(np.abs(ref), 1e-30) * 2.0 ** -12).astype(np.float32)
    got, acc, rc = _hook(X, mode, fill)
    assert rc == 0
    assert (acc[0], acc[1], acc[3]) == (3.0, 5.0, 7.0), acc
    assert (fill != 0).all() and (got != 0).any()
    grad = got.astype(np.float64) - fill.astype(np.float64)
    rep = TG.check_regulariser(X, mode, grad, float(acc[2]), where=case, raise_=False)
    print("REG RATIOS | %s | %d x %d | %s | row 0 %.2f | rows >= 1 %.2f | value %.2f" % ("contexts" if mode else "characters", X.shape[0], X.shape[1],
                                                                                      case[4], rep["row0"], rep["body"], rep["value"]))
    TG.check_regulariser(X, mode, grad, float(acc[2]), where=case)


def test_regulariser_hook_refuses():
    """KL_ERR_SHAPE where the launcher refuses (more columns than its statistics kernel has LDS for), KL_ERR_ARG for no rule"""
    import torch
    X = np.zeros((2, 16384), dtype=np.float32)
    _g, acc, rc = _hook(X, 0, np.zeros_like(X))
    assert rc == 1 and acc[2] == 0.0      # KL_ERR_SHAPE, nothing launched
    _g, _acc, rc = _hook(np.ones((3, 8), dtype=np.float32), 2, np.zeros((3, 8), dtype=np.float32))
    assert rc == 5                        # KL_ERR_ARG
    torch.cuda.synchronize()
