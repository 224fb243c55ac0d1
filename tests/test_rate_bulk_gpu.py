"""Bulk rating on the GPU (run with -m gpu on an MI355X): kl_rate_window_bulk, kl_rate_scatter, kl_rate_text_bits, the engine
wrappers, `Rater.rate_batch(precision="bf16")` and `keraslm-rate score`.

kl_rate_window_bulk is kl_rate_window's delivery behind the recurrence and logits of a bf16 validation window: held to
kl_forward_window in bf16 on the same training-size workspace (the same launches: states bit for bit, the picked element
within the 1e-6 test_rate_window_is_forward_window_picked holds for "same logits, same operations") and to the f64 oracle
within the bounds test_validation_windows_bf16 holds that forward to.  The two corpus-order kernels are held to their numpy
statements in lib/ratebulk.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.test_rate_window_gpu import gather, host_bits, make_model, ptr, window_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KL_ERR_STATE, KL_ERR_WORKSPACE, KL_ERR_ARG = 3, 4, 5


def device():
    import torch
    return torch, torch.device("cuda:0")


def lib_and_stream():
    from ocrd_keraslm_amd.lib import hipabi
    torch, dev = device()
    return hipabi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---------------------------------------------------------------------------------------------- kl_rate_scatter
@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("B,T", [(5, 7), (70, 33)])
def test_scatter_is_scatter_host(B, T, n_ctx):
    """bit for bit, any bit pattern (NaNs included); vlen 0, 1, T and T + 3 (clipped to T); the last row ends beyond n_out;
    everything else keeps its marker"""
    torch, dev = device()
    lib, stream = lib_and_stream()
    rng = np.random.default_rng(B * 10 + n_ctx)
    tprob = rng.integers(0, 2 ** 32, (B, T), dtype=np.uint64).astype(np.uint32)
    rows = np.zeros((B, 4 + n_ctx), dtype=np.int64)
    rows[:, 0] = np.arange(B) * (T + 2) + 3          # (disjoint ranges with gaps between them)
    rows[:, 1] = np.array([0, 1, T, T + 3])[np.arange(B) % 4]
    rows[-1, 1] = T
    rows[:, 2:] = rng.integers(-1, 200, (B, 2 + n_ctx))      # (not read here)
    n_out = int(rows[-1, 0]) + 1 + T // 2            # the last row's second half lies beyond the end
    marker = np.uint32(0x7fc0beef)
    want = np.full(n_out, marker, dtype=np.uint32)
    ratebulk.scatter_host(tprob, rows, want)
    assert (want[int(rows[-1, 0]) + 1:] != marker).all() and (want == marker).sum() >= B      # both kinds of position exist
    # (a guard band behind n_out: a write beyond the end would show in it)
    out_d = torch.from_numpy(np.full(n_out + 64, marker, dtype=np.uint32).view(np.float32)).to(dev)
    tprob_d = torch.from_numpy(tprob.view(np.float32)).to(dev)
    rows_d = torch.from_numpy(rows).to(dev)
    assert lib.kl_rate_scatter(ptr(tprob_d), ptr(rows_d), B, T, n_ctx, ptr(out_d), n_out, stream) == 0
    torch.cuda.synchronize()
    got = out_d.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n_out], want)
    assert (got[n_out:] == marker).all()


def test_scatter_and_text_bits_argument_errors():
    torch, dev = device()
    lib, stream = lib_and_stream()
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    i64 = torch.zeros(64, dtype=torch.int64, device=dev)
    d = torch.zeros(8, dtype=torch.float64, device=dev)
    ok = lambda **k: lib.kl_rate_scatter(k.get("tprob", ptr(f)), k.get("plan", ptr(i64)), k.get("B", 2), k.get("T", 4),
                                         k.get("n_ctx", 1), k.get("out", ptr(f)), 64, stream)
    assert ok() == 0
    for bad in (dict(tprob=None), dict(plan=None), dict(out=None), dict(B=0), dict(T=0), dict(n_ctx=-1), dict(n_ctx=9),
                dict(tprob=C.c_void_p(f.data_ptr() + 2)), dict(plan=C.c_void_p(i64.data_ptr() + 4)),
                dict(out=C.c_void_p(f.data_ptr() + 1))):
        assert ok(**bad) == KL_ERR_ARG, bad
    tb = lambda **k: lib.kl_rate_text_bits(k.get("probs", ptr(f)), k.get("offsets", ptr(i64)), k.get("n", 3),
                                           k.get("bits", ptr(d)), stream)
    assert tb() == 0
    for bad in (dict(probs=None), dict(offsets=None), dict(bits=None), dict(n=0),
                dict(probs=C.c_void_p(f.data_ptr() + 2)), dict(offsets=C.c_void_p(i64.data_ptr() + 4)),
                dict(bits=C.c_void_p(d.data_ptr() + 4))):
        assert tb(**bad) == KL_ERR_ARG, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- kl_rate_text_bits
def test_text_bits_is_text_bits_host():
    """1e-12 relative (the project's bound for these f64 sums: another order of 1000 additions); a zero probability hits the
    1e-99 clamp; bits are overwritten, not added to; two runs give the same bits"""
    torch, dev = device()
    lib, stream = lib_and_stream()
    rng = np.random.default_rng(4)
    sizes = [0, 1, 2, 65, 1000, 0, 2]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    probs = rng.random(int(offsets[-1])).astype(np.float32) ** 4
    probs[offsets[4] + 77] = 0.0
    want = ratebulk.text_bits_host(probs, offsets)
    assert want[4] > 328.0 and want[0] == want[1] == want[5] == 0.0
    probs_d, off_d = torch.from_numpy(probs).to(dev), torch.from_numpy(offsets).to(dev)
    runs = []
    for _ in range(2):
        bits_d = torch.full((len(sizes),), 123.0, dtype=torch.float64, device=dev)
        assert lib.kl_rate_text_bits(ptr(probs_d), ptr(off_d), len(sizes), ptr(bits_d), stream) == 0
        torch.cuda.synchronize()
        runs.append(bits_d.cpu().numpy())
    got = runs[0]
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))
    assert (got[[0, 1, 5]] == 0.0).all()
    assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (got, want)
    for i in range(len(sizes)):
        own = ratebatch.bits_of(probs[offsets[i]:offsets[i + 1]])
        assert abs(got[i] - own) <= 1e-12 * max(1.0, abs(own))


# ---------------------------------------------------------------------------------------------- kl_rate_window_bulk
class Abi(object):
    """kl_forward_window and kl_rate_window_bulk on the same device buffers of one handle: one training-size workspace"""

    def __init__(self, lm, B, T):
        import torch
        self.lm, self.lib, self.torch, self.B, self.T = lm, lm.lib, torch, B, T
        dev = lm.device
        self.states = torch.zeros((B, 2 * lm.depth, lm.pwidth), dtype=torch.float32, device=dev)
        self.n_ws = lm.lib.kl_rate_bulk_workspace_bytes(lm.handle, B, T)
        assert self.n_ws == lm.lib.kl_window_workspace_bytes(lm.handle, B, T, 1) > 0
        self.ws = torch.empty(self.n_ws, dtype=torch.uint8, device=dev)
        self.probs = torch.empty((B, T, lm.voc_size), dtype=torch.float32, device=dev)
        self.tprob = torch.full((B, T), -5.0, dtype=torch.float32, device=dev)
        self.bits = torch.zeros(B, dtype=torch.float64, device=dev)
        self.status = torch.zeros(4, dtype=torch.float32, device=dev)

    def d(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.lm.device)

    def forward(self, idx, ctx):
        lm = self.lm
        with lm._launch():
            x, z = self.d(idx), (self.d(ctx) if lm.n_ctx else None)
            code = self.lib.kl_forward_window(lm.handle, self.B, self.T, ptr(x), ptr(z), None, ptr(self.states), ptr(self.probs),
                                              None, ptr(self.ws), self.n_ws, lm._stream())
        self.torch.cuda.synchronize()
        return code

    def rate(self, idx, ctx, tgt, tprob=True, bits=True, ws_bytes=None, null_idx=False):
        lm = self.lm
        with lm._launch():
            x, z, y = self.d(idx), (self.d(ctx) if lm.n_ctx else None), (self.d(tgt) if tgt is not None else None)
            code = self.lib.kl_rate_window_bulk(lm.handle, self.B, self.T, None if null_idx else ptr(x), ptr(z), ptr(y),
                                                ptr(self.states), ptr(self.tprob) if tprob else None,
                                                ptr(self.bits) if bits else None, ptr(self.status), ptr(self.ws),
                                                self.n_ws if ws_bytes is None else ws_bytes, lm._stream())
        self.torch.cuda.synchronize()
        return code


# shapes of test_validation_windows_bf16 -- every scan family of the training forward --, then V = 300: the strided pick, and
# V = 256 at width 512: the one-pass pick
SHAPES = [(2, 128, 40, 20, 9, 1), (2, 512, 64, 512, 4, 1), (3, 100, 30, 5, 7, 2), (2, 1024, 40, 48, 4, 1), (6, 128, 30, 24, 5, 1),
          (2, 128, 300, 5, 7, 0), (2, 512, 256, 64, 16, 1)]


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", SHAPES)
def test_rate_window_bulk_is_bf16_forward_window_picked(depth, width, voc, B, T, n_ctx):
    """two consecutive windows: tprob against kl_forward_window's bf16 probabilities gathered at tgt <= 1e-6, states bit for
    bit, 0 where there is no target, bits against an f64 recomputation to 1e-12, no timed-out hand-off"""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    rng = np.random.default_rng(depth * 1000 + width + voc + B)
    a = Abi(lm, B, T)
    start = (0.1 * rng.standard_normal(tuple(a.states.shape))).astype(np.float32)
    if lm.padded:
        start[:, :, lm.width:] = 0.0      # (zero-padded hidden units carry zeros)
    worst = 0.0
    for win in range(2):
        idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
        a.states.copy_(a.torch.from_numpy(start))
        assert a.forward(idx, ctx) == 0
        want = gather(a.probs.cpu().numpy(), tgt)
        st_fwd = a.states.cpu().numpy().copy()
        a.states.copy_(a.torch.from_numpy(start))
        a.bits.zero_()
        assert a.rate(idx, ctx, tgt) == 0
        got = a.tprob.cpu().numpy()
        assert float(a.status[3].item()) == 0.0
        worst = max(worst, float(np.abs(got - want).max()))
        assert (got[tgt < 0] == 0.0).all()
        assert np.array_equal(a.states.cpu().numpy().view(np.uint32), st_fwd.view(np.uint32))
        ref_bits = host_bits(got, tgt)
        assert np.abs(a.bits.cpu().numpy() - ref_bits).max() <= 1e-12 * max(1.0, np.abs(ref_bits).max())
        assert not np.array_equal(st_fwd, start)
        start = st_fwd
    print("max |tprob - probs[tgt]| = %.3g" % worst)
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", [SHAPES[0], SHAPES[1]])
def test_rate_window_bulk_against_the_oracle(depth, width, voc, B, T, n_ctx):
    """the bounds and the model recipe (emb_std = 0.3) of test_validation_windows_bf16: probabilities within 1e-2, carried
    state within 3e-2, two consecutive windows (the engine's bf16-rounded state is carried on, as there)"""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    rng = np.random.default_rng(5)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    a = Abi(lm, B, T)
    st = O.zero_states(cfg, B, np.float64)
    for win in range(2):
        idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
        ref, st, _ = O.forward_window(cfg, w64, idx, ctx, st)
        assert a.rate(idx, ctx, tgt) == 0
        got = a.tprob.cpu().numpy()
        err = float(np.abs(got - gather(ref, tgt)).max())
        print("window %d: max |tprob - oracle| = %.3g" % (win, err))
        assert err < 1e-2, err
        states = a.states.cpu().numpy()[:, :, :width]
        for k in range(2 * depth):
            assert np.abs(states[:, k] - st[k]).max() < 3e-2
        st = [states[:, k].astype(np.float64) for k in range(2 * depth)]
    assert float(a.status[3].item()) == 0.0


def test_engine_pads_and_groups_streams():
    """600 streams at width 512, T = 4: run as 1024 (HipLM._padded_streams); the engine call equals the ABI call on the
    padded arrays, dummy rows deliver nothing and take no bits"""
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n_ctx, B, T = 2, 512, 64, 1, 600, 4
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)      # (rate_window_bulk prepares bf16 by itself)
    Bp = lm._padded_streams(B, T)
    assert Bp == 1024 and lm._stream_groups(B, T) == [(0, B)]
    rng = np.random.default_rng(6)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    torch = lm.torch
    lm.reset_states(B)
    got = lm.rate_window_bulk(lm._dev_i32(idx), lm._dev_i32(ctx), lm._dev_i32(tgt))
    assert lm.precision == hipabi.KL_PREC_BF16
    assert got.is_cuda and tuple(got.shape) == (B, T) and got.dtype == torch.float32
    got = got.cpu().numpy()
    bits = lm.rate_bits_read()
    states = lm.states.cpu().numpy().copy()
    pad = lambda arr, value: np.concatenate([arr, np.full((Bp - B,) + arr.shape[1:], value, dtype=arr.dtype)])
    a = Abi(lm, Bp, T)
    assert a.rate(pad(idx, 0), pad(ctx, 0), pad(tgt, -1)) == 0
    want = a.tprob.cpu().numpy()
    assert np.abs(got - want[:B]).max() <= 1e-6
    assert (want[B:] == 0.0).all() and (a.bits.cpu().numpy()[B:] == 0.0).all()
    assert np.abs(bits - a.bits.cpu().numpy()[:B]).max() <= 1e-12 * np.abs(bits).max()
    assert np.abs(states - a.states.cpu().numpy()[:B]).max() <= 1e-6
    assert (got[tgt < 0] == 0.0).all() and (got[tgt >= 0] > 0.0).all()
    # without probabilities: the same bits
    lm.reset_states(B)
    assert lm.rate_window_bulk(lm._dev_i32(idx), lm._dev_i32(ctx), lm._dev_i32(tgt), want_probs=False) is None
    assert np.array_equal(lm.rate_bits_read(), bits)


def test_error_paths_and_replays():
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n_ctx, B, T = 2, 64, 20, 1, 3, 5
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    rng = np.random.default_rng(3)
    a = Abi(lm, B, T)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    idx2, ctx2, tgt2 = window_inputs(rng, voc, B, T, n_ctx)
    assert lm.lib.kl_rate_bulk_workspace_bytes(lm.handle, 0, T) == 0 == lm.lib.kl_rate_bulk_workspace_bytes(lm.handle, B, 0)
    assert a.rate(idx, ctx, tgt) == KL_ERR_STATE                          # split precision: the training forward is bf16's
    lm.prepare(hipabi.KL_PREC_BF16)
    lm.set_window_mode(True)
    try:
        assert a.rate(idx, ctx, tgt) == KL_ERR_STATE                      # one target per window is not rated
    finally:
        lm.set_window_mode(False)
    assert a.rate(idx, ctx, tgt, ws_bytes=a.n_ws - 1) == KL_ERR_WORKSPACE
    assert a.rate(idx, ctx, tgt, null_idx=True) == KL_ERR_ARG
    assert a.rate(idx, ctx, None) == KL_ERR_ARG                           # a pick without targets
    assert (a.tprob.cpu().numpy() == -5.0).all() and (a.states.cpu().numpy() == 0).all()      # nothing was launched
    # a replay of the captured window reads its own inputs and targets
    assert a.rate(idx, ctx, tgt) == 0
    p1, st1 = a.tprob.cpu().numpy().copy(), a.states.cpu().numpy().copy()
    assert a.rate(idx2, ctx2, tgt2) == 0
    p2 = a.tprob.cpu().numpy().copy()
    b12 = a.bits.cpu().numpy().copy()
    a.states.copy_(a.torch.from_numpy(st1))
    assert a.forward(idx2, ctx2) == 0
    assert np.abs(p2 - gather(a.probs.cpu().numpy(), tgt2)).max() <= 1e-6
    assert not np.array_equal(p1, p2)
    both = host_bits(p1, tgt) + host_bits(p2, tgt2)
    assert np.abs(b12 - both).max() <= 1e-12 * np.abs(both).max()
    # neither output: the states advance, nothing else happens
    a.states.zero_()
    a.bits.zero_()
    assert a.rate(idx, ctx, None, tprob=False, bits=False) == 0
    assert np.array_equal(a.states.cpu().numpy().view(np.uint32), st1.view(np.uint32))
    assert (a.bits.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------- Rater, command line
ALPHABET = "abcdefgh \n"


def small_rater(factory, length=16, seed=7):
    """depth 2 / width 64 over a ten-character alphabet, embeddings of test_validation_windows_bf16's recipe (emb_std 0.3)"""
    from ocrd_keraslm_amd.lib import Rater
    r = Rater(engine_factory=factory) if factory is not None else Rater()
    r.width, r.depth, r.length = 64, 2, length
    r.stateful = True
    r.mapping = (dict((c, i) for i, c in enumerate(sorted(ALPHABET), 1)), dict((i, c) for i, c in enumerate(sorted(ALPHABET), 1)))
    r.voc_size = len(ALPHABET) + 1
    r.configure()
    cfg = O.ModelConfig(2, 64, r.voc_size, 1)
    r.model.set_weights(O.init_weights(cfg, seed=seed, emb_std=0.3, dtype=np.float32), 3)
    r.status = 2
    return r


def random_text(rng, size):
    return "".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), size))


def test_rate_batch_bf16_matches_the_oracle_rater():
    """nine texts -- an empty one, a single character, one of 3 * length + 5 characters --, two contexts, four streams (rows are
    reused): the contract of rate_batch, every probability within 1e-2 of the oracle rater's reset-and-rate loop"""
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    length = 16
    rng = np.random.default_rng(12)
    texts = [random_text(rng, s) for s in (0, 1, 2, length, length + 1, 3 * length + 5, 2 * length + 1, 7, 40)]
    contexts = [[(171 if i % 2 else 185)] for i in range(len(texts))]
    ref = small_rater(OracleLM)
    ref_probs = []
    for t, c in zip(texts, contexts):
        ref.model.reset_states(1)
        ref_probs.append(np.asarray(ref.rate(t, c), dtype=np.float64))
    hip = small_rater(hip_factory)
    hip.model.reset_states(1)
    before = np.asarray(hip.rate(texts[6], contexts[6]), dtype=np.float64)
    probs, bits = hip.rate_batch(texts, contexts, streams=4, precision="bf16")
    assert len(probs) == len(texts) and bits.shape == (len(texts),) and bits.dtype == np.float64
    worst = 0.0
    for i, t in enumerate(texts):
        assert isinstance(probs[i], np.ndarray) and probs[i].dtype == np.float32 and probs[i].shape == (len(t),)
        if len(t):
            assert probs[i][0] == 1.0
            worst = max(worst, float(np.abs(probs[i].astype(np.float64) - ref_probs[i]).max()))
        own = ratebatch.bits_of(probs[i])
        assert abs(bits[i] - own) <= 1e-12 * max(1.0, abs(own))
    print("max |rate_batch(bf16) - oracle loop| = %.3g" % worst)
    assert worst < 1e-2, worst
    assert bits[0] == 0.0 and bits[1] == 0.0 and (bits[2:] > 0).all()
    none, bits_only = hip.rate_batch(texts, contexts, streams=4, want_probs=False, precision="bf16")
    assert none is None and np.array_equal(bits_only, bits)
    # afterwards: a freshly reset single row, and split precision again
    after = np.asarray(hip.rate(texts[6], contexts[6]), dtype=np.float64)
    assert np.abs(after - before).max() < 1e-6
    # nothing but texts without a prediction
    p, b = hip.rate_batch(["", "a"], precision="bf16")
    assert [x.tolist() for x in p] == [[], [1.0]] and b.tolist() == [0.0, 0.0]


@pytest.mark.timeout(600)
def test_score_command_bf16_agrees_with_split(tmp_path):
    """`keraslm-rate score` on three small files, both precisions, one process each: |difference| in nats per character within
    the bf16 loss bound of test_validation_windows_bf16 (2e-2 * max(1, ce)) plus the 1e-3 test_rescore_shard_batch allows"""
    rng = np.random.default_rng(0)
    files = []
    for i, size in enumerate((300, 45, 131)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        name.write_text(random_text(rng, size))
        files.append(str(name))
    r = small_rater(None, length=32)
    model = str(tmp_path / "model.h5")
    r.save(model)
    del r
    out = {}
    for precision in ("split", "bf16"):
        res = subprocess.run([sys.executable, "-m", "ocrd_keraslm_amd.scripts.run", "score", "-m", model, "--streams", "2",
                              "--precision", precision] + files, cwd=ROOT, capture_output=True, text=True, timeout=500)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        lines = [json.loads(l) for l in res.stdout.strip().splitlines() if l.startswith("{")]
        assert [l["file"] for l in lines] == files
        out[precision] = lines
    for a, b, size in zip(out["split"], out["bf16"], (300, 45, 131)):
        assert a["chars"] == b["chars"] == size
        ce, ce16 = a["bits_per_char"] * np.log(2.0), b["bits_per_char"] * np.log(2.0)
        print("%s: %.5f nats/char split, %.5f bf16" % (os.path.basename(a["file"]), ce, ce16))
        assert abs(ce16 - ce) <= 2e-2 * max(1.0, ce) + 1e-3, (ce, ce16)
        assert abs(b["perplexity"] - 2.0 ** b["bits_per_char"]) <= 1e-9 * b["perplexity"]
