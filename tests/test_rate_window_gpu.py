"""kl_rate_window / HipLM.rate_window / Rater.rate_batch on the GPU (run with -m gpu on an MI355X).

Target-only delivery of rating windows: per position the probability of the character that follows, per stream
the f64 sum of -log2(max(p, 1e-99)).  Checked against kl_forward_window on the same handle (the same recurrence and
logits; the picked element must be the one the whole softmax holds at that index), against the f64 oracle, and
through the Rater and the rescoring tool."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def make_model(depth, width, voc, n_ctx=1, seed=4, emb_std=0.5):
    from ocrd_keraslm_amd.lib.engine import HipLM
    from tests.gradcheck import cached_weights
    cfg = O.ModelConfig(depth, width, voc, n_ctx)
    w = cached_weights(depth, width, voc, n_ctx, seed, emb_std)
    lm = HipLM(depth, width, voc, n_ctx)
    return cfg, w, lm


def window_inputs(rng, voc, B, T, n_ctx):
    """targets with a -1 tail, a -2 dummy row and target 0 (the unmapped character is a valid target)"""
    idx = rng.integers(0, voc, (B, T)).astype(np.int32)
    ctx = rng.integers(0, 200, (B, 1, n_ctx)).repeat(T, axis=1).astype(np.int32)
    tgt = rng.integers(0, voc, (B, T)).astype(np.int32)
    tgt[0, 0] = 0
    if T > 2:
        tgt[:, -2:] = -1
        tgt[B // 2, 1] = 0
    if B > 1:
        tgt[-1] = -2
    return idx, ctx, tgt


def gather(probs, tgt):
    """probs [B,T,V] at tgt, 0 where there is no target"""
    p = np.take_along_axis(probs, np.maximum(tgt, 0)[:, :, None], axis=2)[:, :, 0]
    return np.where(tgt >= 0, p, 0.0)


def host_bits(tprob, tgt):
    t = np.log2(np.maximum(tprob.astype(np.float64), 1e-99))
    return -np.where(tgt >= 0, t, 0.0).sum(axis=1)


class Abi(object):
    """both window calls on explicit device buffers of one handle"""

    def __init__(self, lm, B, T):
        import torch
        self.lm, self.lib, self.torch, self.B, self.T = lm, lm.lib, torch, B, T
        dev = lm.device
        self.states = torch.zeros((B, 2 * lm.depth, lm.pwidth), dtype=torch.float32, device=dev)
        self.n_fwd = lm.lib.kl_window_workspace_bytes(lm.handle, B, T, 0)
        self.n_rate = lm.lib.kl_rate_workspace_bytes(lm.handle, B, T)
        self.ws_fwd = torch.empty(self.n_fwd, dtype=torch.uint8, device=dev)
        self.ws_rate = torch.empty(self.n_rate, dtype=torch.uint8, device=dev)
        self.probs = torch.empty((B, T, lm.voc_size), dtype=torch.float32, device=dev)
        self.tprob = torch.empty((B, T), dtype=torch.float32, device=dev)
        self.bits = torch.zeros(B, dtype=torch.float64, device=dev)
        self.status = torch.zeros(4, dtype=torch.float32, device=dev)

    def d(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.lm.device)

    def forward(self, idx, ctx):
        lm = self.lm
        with lm._launch():
            x, z = self.d(idx), (self.d(ctx) if lm.n_ctx else None)
            code = self.lib.kl_forward_window(lm.handle, self.B, self.T, ptr(x), ptr(z), None, ptr(self.states), ptr(self.probs),
                                              None, ptr(self.ws_fwd), self.n_fwd, lm._stream())
        self.torch.cuda.synchronize()
        return code

    def rate(self, idx, ctx, tgt, tprob=True, bits=True, ws_bytes=None, null_idx=False):
        lm = self.lm
        with lm._launch():
            x, z, y = self.d(idx), (self.d(ctx) if lm.n_ctx else None), (self.d(tgt) if tgt is not None else None)
            code = self.lib.kl_rate_window(lm.handle, self.B, self.T, None if null_idx else ptr(x), ptr(z), ptr(y), ptr(self.states),
                                           ptr(self.tprob) if tprob else None, ptr(self.bits) if bits else None,
                                           ptr(self.status), ptr(self.ws_rate), self.n_rate if ws_bytes is None else ws_bytes,
                                           lm._stream())
        self.torch.cuda.synchronize()
        return code


# every (depth, width), n_ctx, V, (B, T) and precision of the list at least once; V = 11 and 300 take the strided
# pick kernel, 96 and 256 the one-pass kernel
@pytest.mark.parametrize("depth,width,n_ctx,voc,B,T,precision", [
    (1, 64, 0, 11, 1, 1, 3), (2, 128, 1, 96, 1, 32, 3), (2, 512, 1, 256, 64, 256, 3), (3, 256, 2, 300, 5, 7, 3),
    (2, 1024, 1, 96, 5, 7, 3), (2, 128, 2, 11, 5, 7, 1), (2, 512, 1, 256, 1, 32, 1), (2, 128, 0, 300, 64, 256, 1),
    (2, 512, 1, 230, 64, 32, 3),
    # width 1024: 2048 rows -- layer 1's gate inputs from the three ring products over the planes --, and five layers -- the
    # two-layer launches hand the window on after layers 0..3 (the routes are asserted in tests/test_forward_view_gpu.py)
    (2, 1024, 1, 40, 64, 32, 3), (5, 1024, 1, 30, 20, 3, 3)])
def test_rate_window_is_forward_window_picked(depth, width, n_ctx, voc, B, T, precision):
    """tprob against kl_forward_window's probabilities gathered at tgt: <= 1e-6 (the same operations in the same order
    should make it 0; one f32 ulp below 1 is 1.2e-7, so 1e-6 is eight ulps of slack for a different contraction by the
    compiler); the final states bit for bit"""
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, precision)
    rng = np.random.default_rng(depth * 1000 + width + voc + B)
    a = Abi(lm, B, T)
    assert a.n_rate > 0
    start = (0.1 * rng.standard_normal(tuple(a.states.shape))).astype(np.float32)
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
        start = st_fwd
    print("max |tprob - probs[tgt]| = %.3g" % worst)
    assert worst <= 1e-6, worst


def test_rate_window_groups_of_streams():
    """more streams than one launch sequence of the split-precision scan takes (HipLM._rating_groups): (300, 32)"""
    depth, width, voc, n_ctx, B, T = 2, 512, 256, 1, 300, 32
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, 3)
    assert len(lm._rating_groups(B)) > 1
    rng = np.random.default_rng(5)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    lm.reset_states(B)
    want = gather(lm.forward_window(idx, ctx).cpu().numpy(), tgt)
    st_fwd = lm.states.cpu().numpy().copy()
    lm.reset_states(B)
    got = lm.rate_window(idx, ctx, tgt).cpu().numpy()
    worst = float(np.abs(got - want).max())
    print("max |tprob - probs[tgt]| = %.3g" % worst)
    assert worst <= 1e-6, worst
    assert np.array_equal(lm.states.cpu().numpy().view(np.uint32), st_fwd.view(np.uint32))
    ref_bits = host_bits(got, tgt)
    assert np.abs(lm.rate_bits_read() - ref_bits).max() <= 1e-12 * np.abs(ref_bits).max()


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,tol", [
    (2, 64, 50, 1, 32, 1, 2e-5), (2, 512, 64, 300, 4, 1, 2e-5), (2, 100, 50, 3, 12, 1, 2e-5), (4, 1024, 64, 2, 6, 2, 2e-5),
    # the cfg2-size model over long windows: the project's stated bound for HIP probabilities (test_rater_golden, [hip])
    (2, 512, 256, 64, 256, 1, 1e-3)])
def test_rate_window_against_the_oracle(depth, width, voc, B, T, n_ctx, tol):
    """split precision, two consecutive windows carrying state, shapes of test_forward_window_parity (which holds the
    whole softmax to 2e-5 on them: one picked element needs no more); bits against an f64 recomputation from the returned
    probabilities with the same clamp, to 1e-12 relative (the reduction itself, not the model)"""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.reset_states(B)
    rng = np.random.default_rng(9)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, B, np.float64)
    total = np.zeros(B)
    worst = 0.0
    for win in range(2):
        idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
        ref, st, _ = O.forward_window(cfg, w64, idx, ctx, st)
        got = lm.rate_window(idx, ctx, tgt).cpu().numpy()
        assert got.shape == (B, T) and got.dtype == np.float32
        worst = max(worst, float(np.abs(got - gather(ref, tgt)).max()))
        assert (got[tgt < 0] == 0.0).all()
        total += host_bits(got, tgt)
    print("max |tprob - oracle| = %.3g" % worst)
    assert worst < tol, worst
    bits = lm.rate_bits_read()
    assert bits.dtype == np.float64 and bits.shape == (B,)
    assert np.abs(bits - total).max() <= 1e-12 * np.abs(total).max()
    assert (lm.rate_bits_read() == 0).all()      # (read with reset)


def test_bits_accumulate_runs_repeat_and_replays_read_their_own_targets():
    depth, width, voc, n_ctx, B, T = 2, 128, 96, 1, 7, 40
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, 3)
    rng = np.random.default_rng(2)
    a = Abi(lm, B, T)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    idx2, ctx2, tgt2 = window_inputs(rng, voc, B, T, n_ctx)

    def run():
        a.states.zero_()
        a.bits.zero_()
        assert a.rate(idx, ctx, tgt) == 0
        first_p, first_b = a.tprob.cpu().numpy().copy(), a.bits.cpu().numpy().copy()
        assert a.rate(idx2, ctx2, tgt2) == 0      # (same shapes and pointers: a replay of the captured window)
        return first_p, first_b, a.tprob.cpu().numpy().copy(), a.bits.cpu().numpy().copy()

    p1, b1, p2, b12 = run()
    q1, c1, q2, c12 = run()
    # two runs from the same state: bit-identical
    assert np.array_equal(p1.view(np.uint32), q1.view(np.uint32)) and np.array_equal(p2.view(np.uint32), q2.view(np.uint32))
    assert np.array_equal(b1.view(np.uint64), c1.view(np.uint64)) and np.array_equal(b12.view(np.uint64), c12.view(np.uint64))
    # the accumulator holds both calls
    assert np.abs(b1 - host_bits(p1, tgt)).max() <= 1e-12 * np.abs(b1).max()
    both = host_bits(p1, tgt) + host_bits(p2, tgt2)
    assert np.abs(b12 - both).max() <= 1e-12 * np.abs(both).max()
    assert (b12[:-1] > b1[:-1]).all() and b12[-1] == 0.0      # (the dummy row has no targets)
    # the second call's values are its own: the same inputs with the second targets alone
    a.states.zero_()
    assert a.rate(idx, ctx, tgt, bits=False) == 0
    assert a.forward(idx2, ctx2) == 0
    assert np.abs(p2 - gather(a.probs.cpu().numpy(), tgt2)).max() <= 1e-6
    assert not np.array_equal(p1, p2)


def test_error_paths():
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n_ctx, B, T = 2, 64, 20, 1, 3, 5
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, 3)
    rng = np.random.default_rng(3)
    a = Abi(lm, B, T)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    assert lm.lib.kl_rate_workspace_bytes(lm.handle, 0, T) == 0
    assert a.rate(idx, ctx, tgt, null_idx=True) == 5                    # KL_ERR_ARG
    assert a.rate(idx, ctx, None) == 5                                  # ... a pick without targets
    assert a.rate(idx, ctx, tgt, ws_bytes=a.n_rate - 1) == 4            # KL_ERR_WORKSPACE
    lm.set_window_mode(True)
    try:
        assert a.rate(idx, ctx, tgt) == 3                               # KL_ERR_STATE: one target per window is not rated
    finally:
        lm.set_window_mode(False)
    # neither output: the states advance as in kl_forward_window, nothing else happens
    a.states.zero_()
    assert a.forward(idx, ctx) == 0
    want = a.states.cpu().numpy().copy()
    a.states.zero_()
    a.bits.zero_()
    assert a.rate(idx, ctx, None, tprob=False, bits=False) == 0
    assert np.array_equal(a.states.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (a.bits.cpu().numpy() == 0).all()
    with pytest.raises(hipabi.KlError):
        lm.set_window_mode(True)
        try:
            lm.rate_window(idx, ctx, tgt)
        finally:
            lm.set_window_mode(False)


def test_rate_batch_hip_matches_the_oracle_rater():
    """test_rate_batch's texts: within 1e-3 of the oracle rater's reset-and-rate loop (as test_rate_matches_reference[hip]);
    the difference to the HIP engine's own loop is printed and held to the same 1e-3 (one row and n rows may take
    different scan kernels, so no tighter bound is fixed in advance)"""
    from tests import test_rate_batch as tb
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = tb.contract_texts(tb.SEAM["model"]["length"])
    ref_probs, ref_bits = tb.loop(tb.make_rater(OracleLM, True, False), texts, contexts)
    hip = tb.make_rater(hip_factory, True, False)
    hip_probs, _ = tb.loop(hip, texts, contexts)
    for streams in (1, 3, 64):
        probs, bits = hip.rate_batch(texts, contexts, streams=streams)
        none, bits_only = hip.rate_batch(texts, contexts, streams=streams, want_probs=False)
        assert none is None and np.array_equal(bits_only, bits)
        worst = worst_loop = 0.0
        for i in range(len(texts)):
            assert probs[i].dtype == np.float32 and len(probs[i]) == len(ref_probs[i])
            if len(probs[i]):
                assert probs[i][0] == 1.0
                worst = max(worst, float(np.abs(probs[i].astype(np.float64) - ref_probs[i]).max()))
                worst_loop = max(worst_loop, float(np.abs(probs[i] - hip_probs[i]).max()))
            own = -np.log2(np.maximum(probs[i][1:].astype(np.float64), 1e-99)).sum()
            assert abs(bits[i] - own) <= 1e-12 * max(1.0, abs(own))
        print("streams %d: max |rate_batch - oracle loop| = %.3g, max |rate_batch - HIP loop| = %.3g" % (streams, worst, worst_loop))
        assert worst < 1e-3 and worst_loop < 1e-3
    # afterwards: a freshly reset single row
    after = hip.rate(texts[6], contexts[6])
    assert np.abs(np.array(after, dtype=np.float64) - hip_probs[6]).max() < 1e-6


@pytest.mark.timeout(600)
def test_rescore_shard_batch(tmp_path):
    """the five documents of test_two_workers_on_one_gpu_rate_every_document through --batch 4: bits per character
    within 1e-3 of the in-process loop (that test's bound)"""
    from ocrd_keraslm_amd.lib import Rater
    alphabet = "abcdefgh \n"
    rng = np.random.default_rng(0)
    docs = []
    for i in range(5):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 10 * i))
        text = "".join(alphabet[j] for j in rng.integers(0, len(alphabet), 300 + 40 * i))
        name.write_text(text)
        docs.append((str(name), text))
    r = Rater()
    r.width, r.depth, r.length = 64, 2, 32
    r.stateful = True
    r.mapping = (dict((c, i) for i, c in enumerate(sorted(alphabet), 1)), dict((i, c) for i, c in enumerate(sorted(alphabet), 1)))
    r.voc_size = len(alphabet) + 1
    r.seed = 3
    r.configure()
    r.status = 2
    model = str(tmp_path / "model.h5")
    r.save(model)
    want = {}
    for path, text in docs:
        r.model.reset_states(1)
        probs = r.rate(text, [int(np.ceil(int(os.path.basename(path).split(".")[0].split("_")[2]) / 10))])
        want[os.path.basename(path)] = -float(np.mean(np.log2(np.maximum(probs[1:], 1e-99))))
    out = str(tmp_path / "out")
    env = dict(os.environ, KL_RESCORE_SAME_GPU="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rescore_shard.py"), "--model", model, "--gpus", "2",
                          "--batch", "4", "--out", out] + [p for p, _ in docs], env=env, capture_output=True, text=True,
                         timeout=500)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    summary = json.loads(res.stdout.strip().splitlines()[-1])
    assert summary["documents"] == 5 and summary["failed_workers"] == 0
    for name, bits in want.items():
        got = json.load(open(os.path.join(out, name + ".json")))
        assert abs(got["bits_per_char"] - bits) < 1e-3, (name, got["bits_per_char"], bits)
        assert got["chars"] == 300 + 40 * int(name.split("title")[1][0])
