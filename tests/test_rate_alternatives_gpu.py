"""kl_test_rate_topk / kl_rate_window_alts / HipLM.rate_window_alts / Rater.rate_alternatives on the GPU (run with -m gpu on
an MI355X).

What the model expected instead: per position the K most probable characters, ordered by (logit descending, id ascending),
and the rank of the character that was written.  The selection kernel alone is held to `ratebatch.alternatives_of` (numpy,
a stable sort) on the same f32 logits, exactly; the window call to kl_rate_window (bit for bit: the same operations) and
to kl_forward_window's whole softmax on the same handle; then the f64 oracle, by value, so that near-ties need no exclusions.

Bounds: 2e-5 for split-precision probabilities against f64 (test_step_batch_parity, test_rate_window_against_the_oracle),
1e-6 for one element against the whole softmax of the same logits (test_rate_window_is_forward_window_picked: eight f32
ulps below 1), 1e-3 for HIP probabilities through the Rater (test_rate_matches_reference[hip])."""
import ctypes as C

import numpy as np
import pytest

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import ratebatch, windows
from tests.test_rate_window_gpu import Abi, gather, make_model, ptr, window_inputs

pytestmark = pytest.mark.gpu

KL_ERR_STATE, KL_ERR_WORKSPACE, KL_ERR_ARG = 3, 4, 5
PATTERNS = ("normal", "rounded", "equal", "ascending", "descending", "spike")
SENT = -7777


def draw_logits(rng, pattern, rows, V):
    if pattern == "normal":
        x = rng.standard_normal((rows, V))
    elif pattern == "rounded":      # multiples of 0.5: many exact ties, within a lane's ids and across lanes
        x = np.round(2.0 * rng.standard_normal((rows, V))) / 2.0
    elif pattern == "equal":
        x = np.full((rows, V), 0.25)
    elif pattern == "ascending":    # the winner sits at the last id
        x = np.tile(np.arange(V) * 0.03125 - 1.0, (rows, 1))
    elif pattern == "descending":
        x = np.tile(1.0 - np.arange(V) * 0.03125, (rows, 1))
    else:                           # everything but the winner underflows to probability 0, and still comes in id order
        x = np.full((rows, V), -80.0)
        x[np.arange(rows), rng.integers(0, V, rows)] = 80.0
    return x.astype(np.float32)


def softmax64(x):
    z = x.astype(np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# (V, B, T, K, ld): fewer ids than lanes; K > V; one stream; the register form with idle lanes (and a padded leading dimension);
# every lane full; V % 4 != 0: the strided form below 256; several ids per lane; a real vocabulary size of
# test_output_layer_gpu.py (200: the register form).  B * T is mostly no multiple of 4: the last workgroup is partly empty.
KERNEL_CASES = [(11, 3, 5, 3, 13), (5, 2, 3, 8, 5), (64, 1, 7, 1, 64), (96, 5, 7, 3, 104), (256, 3, 5, 8, 256),
                (230, 4, 3, 4, 230), (300, 5, 7, 8, 300), (200, 2, 3, 8, 200)]


@pytest.mark.parametrize("V,B,T,K,ld", KERNEL_CASES)
def test_rate_topk_kernel_is_the_stable_sort(V, B, T, K, ld):
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    rows = B * T
    rng = np.random.default_rng(V * 1000 + B * 10 + K)
    worst = 0.0
    for pattern in PATTERNS:
        x = draw_logits(rng, pattern, rows, V)
        tgt = rng.integers(0, V, (B, T)).astype(np.int32)
        flat = tgt.reshape(-1)      # (a view)
        flat[0], flat[1], flat[2], flat[3], flat[4] = 0, V - 1, V // 2, -1, -2
        b2, t2 = np.unravel_index(2, (B, T))
        if pattern in ("normal", "rounded"):      # the target of position 2 is tied with a lower and a higher id
            x[t2 * B + b2, [0, V // 2, V - 1]] = x[t2 * B + b2, V // 2]
        b5, t5 = np.unravel_index(5, (B, T))      # position 5: the model's first choice (rank 0 < K for every K)
        flat[5] = int(np.argmax(x[t5 * B + b5]))
        if rows > 6:
            flat[6] = V                           # no character: probability 0 and no rank, the alternatives as ever
        padded = np.full((rows, ld), 1e30, dtype=np.float32)      # (columns from V on are not the row's: never an alternative)
        padded[:, :V] = x
        x_bm = x.reshape(T, B, V).transpose(1, 0, 2)
        _, want_id, _, want_rank = ratebatch.alternatives_of(x_bm, tgt, K)
        p = softmax64(x_bm)
        d_x, d_y = torch.from_numpy(padded).cuda(), torch.from_numpy(tgt).cuda()
        runs = []
        for _ in range(2):
            tprob = torch.full((rows + 8,), float(SENT), dtype=torch.float32, device="cuda")
            rank = torch.full((rows + 8,), SENT, dtype=torch.int32, device="cuda")
            alt_id = torch.full(((rows + 8) * K,), SENT, dtype=torch.int32, device="cuda")
            alt_p = torch.full(((rows + 8) * K,), float(SENT), dtype=torch.float32, device="cuda")
            assert lib.kl_test_rate_topk(ptr(d_x), ld, rows, V, ptr(d_y), B, T, K, ptr(tprob), ptr(alt_id), ptr(alt_p), ptr(rank),
                                         None) == 0
            torch.cuda.synchronize()
            out = [t.cpu().numpy() for t in (tprob, alt_id, alt_p, rank)]
            for a, n in zip(out, (rows, rows * K, rows * K, rows)):      # nothing behind the last row is touched
                assert (a[n:] == SENT).all(), pattern
            runs.append((out[0][:rows].reshape(B, T), out[1][:rows * K].reshape(B, T, K), out[2][:rows * K].reshape(B, T, K),
                         out[3][:rows].reshape(B, T)))
        (tp, ids, ap, rk), again = runs
        for a, b in zip(runs[0], again):      # two runs: bit-identical
            assert np.array_equal(u32(a), u32(b)), pattern
        assert np.array_equal(ids, want_id), (pattern, ids[want_id != ids], want_id[want_id != ids])
        assert np.array_equal(rk, want_rank), pattern
        none = tgt < 0
        assert (tp[none] == 0).all() and (ids[none] == -1).all() and (ap[none] == 0).all() and (rk[none] == -1).all(), pattern
        assert (tp[tgt >= V] == 0).all() and (rk[tgt >= V] == -1).all(), pattern
        assert (ap[ids < 0] == 0).all(), pattern
        if K > V:
            assert (ids[~none][:, V:] == -1).all() and (ids[~none][:, :V] >= 0).all(), pattern
        want_p = np.where(ids >= 0, np.take_along_axis(p, np.maximum(ids, 0), axis=2), 0.0)
        known = (tgt >= 0) & (tgt < V)
        want_t = np.where(known, np.take_along_axis(p, np.where(known, tgt, 0)[:, :, None], axis=2)[:, :, 0], 0.0)
        worst = max(worst, float(np.abs(ap - want_p).max()), float(np.abs(tp - want_t).max()))
        # rank < K: the target is among the alternatives, with the very float tprob holds
        hit = known & (rk < K)
        assert hit.any(), pattern
        bb, tt = np.nonzero(hit)
        assert np.array_equal(ids[bb, tt, rk[bb, tt]], tgt[bb, tt]), pattern
        assert np.array_equal(u32(ap[bb, tt, rk[bb, tt]]), u32(tp[bb, tt])), pattern
    print("V %d: max |alt_p, tprob - f64 softmax| = %.3g" % (V, worst))
    assert worst < 2e-5, worst


def test_rate_topk_kernel_refuses():
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    V, B, T = 11, 2, 3
    x = torch.zeros((B * T, V), dtype=torch.float32, device="cuda")
    y = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    f, i = torch.zeros(B * T * 8, dtype=torch.float32, device="cuda"), torch.zeros(B * T * 8, dtype=torch.int32, device="cuda")
    call = lambda K, rows=B * T, ids=i: lib.kl_test_rate_topk(ptr(x), V, rows, V, ptr(y), B, T, K, ptr(f), ptr(ids), ptr(f), ptr(i), None)
    assert call(0) == KL_ERR_ARG and call(9) == KL_ERR_ARG
    assert call(3, rows=B * T + 1) == KL_ERR_ARG
    assert call(3, ids=None) == KL_ERR_ARG
    assert call(3) == 0
    torch.cuda.synchronize()


class AltsAbi(Abi):
    """kl_rate_window_alts on ONE set of device buffers for every K: the same pointers, so that only K tells the calls apart"""

    def __init__(self, lm, B, T):
        super(AltsAbi, self).__init__(lm, B, T)
        torch, dev = self.torch, lm.device
        self.n_alts = dict((K, lm.lib.kl_rate_alts_workspace_bytes(lm.handle, B, T, K)) for K in (1, 3, 8))
        self.ws_alts = torch.empty(self.n_alts[8], dtype=torch.uint8, device=dev)
        self.a_tprob = torch.empty((B, T), dtype=torch.float32, device=dev)
        self.a_rank = torch.empty((B, T), dtype=torch.int32, device=dev)
        self.a_id = torch.empty(B * T * 8, dtype=torch.int32, device=dev)
        self.a_p = torch.empty(B * T * 8, dtype=torch.float32, device=dev)

    def alts(self, idx, ctx, tgt, K, tprob=True, rank=True, bits=True, ws_bytes=None, null_ids=False, null_p=False):
        lm = self.lm
        with lm._launch():
            x, z, y = self.d(idx), (self.d(ctx) if lm.n_ctx else None), (self.d(tgt) if tgt is not None else None)
            code = self.lib.kl_rate_window_alts(
                lm.handle, self.B, self.T, K, ptr(x), ptr(z), ptr(y), ptr(self.states), ptr(self.a_tprob) if tprob else None,
                None if null_ids else ptr(self.a_id), None if null_p else ptr(self.a_p), ptr(self.a_rank) if rank else None,
                ptr(self.bits) if bits else None, ptr(self.status), ptr(self.ws_alts),
                self.n_alts[8] if ws_bytes is None else ws_bytes, lm._stream())
        self.torch.cuda.synchronize()
        return code

    def results(self, K):
        n = self.B * self.T * K
        return (self.a_tprob.cpu().numpy().copy(), self.a_id[:n].cpu().numpy().reshape(self.B, self.T, K).copy(),
                self.a_p[:n].cpu().numpy().reshape(self.B, self.T, K).copy(), self.a_rank.cpu().numpy().copy())


def against_the_whole_softmax(full, tgt, ids, ap, rk, tol):
    """the alternatives of the positions with a target against a distribution of the same logits, by value: alt_p is the
    distribution's value at alt_id, non-increasing, over distinct ids; nothing outside the list lies more than tol above
    its last entry; the rank is the number of ids ahead of the target, give or take those within tol of it"""
    K = ids.shape[-1]
    V = full.shape[-1]
    assert K <= V
    sel = tgt >= 0
    p, i, a, r, y = full[sel].astype(np.float64), ids[sel], ap[sel], rk[sel], tgt[sel]
    assert ((i >= 0) & (i < V)).all()
    assert (np.sort(i, axis=1)[:, 1:] != np.sort(i, axis=1)[:, :-1]).all()
    assert (np.diff(a, axis=1) <= 0).all()
    worst = float(np.abs(a - np.take_along_axis(p, i, axis=1)).max())
    assert worst <= tol, worst
    rest = p.copy()
    np.put_along_axis(rest, i, -1.0, axis=1)
    assert (rest.max(axis=1) <= a[:, -1] + tol).all()
    py = np.take_along_axis(p, y[:, None], axis=1)
    assert ((p > py + tol).sum(axis=1) <= r).all() and (r <= (p > py - tol).sum(axis=1)).all()
    return worst


@pytest.mark.parametrize("depth,width,n_ctx,voc,B,T,precision", [
    (1, 64, 0, 11, 1, 1, 3), (2, 128, 1, 96, 5, 7, 3), (3, 256, 2, 300, 5, 7, 3), (2, 128, 2, 11, 5, 7, 1)])
def test_rate_window_alts_is_rate_window_and_forward_window(depth, width, n_ctx, voc, B, T, precision):
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, precision)
    rng = np.random.default_rng(depth * 1000 + width + voc + B)
    a = AltsAbi(lm, B, T)
    assert a.n_alts[8] >= a.n_alts[3] >= a.n_alts[1] > a.n_rate
    start = (0.1 * rng.standard_normal(tuple(a.states.shape))).astype(np.float32)
    worst = 0.0
    for win in range(2):
        idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
        a.states.copy_(a.torch.from_numpy(start))
        assert a.forward(idx, ctx) == 0
        full = a.probs.cpu().numpy()
        a.states.copy_(a.torch.from_numpy(start))
        a.bits.zero_()
        assert a.rate(idx, ctx, tgt) == 0
        want_p, want_bits, want_st = a.tprob.cpu().numpy(), a.bits.cpu().numpy().copy(), a.states.cpu().numpy().copy()
        runs = []
        for K in (3, 8, 3):      # one set of buffers: a capture per K, the third call replays the first's
            a.states.copy_(a.torch.from_numpy(start))
            a.bits.zero_()
            assert a.alts(idx, ctx, tgt, K) == 0
            assert float(a.status[3].item()) == 0.0
            tp, ids, ap, rk = a.results(K)
            assert np.array_equal(u32(tp), u32(want_p))
            assert np.array_equal(a.bits.cpu().numpy().view(np.uint64), want_bits.view(np.uint64))
            assert np.array_equal(u32(a.states.cpu().numpy()), u32(want_st))
            none = tgt < 0
            assert (ids[none] == -1).all() and (ap[none] == 0).all() and (rk[none] == -1).all()
            worst = max(worst, against_the_whole_softmax(full, tgt, ids, ap, rk, 1e-6))
            hit = (tgt >= 0) & (rk < K)
            bb, tt = np.nonzero(hit)
            assert np.array_equal(ids[bb, tt, rk[bb, tt]], tgt[bb, tt])
            assert np.array_equal(u32(ap[bb, tt, rk[bb, tt]]), u32(tp[bb, tt]))
            runs.append((tp, ids, ap, rk))
        for x, y in zip(runs[0], runs[2]):
            assert np.array_equal(u32(x), u32(y))
        assert np.array_equal(runs[1][1][:, :, :3], runs[0][1]) and np.array_equal(u32(runs[1][2][:, :, :3]), u32(runs[0][2]))
        assert np.array_equal(runs[1][3], runs[0][3])
        start = want_st
    print("max |alt_p - probs[alt_id]| = %.3g" % worst)


def test_rate_window_alts_optional_outputs_and_error_paths():
    depth, width, voc, n_ctx, B, T = 2, 64, 20, 1, 3, 5
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, 3)
    rng = np.random.default_rng(3)
    a = AltsAbi(lm, B, T)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    lib, h = lm.lib, lm.handle
    assert lib.kl_rate_alts_workspace_bytes(h, 0, T, 3) == 0
    assert lib.kl_rate_alts_workspace_bytes(h, B, T, 0) == 0 and lib.kl_rate_alts_workspace_bytes(h, B, T, 9) == 0
    assert a.alts(idx, ctx, tgt, 0) == KL_ERR_ARG and a.alts(idx, ctx, tgt, 9) == KL_ERR_ARG
    assert a.alts(idx, ctx, tgt, 3, null_ids=True) == KL_ERR_ARG
    assert a.alts(idx, ctx, tgt, 3, null_p=True) == KL_ERR_ARG
    assert a.alts(idx, ctx, None, 3) == KL_ERR_ARG
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_alts[3] - 1) == KL_ERR_WORKSPACE
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_rate) == KL_ERR_WORKSPACE      # (the rate workspace alone has no staging area)
    lm.set_window_mode(True)
    try:
        assert a.alts(idx, ctx, tgt, 3) == KL_ERR_STATE
    finally:
        lm.set_window_mode(False)
    # the exact size is enough; without the optional outputs their buffers stay as they were
    a.states.zero_()
    a.bits.zero_()
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_alts[3]) == 0
    tp, ids, ap, rk = a.results(3)
    bits = a.bits.cpu().numpy().copy()
    a.a_tprob.fill_(SENT)
    a.a_rank.fill_(SENT)
    a.states.zero_()
    a.bits.zero_()
    assert a.alts(idx, ctx, tgt, 3, tprob=False, rank=False, bits=False, ws_bytes=a.n_alts[3]) == 0
    tp2, ids2, ap2, rk2 = a.results(3)
    assert (tp2 == SENT).all() and (rk2 == SENT).all() and (a.bits.cpu().numpy() == 0).all()
    assert np.array_equal(ids2, ids) and np.array_equal(u32(ap2), u32(ap))
    a.states.zero_()
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_alts[3]) == 0      # ... and all of them again
    tp3, ids3, ap3, rk3 = a.results(3)
    assert np.array_equal(u32(tp3), u32(tp)) and np.array_equal(rk3, rk) and np.array_equal(ids3, ids)
    assert np.array_equal(a.bits.cpu().numpy().view(np.uint64), bits.view(np.uint64))
    with pytest.raises(ValueError):
        lm.rate_window_alts(idx, ctx, tgt, 9)


def against_the_oracle(p, y, ids, ap, rk, tol):
    """case by value, p [n][V] the oracle's distributions, y [n] targets >= 0: returns the largest |alt_p - p[alt_id]|"""
    K = min(ids.shape[1], p.shape[1])
    at = np.take_along_axis(p, ids[:, :K].astype(np.int64), axis=1)
    worst = float(np.abs(ap[:, :K] - at).max())
    assert worst < tol, worst
    best = -np.sort(-p, axis=1)[:, :K]
    assert (at > best - 2 * tol).all()
    py = np.take_along_axis(p, y[:, None].astype(np.int64), axis=1)
    assert ((p > py + 2 * tol).sum(axis=1) <= rk).all() and (rk <= (p > py - 2 * tol).sum(axis=1)).all()
    return worst


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,tol", [
    (2, 64, 50, 1, 32, 1, 2e-5), (2, 100, 50, 3, 12, 1, 2e-5), (4, 1024, 64, 2, 6, 2, 2e-5)])
def test_rate_window_alts_against_the_oracle(depth, width, voc, B, T, n_ctx, tol):
    """split precision, two consecutive windows carrying state, the shapes and the bound of test_rate_window_against_the_oracle;
    no position is left out"""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.reset_states(B)
    rng = np.random.default_rng(9)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, B, np.float64)
    worst = 0.0
    K = 3
    for win in range(2):
        idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
        ref, st, _ = O.forward_window(cfg, w64, idx, ctx, st)
        tp, ids, ap, rk = (t.cpu().numpy() for t in lm.rate_window_alts(idx, ctx, tgt, K))
        assert tp.shape == rk.shape == (B, T) and ids.shape == ap.shape == (B, T, K)
        assert tp.dtype == ap.dtype == np.float32 and ids.dtype == rk.dtype == np.int32
        sel = tgt >= 0
        assert (tp[~sel] == 0).all() and (ids[~sel] == -1).all() and (ap[~sel] == 0).all() and (rk[~sel] == -1).all()
        assert np.abs(tp - gather(ref, tgt)).max() < tol
        worst = max(worst, against_the_oracle(ref[sel], tgt[sel], ids[sel], ap[sel], rk[sel], tol))
    print("max |alt_p - oracle| = %.3g" % worst)
    lm.rate_bits_read()


def test_rate_window_alts_groups_of_streams():
    """more streams than one launch sequence of the split-precision scan takes (HipLM._rating_groups): the batch-major
    outputs are sliced by stream"""
    groups_of_streams(3)


def test_rate_window_alts_groups_of_streams_k8():
    """... with the widest rows the outputs have (K = 8): a group's slice of alt_id / alt_p is 8 * T words per stream"""
    groups_of_streams(8)


def groups_of_streams(K):
    depth, width, voc, n_ctx, B, T = 2, 512, 256, 1, 300, 4
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, 3)
    assert len(lm._rating_groups(B)) > 1
    rng = np.random.default_rng(5)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    lm.reset_states(B)
    full = lm.forward_window(idx, ctx).cpu().numpy()
    st_fwd = lm.states.cpu().numpy().copy()
    lm.reset_states(B)
    want = lm.rate_window(idx, ctx, tgt).cpu().numpy()
    want_bits = lm.rate_bits_read()
    lm.reset_states(B)
    tp, ids, ap, rk = (t.cpu().numpy() for t in lm.rate_window_alts(idx, ctx, tgt, K))
    assert np.array_equal(u32(tp), u32(want))
    assert np.array_equal(lm.rate_bits_read().view(np.uint64), want_bits.view(np.uint64))
    assert np.array_equal(u32(lm.states.cpu().numpy()), u32(st_fwd))
    none = tgt < 0
    assert (ids[none] == -1).all() and (ap[none] == 0).all() and (rk[none] == -1).all()
    worst = against_the_whole_softmax(full, tgt, ids, ap, rk, 1e-6)
    print("max |alt_p - probs[alt_id]| = %.3g" % worst)
    # ... and the same ids as the numpy statement finds in that softmax wherever its k + 1 best are further apart than the bound
    _, ref_ids, _, _ = ratebatch.alternatives_of(full, tgt, K + 1)
    top = -np.sort(-full.astype(np.float64), axis=2)[:, :, :K + 1]
    clear = (tgt >= 0) & (np.diff(-top, axis=2).min(axis=2) > 2e-6)
    assert clear.any() and np.array_equal(ids[clear], ref_ids[clear][:, :K])


def oracle_distributions(rater, texts, contexts):
    """per text the oracle's whole distribution at every position but the first, [n - 1][V]: reset, then window by window"""
    out = []
    for text, context in zip(texts, contexts):
        text = windows.normalize(text)
        rater.model.reset_states(1)
        parts = [np.asarray(rater.model.forward_window(x[None], z[None]))[0]
                 for x, z, _ in windows.stateful_windows(text, context, rater.length, rater.mapping[0])]
        out.append(np.concatenate(parts)[:len(text) - 1] if parts else np.zeros((0, rater.voc_size)))
    return out


def test_rate_alternatives_hip_matches_rate_batch_and_the_oracle_rater():
    from tests import test_rate_batch as tb
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = tb.contract_texts(tb.SEAM["model"]["length"])
    oracle = tb.make_rater(OracleLM, True, False)
    dist = oracle_distributions(oracle, texts, contexts)
    hip = tb.make_rater(hip_factory, True, False)
    assert hasattr(hip.model, "rate_window_alts")
    tol = 1e-3
    for streams, k in ((1, 3), (3, 3), (64, 3), (3, 8)):
        probs, bits = hip.rate_batch(texts, contexts, streams=streams)
        rated, bits2 = hip.rate_alternatives(texts, contexts, k=k, streams=streams)
        assert np.array_equal(bits2.view(np.uint64), bits.view(np.uint64))
        worst = 0.0
        for i, t in enumerate(texts):
            one, n = rated[i], len(windows.normalize(t))
            assert one.probs.shape == one.rank.shape == (n,) and one.alt_ids.shape == one.alt_probs.shape == (n, k)
            assert np.array_equal(u32(one.probs), u32(probs[i])), i
            if n:
                assert one.probs[0] == 1.0 and one.rank[0] == -1 and (one.alt_ids[0] == -1).all() and not one.alt_probs[0].any()
            if n > 1:
                y = windows.encode(windows.normalize(t), hip.mapping[0])[1:]
                assert np.abs(one.probs[1:] - np.take_along_axis(dist[i], y[:, None].astype(np.int64), axis=1)[:, 0]).max() < tol
                worst = max(worst, against_the_oracle(dist[i], y, one.alt_ids[1:], one.alt_probs[1:], one.rank[1:], tol))
                hit = one.rank[1:] < k
                at = np.nonzero(hit)[0] + 1
                assert np.array_equal(one.alt_ids[at, one.rank[at]], y[at - 1])
                assert np.array_equal(u32(one.alt_probs[at, one.rank[at]]), u32(one.probs[at]))
        print("streams %d, k %d: max |alt_p - oracle| = %.3g" % (streams, k, worst))
    # afterwards: a freshly reset single row
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()
