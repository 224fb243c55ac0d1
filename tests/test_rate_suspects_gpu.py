"""Suspect characters on the GPU (run with -m gpu on an MI355X): kl_rate_window_alts_bulk, kl_rate_scatter_alts, kl_rate_select,
the engine wrappers, `Rater.rate_alternatives(precision="bf16")` and `Rater.suspects`.

kl_rate_window_alts_bulk is kl_rate_window_alts' delivery behind kl_rate_window_bulk's recurrence and logits: tprob, states
and bits are held to kl_rate_window_bulk bit for bit, the alternatives to kl_forward_window's bf16 softmax on the same
workspace within the 1e-6 test_rate_window_alts_is_rate_window_and_forward_window holds for "same logits, same operations".
The two corpus-order kernels are held to their numpy statements in lib/ratebulk.py, bit for bit.  Through the Rater: 1e-2
against the oracle for the bf16 path (test_rate_batch_bf16_matches_the_oracle_rater), 4e-5 between two split-precision
routes (each within 2e-5 of the oracle: test_rate_window_against_the_oracle, test_rate_window_alts_against_the_oracle)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.test_rate_alternatives_gpu import against_the_oracle, against_the_whole_softmax, oracle_distributions, u32
from tests.test_rate_bulk_gpu import Abi, device, lib_and_stream, random_text, small_rater
from tests.test_rate_suspects import contract_texts, same_as_filter, settings_of
from tests.test_rate_window_gpu import make_model, ptr, window_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KL_ERR_STATE, KL_ERR_WORKSPACE, KL_ERR_ARG = 3, 4, 5
MARK = np.uint32(0x7fc0beef)
GUARD = 64


def header_constant(name):
    """the documented value of a #define of include/keraslm_hip.h"""
    text = open(os.path.join(ROOT, "include", "keraslm_hip.h")).read()
    found = re.findall(r"^#define %s (\d+)$" % name, text, flags=re.M)
    assert len(found) == 1
    return int(found[0])


BLOCK = header_constant("KL_RATE_SELECT_BLOCK")
SCAN_THREADS = header_constant("KL_RATE_SELECT_SCAN_THREADS")


def bit_patterns(rng, shape):
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)


def marked(torch, dev, n, dtype):
    """n + GUARD words of the marker, as a device tensor of dtype (4-byte elements)"""
    return torch.from_numpy(np.full(n + GUARD, MARK, dtype=np.uint32)).to(dev).view(dtype)


def words(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1)


# ---------------------------------------------------------------------------------------------- kl_rate_scatter_alts
@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("B,T,K", [(5, 7, 1), (70, 33, 8)])
def test_scatter_alts_is_scatter_alts_host(B, T, K, n_ctx):
    """bit for bit, any bit pattern; vlen 0, 1, T and T + 3 (clipped to T); the last row ends beyond n_out; every other word,
    and a guard band behind each output, keeps its marker"""
    torch, dev = device()
    lib, stream = lib_and_stream()
    rng = np.random.default_rng(B * 10 + n_ctx)
    src = [bit_patterns(rng, (B, T)), bit_patterns(rng, (B, T)), bit_patterns(rng, (B, T, K)), bit_patterns(rng, (B, T, K))]
    rows = np.zeros((B, 4 + n_ctx), dtype=np.int64)
    rows[:, 0] = np.arange(B) * (T + 2) + 3          # (disjoint ranges with gaps between them)
    rows[:, 1] = np.array([0, 1, T, T + 3])[np.arange(B) % 4]
    rows[-1, 1] = T
    rows[:, 2:] = rng.integers(-1, 200, (B, 2 + n_ctx))      # (not read here)
    n_out = int(rows[-1, 0]) + 1 + T // 2            # the last row's second half lies beyond the end
    want = [np.full(n_out, MARK, dtype=np.uint32), np.full(n_out, MARK, dtype=np.uint32),
            np.full((n_out, K), MARK, dtype=np.uint32), np.full((n_out, K), MARK, dtype=np.uint32)]
    ratebulk.scatter_alts_host(src[0], src[1], src[2], src[3], rows, *want)
    assert (want[0][int(rows[-1, 0]) + 1:] != MARK).all() and (want[0] == MARK).sum() >= B      # both kinds of position exist
    kinds = (torch.float32, torch.int32, torch.int32, torch.float32)
    src_d = [torch.from_numpy(a).to(dev).view(k) for a, k in zip(src, kinds)]
    out_d = [marked(torch, dev, n_out * w, k) for w, k in zip((1, 1, K, K), kinds)]
    rows_d = torch.from_numpy(rows).to(dev)
    assert lib.kl_rate_scatter_alts(ptr(src_d[0]), ptr(src_d[1]), ptr(src_d[2]), ptr(src_d[3]), ptr(rows_d), B, T, K, n_ctx,
                                    ptr(out_d[0]), ptr(out_d[1]), ptr(out_d[2]), ptr(out_d[3]), n_out, stream) == 0
    torch.cuda.synchronize()
    for got, ref in zip(out_d, want):
        got = words(got)
        assert np.array_equal(got[:ref.size], ref.reshape(-1))
        assert got.size == ref.size + GUARD and (got[ref.size:] == MARK).all()


def test_scatter_alts_argument_errors():
    torch, dev = device()
    lib, stream = lib_and_stream()
    f = torch.zeros(256, dtype=torch.float32, device=dev)
    i = torch.zeros(256, dtype=torch.int32, device=dev)
    i64 = torch.zeros(64, dtype=torch.int64, device=dev)
    out = [marked(torch, dev, 64 * w, k) for w, k in zip((1, 1, 2, 2), (torch.float32, torch.int32, torch.int32, torch.float32))]
    names = ("tprob", "rank", "alt_id", "alt_p", "plan", "out_prob", "out_rank", "out_alt_id", "out_alt_p")
    good = dict(zip(names, [ptr(f), ptr(i), ptr(i), ptr(f), ptr(i64)] + [ptr(t) for t in out]))

    def call(**k):
        a = dict(good, **k)
        return lib.kl_rate_scatter_alts(a["tprob"], a["rank"], a["alt_id"], a["alt_p"], a["plan"], k.get("B", 2), k.get("T", 4),
                                        k.get("K", 2), k.get("n_ctx", 1), a["out_prob"], a["out_rank"], a["out_alt_id"],
                                        a["out_alt_p"], 64, stream)

    bad = [{name: None} for name in names] + [dict(B=0), dict(T=0), dict(K=0), dict(K=9), dict(n_ctx=-1), dict(n_ctx=9)]
    bad += [{name: C.c_void_p(good[name].value + 2)} for name in names if name != "plan"] + [dict(plan=C.c_void_p(i64.data_ptr() + 4))]
    for case in bad:
        assert call(**case) == KL_ERR_ARG, case
    torch.cuda.synchronize()
    for t in out:
        assert (words(t) == MARK).all()
    assert call() == 0      # (plan rows of zeros: vlen 0, nothing is written)
    torch.cuda.synchronize()
    for t in out:
        assert (words(t) == MARK).all()


# ---------------------------------------------------------------------------------------------- kl_rate_select
class Select(object):
    """kl_rate_select on device copies of host arrays; outputs of `room` entries plus a guard band, prefilled with the marker"""

    def __init__(self, probs, rank, alt_id, alt_p):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.n, self.K = len(probs), alt_id.shape[1]
        up = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.src = [up(probs), up(rank), up(alt_id), up(alt_p)]
        self.n_ws = self.lib.kl_rate_select_workspace_bytes(self.n)
        self.ws = self.torch.empty(max(self.n_ws, 8), dtype=self.torch.uint8, device=self.dev)

    def run(self, max_prob, min_rank, capacity, room=None, null_out=False, ws_bytes=None, shift=None, **override):
        torch = self.torch
        room = capacity if room is None else room
        self.count = torch.full((1,), -77, dtype=torch.int64, device=self.dev)
        self.pos = torch.full((room + GUARD,), -77, dtype=torch.int64, device=self.dev)
        self.out = [marked(torch, self.dev, room * w, k)
                    for w, k in zip((1, 1, self.K, self.K), (torch.float32, torch.int32, torch.int32, torch.float32))]
        a = dict(probs=ptr(self.src[0]), rank=ptr(self.src[1]), alt_id=ptr(self.src[2]), alt_p=ptr(self.src[3]), n=self.n,
                 K=self.K, count=ptr(self.count), ws=ptr(self.ws), sel_pos=ptr(self.pos), sel_prob=ptr(self.out[0]),
                 sel_rank=ptr(self.out[1]), sel_alt_id=ptr(self.out[2]), sel_alt_p=ptr(self.out[3]))
        if null_out:
            a.update(sel_pos=None, sel_prob=None, sel_rank=None, sel_alt_id=None, sel_alt_p=None)
        a.update(override)
        for name, by in (shift or {}).items():      # (a misaligned pointer)
            a[name] = C.c_void_p(a[name].value + by)
        code = self.lib.kl_rate_select(a["probs"], a["rank"], a["alt_id"], a["alt_p"], a["n"], a["K"], C.c_float(max_prob),
                                       min_rank, capacity, a["sel_pos"], a["sel_prob"], a["sel_rank"], a["sel_alt_id"],
                                       a["sel_alt_p"], a["count"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes,
                                       self.stream)
        torch.cuda.synchronize()
        return code

    def results(self):
        return int(self.count.item()), self.pos.cpu().numpy(), [words(t) for t in self.out]

    def untouched(self, first=0):
        """every output entry from `first` on, guard bands included, holds its marker"""
        count, pos, out = self.results()
        return (pos[first:] == -77).all() and all((o[first * w:] == MARK).all() for o, w in zip(out, (1, 1, self.K, self.K)))


def select_inputs(rng, n, K, pattern):
    probs = rng.random(n).astype(np.float32)
    rank = rng.integers(0, 6, n).astype(np.int32)
    if pattern != "all":      # some NaN probabilities and some positions without a prediction
        probs[rng.random(n) < 0.05] = np.float32("nan")
        rank[rng.random(n) < 0.05] = -1
    alt_id = bit_patterns(rng, (n, K)).view(np.int32)
    alt_p = bit_patterns(rng, (n, K)).view(np.float32)
    max_prob, min_rank = {"none": (-1.0, 0), "all": (float("inf"), 0), "half": (0.5, 0)}[pattern]
    if pattern == "half" and n > 2:
        probs[n // 2] = np.float32(0.5)      # a tie at the threshold is selected
        rank[n // 2] = 3
    return probs, rank, alt_id, alt_p, max_prob, min_rank


# one wave short of, exactly and one past a wave; the same around the block a workgroup owns; more blocks than the offsets
# workgroup takes per round (its second round starts inside the input)
SELECT_SIZES = [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 300000]


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_is_select_host(n):
    assert -(-300000 // BLOCK) > SCAN_THREADS
    rng = np.random.default_rng(n)
    for K in (1, 8):
        for pattern in ("none", "all", "half"):
            probs, rank, alt_id, alt_p, max_prob, min_rank = select_inputs(rng, n, K, pattern)
            want = ratebulk.select_host(probs, rank, alt_id, alt_p, max_prob, min_rank)
            m = len(want[0])
            assert {"none": m == 0, "all": m == n, "half": n < 64 or 0 < m < n}[pattern]
            s = Select(probs, rank, alt_id, alt_p)
            assert s.n_ws >= 8 * -(-n // BLOCK)
            # the counting call: no outputs at all
            assert s.run(max_prob, min_rank, 0, null_out=True) == 0
            assert s.results()[0] == m
            for capacity in sorted(set([m, m // 2, max(m - 1, 0)])):
                runs = []
                for _ in range(2 if capacity == m else 1):
                    assert s.run(max_prob, min_rank, capacity, room=m) == 0
                    count, pos, out = s.results()
                    assert count == m, (K, pattern, capacity)      # the full count, whatever the capacity
                    assert np.array_equal(pos[:capacity], want[0][:capacity])
                    for got, ref, w in zip(out, want[1:], (1, 1, K, K)):
                        assert np.array_equal(got[:capacity * w], u32(ref[:capacity]).reshape(-1)), (K, pattern, capacity)
                    assert s.untouched(first=capacity)             # entries from `capacity` on keep their marker
                    runs.append((pos, out))
                if len(runs) == 2:                                 # two runs are identical
                    assert np.array_equal(runs[0][0], runs[1][0])
                    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_select_errors_return_before_any_launch():
    rng = np.random.default_rng(2)
    n, K = 300, 3
    probs, rank, alt_id, alt_p, _, _ = select_inputs(rng, n, K, "all")
    s = Select(probs, rank, alt_id, alt_p)
    lib = s.lib
    assert lib.kl_rate_select_workspace_bytes(0) == 0 and s.n_ws > 0
    cases = [dict(probs=None), dict(rank=None), dict(alt_id=None), dict(alt_p=None), dict(count=None), dict(ws=None), dict(n=0),
             dict(K=0), dict(K=9), dict(sel_pos=None), dict(sel_alt_p=None)]
    cases += [dict(shift={name: by}) for name, by in (("probs", 2), ("rank", 1), ("alt_id", 2), ("alt_p", 2), ("sel_pos", 4),
                                                      ("sel_prob", 2), ("sel_alt_id", 2), ("count", 4), ("ws", 4))]
    for case in cases:
        assert s.run(1.0, 0, n, **case) == KL_ERR_ARG, case
        assert s.untouched() and int(s.count.item()) == -77
    assert s.run(1.0, -1, n) == KL_ERR_ARG and s.untouched() and int(s.count.item()) == -77
    assert s.run(float("nan"), 0, n) == KL_ERR_ARG and s.untouched() and int(s.count.item()) == -77
    assert s.run(1.0, 0, n, ws_bytes=s.n_ws - 1) == KL_ERR_WORKSPACE and s.untouched() and int(s.count.item()) == -77
    assert s.run(1.0, 0, n) == 0 and s.results()[0] == n


# ---------------------------------------------------------------------------------------------- kl_rate_window_alts_bulk
class AltsBulkAbi(Abi):
    """kl_forward_window, kl_rate_window_bulk and kl_rate_window_alts_bulk on ONE workspace -- the training window's plus the
    staging area of K = 8 -- and one set of output buffers for every K"""

    def __init__(self, lm, B, T):
        super(AltsBulkAbi, self).__init__(lm, B, T)
        torch, dev = self.torch, lm.device
        self.n_alts = dict((K, lm.lib.kl_rate_alts_bulk_workspace_bytes(lm.handle, B, T, K)) for K in (1, 3, 8))
        assert self.n_alts[8] >= self.n_alts[3] >= self.n_alts[1] > self.n_ws
        self.ws = torch.empty(self.n_alts[8], dtype=torch.uint8, device=dev)      # (the parent's calls pass n_ws bytes of it)
        self.a_tprob = torch.full((B, T), -5.0, dtype=torch.float32, device=dev)
        self.a_rank = torch.full((B, T), -5, dtype=torch.int32, device=dev)
        self.a_id = torch.full((B * T * 8,), -5, dtype=torch.int32, device=dev)
        self.a_p = torch.full((B * T * 8,), -5.0, dtype=torch.float32, device=dev)

    def alts(self, idx, ctx, tgt, K, ws_bytes=None, null_idx=False):
        lm = self.lm
        with lm._launch():
            x, z, y = self.d(idx), (self.d(ctx) if lm.n_ctx else None), (self.d(tgt) if tgt is not None else None)
            code = self.lib.kl_rate_window_alts_bulk(
                lm.handle, self.B, self.T, K, None if null_idx else ptr(x), ptr(z), ptr(y), ptr(self.states), ptr(self.a_tprob),
                ptr(self.a_id), ptr(self.a_p), ptr(self.a_rank), ptr(self.bits), ptr(self.status), ptr(self.ws),
                self.n_alts[8] if ws_bytes is None else ws_bytes, lm._stream())
        self.torch.cuda.synchronize()
        return code

    def results(self, K):
        n = self.B * self.T * K
        return (self.a_tprob.cpu().numpy().copy(), self.a_id[:n].cpu().numpy().reshape(self.B, self.T, K).copy(),
                self.a_p[:n].cpu().numpy().reshape(self.B, self.T, K).copy(), self.a_rank.cpu().numpy().copy())


# a subset of test_rate_bulk_gpu.SHAPES: a thin scan, the wide scans, V above 256 (the strided form), the register form
ALTS_SHAPES = [(2, 128, 40, 20, 9, 1), (2, 512, 64, 512, 4, 1), (2, 128, 300, 5, 7, 0), (2, 512, 256, 64, 16, 1)]


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", ALTS_SHAPES)
def test_rate_window_alts_bulk_is_rate_window_bulk_and_forward_window(depth, width, voc, B, T, n_ctx):
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    rng = np.random.default_rng(depth * 1000 + width + voc + B)
    a = AltsBulkAbi(lm, B, T)
    start = (0.1 * rng.standard_normal(tuple(a.states.shape))).astype(np.float32)
    if lm.padded:
        start[:, :, lm.width:] = 0.0      # (zero-padded hidden units carry zeros)
    worst = 0.0
    for win in range(2):
        idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
        a.states.copy_(a.torch.from_numpy(start))
        assert a.forward(idx, ctx) == 0
        full = a.probs.cpu().numpy()
        a.states.copy_(a.torch.from_numpy(start))
        a.bits.zero_()
        assert a.rate(idx, ctx, tgt) == 0
        want_p, want_bits, want_st = a.tprob.cpu().numpy().copy(), a.bits.cpu().numpy().copy(), a.states.cpu().numpy().copy()
        assert not np.array_equal(want_st, start)
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
            assert none.any() and (tp[none] == 0).all() and (ids[none] == -1).all() and (ap[none] == 0).all() and (rk[none] == -1).all()
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


def test_rate_window_alts_bulk_error_paths():
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n_ctx, B, T = 2, 64, 20, 1, 3, 5
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    rng = np.random.default_rng(3)
    a = AltsBulkAbi(lm, B, T)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    h = lm.handle
    size = lm.lib.kl_rate_alts_bulk_workspace_bytes
    assert size(h, 0, T, 3) == 0 == size(h, B, 0, 3) and size(h, B, T, 0) == 0 == size(h, B, T, 9)
    assert a.alts(idx, ctx, tgt, 3) == KL_ERR_STATE                          # split precision: the training forward is bf16's
    lm.prepare(hipabi.KL_PREC_BF16)
    lm.set_window_mode(True)
    try:
        assert a.alts(idx, ctx, tgt, 3) == KL_ERR_STATE                      # one target per window is not rated
    finally:
        lm.set_window_mode(False)
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_alts[3] - 1) == KL_ERR_WORKSPACE
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_ws) == KL_ERR_WORKSPACE     # (the training window alone has no staging area)
    assert a.alts(idx, ctx, tgt, 3, null_idx=True) == KL_ERR_ARG
    assert a.alts(idx, ctx, None, 3) == KL_ERR_ARG
    assert a.alts(idx, ctx, tgt, 0) == KL_ERR_ARG and a.alts(idx, ctx, tgt, 9) == KL_ERR_ARG
    # nothing was launched
    assert (a.a_tprob.cpu().numpy() == -5.0).all() and (a.a_rank.cpu().numpy() == -5).all()
    assert (a.a_id.cpu().numpy() == -5).all() and (a.a_p.cpu().numpy() == -5.0).all()
    assert (a.states.cpu().numpy() == 0).all() and (a.bits.cpu().numpy() == 0).all()
    # the exact size is enough
    assert a.alts(idx, ctx, tgt, 3, ws_bytes=a.n_alts[3]) == 0
    tp, ids, ap, rk = a.results(3)
    assert (tp[tgt >= 0] > 0).all() and (ids[tgt >= 0] >= 0).all()
    with pytest.raises(ValueError):
        lm.rate_window_alts_bulk(idx, ctx, tgt, 9)


# ---------------------------------------------------------------------------------------------- engine
def test_engine_pads_and_groups_streams():
    """600 streams at width 512, T = 4: run as 1024 (HipLM._padded_streams); the engine call equals the ABI call on the
    padded arrays, dummy rows deliver nothing and take no bits"""
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n_ctx, B, T, K = 2, 512, 64, 1, 600, 4, 3
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)      # (rate_window_alts_bulk prepares bf16 by itself)
    Bp = lm._padded_streams(B, T)
    assert Bp == 1024 and lm._stream_groups(B, T) == [(0, B)]
    rng = np.random.default_rng(6)
    idx, ctx, tgt = window_inputs(rng, voc, B, T, n_ctx)
    torch = lm.torch
    lm.reset_states(B)
    got = lm.rate_window_alts_bulk(lm._dev_i32(idx), lm._dev_i32(ctx), lm._dev_i32(tgt), K)
    assert lm.precision == hipabi.KL_PREC_BF16
    assert all(t.is_cuda for t in got)
    assert [tuple(t.shape) for t in got] == [(B, T), (B, T, K), (B, T, K), (B, T)]
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.float32, torch.int32]
    tp, ids, ap, rk = (t.cpu().numpy() for t in got)
    bits = lm.rate_bits_read()
    states = lm.states.cpu().numpy().copy()
    pad = lambda arr, value: np.concatenate([arr, np.full((Bp - B,) + arr.shape[1:], value, dtype=arr.dtype)])
    a = AltsBulkAbi(lm, Bp, T)
    assert a.alts(pad(idx, 0), pad(ctx, 0), pad(tgt, -1), K) == 0
    wtp, wids, wap, wrk = a.results(K)
    assert np.array_equal(ids, wids[:B]) and np.array_equal(rk, wrk[:B])
    assert np.abs(tp - wtp[:B]).max() <= 1e-6 and np.abs(ap - wap[:B]).max() <= 1e-6
    assert (wtp[B:] == 0.0).all() and (wids[B:] == -1).all() and (wap[B:] == 0.0).all() and (wrk[B:] == -1).all()
    assert (a.bits.cpu().numpy()[B:] == 0.0).all()
    assert np.abs(bits - a.bits.cpu().numpy()[:B]).max() <= 1e-12 * np.abs(bits).max()
    assert np.abs(states - a.states.cpu().numpy()[:B]).max() <= 1e-6
    none = tgt < 0
    assert (tp[none] == 0.0).all() and (ids[none] == -1).all() and (rk[none] == -1).all() and (tp[~none] > 0.0).all()
    # the same probabilities as rate_window_bulk through the engine
    lm.reset_states(B)
    plain = lm.rate_window_bulk(lm._dev_i32(idx), lm._dev_i32(ctx), lm._dev_i32(tgt)).cpu().numpy()
    assert np.array_equal(u32(plain), u32(tp)) and np.array_equal(lm.rate_bits_read(), bits)


def test_engine_rate_select_counts_first():
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(8)
    n, K = 3 * BLOCK + 17, 4
    probs, rank, alt_id, alt_p, max_prob, min_rank = select_inputs(rng, n, K, "half")
    up = lambda a: torch.from_numpy(a).to(dev)
    src = [up(probs), up(rank), up(alt_id), up(alt_p)]
    want = ratebulk.select_host(probs, rank, alt_id, alt_p, max_prob, min_rank)
    got = lm.rate_select(*src, max_prob=max_prob, min_rank=min_rank)
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.int64 and got[0].numel() == len(want[0]) > 0
    for g, r in zip(got, want):
        g = g.cpu().numpy()
        assert g.shape == r.shape and np.array_equal(g.view(np.uint8), np.ascontiguousarray(r).view(np.uint8))
    none = lm.rate_select(*src, max_prob=-1.0, min_rank=0)
    assert [tuple(t.shape) for t in none] == [(0,), (0,), (0,), (0, K), (0, K)]
    with pytest.raises(ValueError):
        lm.rate_select(*src, max_prob=0.5, min_rank=-1)
    with pytest.raises(ValueError):
        lm.rate_select(*src, max_prob=float("nan"), min_rank=0)


# ---------------------------------------------------------------------------------------------- Rater
def test_rater_bf16_alternatives_and_suspects():
    """the small rater of test_rate_batch_bf16_matches_the_oracle_rater, its nine texts, two contexts, four streams"""
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = contract_texts()
    k = 3
    dist = oracle_distributions(small_rater(OracleLM), texts, contexts)
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "rate_window_alts_bulk") and hasattr(hip.model, "rate_select")
    hip.model.reset_states(1)
    before = np.asarray(hip.rate(texts[6], contexts[6]), dtype=np.float64)
    probs, bits = hip.rate_batch(texts, contexts, streams=4, precision="bf16")
    rated, bits2 = hip.rate_alternatives(texts, contexts, k=k, streams=4, precision="bf16")
    assert (np.abs(bits2 - bits) <= 1e-12 * np.maximum(1.0, np.abs(bits))).all()
    worst = 0.0
    for i, t in enumerate(texts):
        one, n = rated[i], len(windows.normalize(t))
        assert one.probs.shape == one.rank.shape == (n,) and one.alt_ids.shape == one.alt_probs.shape == (n, k)
        assert one.probs.dtype == one.alt_probs.dtype == np.float32 and one.rank.dtype == one.alt_ids.dtype == np.int32
        assert np.array_equal(u32(one.probs), u32(probs[i])), i
        if n:
            assert one.probs[0] == 1.0 and one.rank[0] == -1 and (one.alt_ids[0] == -1).all() and not one.alt_probs[0].any()
        if n > 1:
            y = windows.encode(windows.normalize(t), hip.mapping[0])[1:]
            worst = max(worst, against_the_oracle(dist[i], y, one.alt_ids[1:], one.alt_probs[1:], one.rank[1:], 1e-2))
            at = np.nonzero(one.rank[1:] < k)[0] + 1
            assert np.array_equal(one.alt_ids[at, one.rank[at]], y[at - 1])
            assert np.array_equal(u32(one.alt_probs[at, one.rank[at]]), u32(one.probs[at]))
    print("max |alt_p(bf16) - oracle| = %.3g" % worst)
    # suspects on the device: the filter of that result, bit for bit
    predicted = sum(max(len(t) - 1, 0) for t in texts)
    counts = []
    for max_prob, min_rank in settings_of(rated):
        found, bits3 = hip.suspects(texts, contexts, k=k, streams=4, max_prob=max_prob, min_rank=min_rank, precision="bf16")
        assert np.array_equal(bits3.view(np.uint64), bits2.view(np.uint64))
        counts.append(same_as_filter(found, rated, max_prob, min_rank))
    assert counts[0] == predicted and counts[1] == 0 and 0 < counts[2] < predicted
    # split precision: the bulk plan through rate_window_alts against rate_alternatives' own plan, the threshold in the widest
    # gap of the probabilities so that no position sits on it
    ref, _ = hip.rate_alternatives(texts, contexts, k=k, streams=4, precision="split")
    flat = np.sort(np.concatenate([r.probs[1:] for r in ref]).astype(np.float64))
    gaps = np.diff(flat)
    g = int(np.argmax(gaps))
    print("widest gap of the sorted probabilities: %.3g" % gaps[g])
    assert gaps[g] >= 1e-4
    max_prob = 0.5 * (flat[g] + flat[g + 1])
    found, _ = hip.suspects(texts, contexts, k=k, streams=4, max_prob=max_prob, min_rank=0, precision="split")
    assert 0 < sum(len(f) for f in found) < predicted
    for one, r in zip(found, ref):
        keep = np.nonzero((r.rank >= 0) & (r.probs <= np.float32(max_prob)))[0]
        assert np.array_equal(one.positions, keep)
        if len(keep):
            assert np.abs(one.probs.astype(np.float64) - r.probs[keep]).max() <= 4e-5
    # afterwards: a freshly reset single row, and a split-precision rate as before the bulk calls
    hip.suspects(texts, contexts, k=k, streams=4, precision="bf16")
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()
    after = np.asarray(hip.rate(texts[6], contexts[6]), dtype=np.float64)
    assert np.abs(after - before).max() < 1e-6
    # nothing but texts without a prediction
    found, b = hip.suspects(["", "a"], precision="bf16")
    assert [len(f) for f in found] == [0, 0] and b.tolist() == [0.0, 0.0]
    rated, b = hip.rate_alternatives(["", "a"], precision="bf16")
    assert [len(r) for r in rated] == [0, 1] and rated[1].probs.tolist() == [1.0] and b.tolist() == [0.0, 0.0]
