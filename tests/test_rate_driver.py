"""The corpus-order driver of `Rater` (`_rate_in_corpus_order`) and what hangs on it -- `rate_batch(precision="bf16")`,
`rate_alternatives(precision="bf16")`, `suspects`, `corrections` -- on the CPU.

`HostLM` is the oracle-backed engine double with the device-side calls the driver uses, each written ONLY from the numpy
statements the project already has (ratebulk.windows_host, scatter_host, scatter_alts_host, text_bits_host, select_host,
variant_windows_host, ratebatch.alternatives_of and bits_of) over CPU torch tensors: a Rater on it takes the device path,
a Rater on plain OracleLM the fallbacks.  Both are f64 numpy over different batch compositions, rounded to f32 where the
device delivers f32: probabilities may differ by rounding (rtol 2**-22, two f32 ulps), bits and costs are f64 sums of at most
a few hundred terms (rtol 1e-12), everything discrete is equal.  HostLM sums a stream's bits over the unrounded f64
probabilities, as the fallback of `corrections` sums its costs.

The seed, max_prob and min_gain are chosen so that no decision of the run is a near-tie; `margins` asserts that on the
fallback's output, so another seed that breaks it fails loudly instead of flaking."""
import numpy as np
import pytest
import torch

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import Rater, ratebatch, ratebulk
from tests.oracle_engine import OracleLM

ALPHABET = "abcdefghij"      # V = 11 with the unmapped id 0
LENGTH = 8
SIZES = (0, 1, 2, 5, 10, 12, 13, 17, 20, 3 * LENGTH)      # six texts of several windows on four rows: rows are reused
STREAMS = 4
SEED = 5
MAX_PROB, MIN_RANK, MIN_GAIN = 0.05, 1, 1.0
SCALE = 3.0          # all weights of the seeded model times this: peaked distributions, gains of several bits
LEFT, AHEAD = 5, 3
P_RTOL, F64_RTOL = 2.0 ** -22, 1e-12


def _a(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class HostLM(OracleLM):
    """OracleLM plus HipLM's device-side rating calls on CPU tensors, each one the project's own numpy statement"""
    torch = torch
    device = torch.device("cpu")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.rate_bits = None
        self.seen = {"B": set(), "reset_where": 0, "calls": set()}

    def reset_states_where(self, mask_d):
        self.seen["reset_where"] += 1
        for s in self.states:
            s[_a(mask_d)] = 0

    def assemble_windows(self, corpus, plan, T, n_ctx):
        assert plan.shape[1] == 4 + n_ctx
        return tuple(_t(a) for a in ratebulk.windows_host(_a(corpus), _a(plan), T))

    def _rate(self, name, idx, ctx, tgt, k):
        x, y = _a(idx), _a(tgt)
        self.seen["B"].add(len(x))
        self.seen["calls"].add(name)
        tprob, alt_id, alt_p, rank = ratebatch.alternatives_of(self.forward_window(x, _a(ctx)), y, k)
        if self.rate_bits is None or len(self.rate_bits) != len(x):
            self.rate_bits = np.zeros(len(x), dtype=np.float64)
        for b in range(len(x)):      # (bits_of skips a first character: a 1.0 in front of the row's valid positions)
            self.rate_bits[b] += ratebatch.bits_of(np.concatenate([[1.0], tprob[b][y[b] >= 0]]))
        return _t(tprob.astype(np.float32)), _t(alt_id), _t(alt_p.astype(np.float32)), _t(rank)

    def rate_window(self, idx, ctx, tgt, want_probs=True):
        p = self._rate("rate_window", idx, ctx, tgt, 1)[0]
        return p if want_probs else None

    def rate_window_bulk(self, idx, ctx, tgt, want_probs=True):
        p = self._rate("rate_window_bulk", idx, ctx, tgt, 1)[0]
        return p if want_probs else None

    def rate_window_alts(self, idx, ctx, tgt, k):
        return self._rate("rate_window_alts", idx, ctx, tgt, k)

    def rate_window_alts_bulk(self, idx, ctx, tgt, k):
        return self._rate("rate_window_alts_bulk", idx, ctx, tgt, k)

    def rate_scatter(self, tprob, plan, n_ctx, out):
        self.seen["calls"].add("rate_scatter")
        ratebulk.scatter_host(_a(tprob), _a(plan), out.numpy())      # (in place: the array shares the tensor's memory)
        return out

    def rate_scatter_alts(self, tprob, rank, alt_id, alt_p, plan, n_ctx, out_prob, out_rank, out_alt_id, out_alt_p):
        self.seen["calls"].add("rate_scatter_alts")
        ratebulk.scatter_alts_host(_a(tprob), _a(rank), _a(alt_id), _a(alt_p), _a(plan), out_prob.numpy(), out_rank.numpy(),
                                   out_alt_id.numpy(), out_alt_p.numpy())

    def rate_text_bits(self, probs, offsets):
        return _t(ratebulk.text_bits_host(_a(probs), _a(offsets)))

    def rate_select(self, probs, rank, alt_id, alt_p, max_prob, min_rank):
        return tuple(_t(a) for a in ratebulk.select_host(_a(probs), _a(rank), _a(alt_id), _a(alt_p), max_prob, min_rank))

    def variant_windows(self, corpus_d, offsets_d, text_ctx_d, sel_pos_d, sel_alt_id_d, left, ahead, deletions, T,
                        insertions=False):
        return tuple(_t(a) for a in ratebulk.variant_windows_host(
            _a(corpus_d), _a(offsets_d), None if text_ctx_d is None else _a(text_ctx_d), _a(sel_pos_d), _a(sel_alt_id_d),
            left, ahead, deletions, T, int(insertions)))

    def rate_bits_take_all(self):
        out = _t(self.rate_bits.copy())
        self.rate_bits[:] = 0
        return out

    def rate_bits_take(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        out = _t(self.rate_bits[rows])
        self.rate_bits[rows] = 0
        return out

    def rate_bits_read(self, reset=True):
        v = np.zeros(0, dtype=np.float64) if self.rate_bits is None else self.rate_bits.copy()
        if reset and self.rate_bits is not None:
            self.rate_bits[:] = 0
        return v

    def rate_status_check(self):
        pass


class RecordingLM(OracleLM):
    """plain OracleLM (the fallbacks) that keeps every distribution it delivered, for `margins`"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.delivered = []

    def forward_window(self, idx, ctx, tgt=None, want_probs=True):
        probs = super().forward_window(idx, ctx, tgt, want_probs)
        if probs is not None:
            self.delivered.append(np.array(probs))
        return probs


def rater_on(factory, n_ctx):
    """depth 2 / width 16 over ten characters (V = 11), windows of 8"""
    r = Rater(engine_factory=factory)
    r.width, r.depth, r.length, r.n_ctx = 16, 2, LENGTH, n_ctx
    r.stateful = True
    r.mapping = (dict((c, i) for i, c in enumerate(ALPHABET, 1)), dict((i, c) for i, c in enumerate(ALPHABET, 1)))
    r.voc_size = len(ALPHABET) + 1
    r.configure()
    w = O.init_weights(O.ModelConfig(2, 16, r.voc_size, n_ctx), seed=SEED, emb_std=0.3, dtype=np.float32)
    r.model.set_weights(dict((name, SCALE * a) for name, a in w.items()), 3)
    r.status = 2
    return r


def corpus(n_ctx):
    rng = np.random.default_rng(SEED)
    texts = ["".join(ALPHABET[int(c)] for c in rng.integers(0, len(ALPHABET), size)) for size in SIZES]
    contexts = [[171 if i % 2 else 185, 3 + i][:n_ctx] for i in range(len(texts))] if n_ctx else None
    return texts, contexts


@pytest.fixture(scope="module", params=[0, 2], ids=["n_ctx0", "n_ctx2"])
def pair(request):
    """(n_ctx, fallback rater on OracleLM, device-path rater on HostLM, texts, contexts)"""
    n_ctx = request.param
    texts, contexts = corpus(n_ctx)
    return n_ctx, rater_on(RecordingLM, n_ctx), rater_on(HostLM, n_ctx), texts, contexts


def margins(ref, rated=None, found=None):
    """the three conditions on the inputs, on the fallback's output: no two logits of a position within 1e-9, no probability
    within relative 1e-5 of max_prob, no gain within 1e-9 of min_gain"""
    for full in ref.model.delivered:
        logits = np.sort(np.log(full), axis=-1)
        assert np.diff(logits, axis=-1).min() > 1e-9, "two logits of a position tie: choose another seed"
    ref.model.delivered = []
    for one in rated or ():
        assert (np.abs(one.probs.astype(np.float64) - MAX_PROB) > 1e-5 * MAX_PROB).all(), "a probability at max_prob"
    for one in found or ():
        with np.errstate(invalid="ignore"):
            gains = one.cost[:, :1] - one.cost[:, 1:]
        gains = gains[np.isfinite(gains)]
        assert (np.abs(gains - MIN_GAIN) > 1e-9).all(), "a gain at min_gain"


def same_bits(got, want):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=F64_RTOL, atol=0)


def same_rated(got, want, names):
    """probabilities within rounding, everything else equal"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for name in names:
            a, b = getattr(g, name), getattr(w, name)
            assert a.dtype == b.dtype and a.shape == b.shape, name
            if name in ("probs", "alt_probs"):
                np.testing.assert_allclose(a, b, rtol=P_RTOL, atol=0, err_msg=name)
            elif name in ("cost", "gain"):
                np.testing.assert_allclose(a, b, rtol=F64_RTOL, atol=0, err_msg=name)      # (+inf == +inf: no such variant)
            else:
                assert np.array_equal(a, b), name


def test_rate_batch(pair):
    n_ctx, ref, dev, texts, contexts = pair
    want, want_bits = ref.rate_batch(texts, contexts, streams=STREAMS, precision="bf16")
    margins(ref)
    got, got_bits = dev.rate_batch(texts, contexts, streams=STREAMS, precision="bf16")
    # (the driver ran, with target-only delivery: rows reused, more than one batch size)
    seen = dev.model.seen
    assert seen["calls"] == {"rate_window_bulk", "rate_scatter"} and seen["reset_where"] > 0 and len(seen["B"]) > 1
    assert len(got) == len(want) == len(texts)
    for g, w, t in zip(got, want, texts):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape == (len(t),)
        np.testing.assert_allclose(g, w, rtol=P_RTOL, atol=0)
    same_bits(got_bits, want_bits)
    none, only_bits = dev.rate_batch(texts, contexts, streams=STREAMS, want_probs=False, precision="bf16")
    assert none is None
    same_bits(only_bits, want_bits)
    assert dev.model.states[0].shape[0] == 1      # (a freshly reset single row)


@pytest.mark.parametrize("k", [1, 3])
def test_rate_alternatives(pair, k):
    n_ctx, ref, dev, texts, contexts = pair
    want, want_bits = ref.rate_alternatives(texts, contexts, k=k, streams=STREAMS, precision="bf16")
    margins(ref)
    dev.model.seen["calls"].clear()
    got, got_bits = dev.rate_alternatives(texts, contexts, k=k, streams=STREAMS, precision="bf16")
    assert dev.model.seen["calls"] == {"rate_window_alts_bulk", "rate_scatter_alts"}
    same_rated(got, want, ("probs", "rank", "alt_ids", "alt_probs"))
    same_bits(got_bits, want_bits)
    # rate_batch(precision="bf16") delivers the same probabilities, bit for bit
    probs = dev.rate_batch(texts, contexts, streams=STREAMS, precision="bf16")[0]
    assert all(np.array_equal(p, g.probs) for p, g in zip(probs, got))


@pytest.mark.parametrize("precision", ["bf16", "split"])
@pytest.mark.parametrize("k", [1, 3])
def test_suspects(pair, k, precision):
    n_ctx, ref, dev, texts, contexts = pair
    rated = ref.rate_alternatives(texts, contexts, k=k, streams=STREAMS, precision=precision)[0]
    want, want_bits = ref.suspects(texts, contexts, k=k, streams=STREAMS, max_prob=MAX_PROB, min_rank=MIN_RANK,
                                   precision=precision)
    margins(ref, rated)
    got, got_bits = dev.suspects(texts, contexts, k=k, streams=STREAMS, max_prob=MAX_PROB, min_rank=MIN_RANK,
                                 precision=precision)
    assert 0 < sum(len(w) for w in want) < sum(max(len(t) - 1, 0) for t in texts)      # (some suspects, not everything)
    same_rated(got, want, ("positions", "probs", "rank", "alt_ids", "alt_probs"))
    same_bits(got_bits, want_bits)


@pytest.mark.parametrize("precision", ["bf16", "split"])
@pytest.mark.parametrize("k", [1, 3])
def test_corrections(pair, k, precision):
    n_ctx, ref, dev, texts, contexts = pair
    kwargs = dict(k=k, streams=STREAMS, max_prob=MAX_PROB, min_rank=MIN_RANK, left=LEFT, ahead=AHEAD, deletions=True,
                  min_gain=MIN_GAIN, precision=precision, insertions=True)
    rated = ref.rate_alternatives(texts, contexts, k=k, streams=STREAMS, precision=precision)[0]
    want, want_bits = ref.corrections(texts, contexts, **kwargs)
    margins(ref, rated, want)
    got, got_bits = dev.corrections(texts, contexts, **kwargs)
    ops = np.concatenate([w.best_op for w in want])
    assert (ops != ratebatch.Corrections.OP_NONE).any() and (ops == ratebatch.Corrections.OP_NONE).any()
    same_rated(got, want, ("positions", "probs", "rank", "alt_ids", "alt_probs", "cost", "best_id", "gain", "best_op"))
    same_bits(got_bits, want_bits)


def test_no_predictions(pair):
    """nothing but empty texts and single characters: every caller's early return"""
    n_ctx, ref, dev, texts, contexts = pair
    texts = ["", "a", ""]
    for r in (ref, dev):
        probs, bits = r.rate_batch(texts, None, streams=STREAMS, precision="bf16")
        assert [p.tolist() for p in probs] == [[], [1.0], []] and not bits.any()
        rated, bits = r.rate_alternatives(texts, None, k=3, streams=STREAMS, precision="bf16")
        assert [len(one.probs) for one in rated] == [0, 1, 0] and rated[1].rank.tolist() == [-1] and not bits.any()
        for found, bits in (r.suspects(texts, None, streams=STREAMS), r.corrections(texts, None, streams=STREAMS)):
            assert [len(f) for f in found] == [0, 0, 0] and not bits.any()
    ref.model.delivered = []


@pytest.mark.parametrize("k", [0, 3])
def test_plan_loop_split(pair, k):
    """the other loop, `_run_plan` over a ratebatch.Plan (precision="split"): its device branch -- rate_window(_alts), a text's
    bits taken from its row's sum where it ends -- against its fallback branch.  HostLM's sums are over unrounded f64
    probabilities, the fallback's over the f32 it returns: rounding p by at most 2**-24 relative moves log2(p) by at most
    2**-24 / ln 2 < 2**-23, so the bits of a text of m predictions agree within m * 2**-23."""
    n_ctx, ref, dev, texts, contexts = pair
    rate = (lambda r: r.rate_alternatives(texts, contexts, k=k, streams=STREAMS)) if k else (
        lambda r: r.rate_batch(texts, contexts, streams=STREAMS))
    want, want_bits = rate(ref)
    margins(ref)
    dev.model.seen["calls"].clear()
    got, got_bits = rate(dev)
    assert dev.model.seen["calls"] == {"rate_window_alts" if k else "rate_window"}
    if k:
        same_rated(got, want, ("probs", "rank", "alt_ids", "alt_probs"))
    else:
        for g, w in zip(got, want):
            assert g.dtype == w.dtype == np.float32 and g.shape == w.shape
            np.testing.assert_allclose(g, w, rtol=P_RTOL, atol=0)
    preds = np.array([max(len(t) - 1, 0) for t in texts], dtype=np.float64)
    assert (np.abs(got_bits - want_bits) <= preds * 2.0 ** -23).all()
