"""Corrections on the GPU (run with -m gpu on an MI355X): kl_variant_windows, `HipLM.variant_windows` and `Rater.corrections`.

kl_variant_windows is held to its numpy statement (`ratebulk.variant_windows_host`, itself held to brute force in
test_rate_corrections.py) bit for bit, with a guard band behind every output.  `Rater.corrections(precision="bf16")` is held,
bit for bit, to `lm.rate_window_bulk` on the host statement's windows, uploaded in the same chunks from zero states -- the same
launches on the same inputs --; `precision="split"` to the CPU double within the first-order bound of the project's 2e-5 on a
split-precision probability: |cost - cost_oracle| <= 2 * sum over the scored positions of 2e-5 / (p_oracle * ln 2)."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk, windows
from tests.test_rate_bulk_gpu import device, lib_and_stream
from tests.test_rate_corrections import (SPLIT, decided, gap_threshold, oracle_costs, same_suspects, variant_corpus,
                                         variant_suspects, wide_rater, wide_texts)
from tests.test_rate_suspects_gpu import GUARD, MARK, marked, words
from tests.test_rate_window_gpu import ptr

pytestmark = pytest.mark.gpu

KL_ERR_ARG = 5
SHAPES = [(1, 1, 1, 0, 3), (37, 3, 5, 4, 9), (300, 8, 40, 7, 64)]      # (S, K, left, ahead, T)


def suspects_for(corpus, offsets, S, K):
    """S suspects of the CPU test's kinds; a single one is the last character of the long text (a valid row, nothing after it)"""
    if S == 1:
        pos, alts = variant_suspects(corpus, offsets, K=K)
        at = int(np.nonzero(pos == offsets[7] - 1)[0][0])
        return pos[at:at + 1].copy(), (alts[at:at + 1] % 9 + 1).astype(np.int32)
    return variant_suspects(corpus, offsets, count=S, K=K)


class Variants(object):
    """kl_variant_windows on device copies of host arrays; every output is followed by a guard band and prefilled with the marker"""

    def __init__(self, corpus, offsets, text_ctx, pos, alts, T, R):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        torch = self.torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
        self.src = dict(corpus=up(corpus), offsets=up(offsets), sel_pos=up(pos), sel_alt_id=up(alts),
                        text_ctx=up(text_ctx) if self.n_ctx else None)
        self.n_corpus, self.n_texts, self.S, self.K, self.T = len(corpus), len(offsets) - 1, len(pos), alts.shape[1], T
        rows = self.S * R
        self.sizes = dict(idx=rows * T, ctx=rows * T * self.n_ctx, tgt=rows * T, valid=rows)
        self.fresh()

    def fresh(self):
        self.out = dict((name, marked(self.torch, self.dev, n, self.torch.int32)) for name, n in self.sizes.items())

    def run(self, left, ahead, deletions, shift=None, **override):
        a = dict((name, ptr(t) if t is not None else None) for name, t in self.src.items())
        a.update((name, ptr(t)) for name, t in self.out.items())
        if not self.n_ctx:
            a["ctx"] = None
        a.update(n_corpus=self.n_corpus, n_texts=self.n_texts, n_ctx=self.n_ctx, S=self.S, K=self.K, left=left, ahead=ahead,
                 deletions=deletions, T=self.T)
        a.update(override)
        for name, by in (shift or {}).items():      # (a misaligned pointer)
            a[name] = C.c_void_p(a[name].value + by)
        code = self.lib.kl_variant_windows(a["corpus"], a["n_corpus"], a["offsets"], a["n_texts"], a["text_ctx"], a["n_ctx"],
                                           a["sel_pos"], a["sel_alt_id"], a["S"], a["K"], a["left"], a["ahead"], a["deletions"],
                                           a["T"], a["idx"], a["ctx"], a["tgt"], a["valid"], self.stream)
        self.torch.cuda.synchronize()
        return code

    def results(self):
        return dict((name, words(t)) for name, t in self.out.items())

    def untouched(self):
        return all((w == MARK).all() for w in self.results().values())


# ---------------------------------------------------------------------------------------------- kl_variant_windows
@pytest.mark.parametrize("n_ctx", [0, 2, 3])
@pytest.mark.parametrize("deletions", [0, 1])
@pytest.mark.parametrize("S,K,left,ahead,T", SHAPES)
def test_variant_windows_is_variant_windows_host(S, K, left, ahead, T, deletions, n_ctx):
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = suspects_for(corpus, offsets, S, K)
    assert len(pos) == S and alts.shape == (S, K)
    R = K + 1 + deletions
    want = dict(zip(("idx", "ctx", "tgt", "valid"),
                    ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T)))
    ok = want["valid"].reshape(S, R)
    assert ok.any() and (S == 1 or not ok.all())
    v = Variants(corpus, offsets, text_ctx, pos, alts, T, R)
    runs = []
    for _ in range(2):
        v.fresh()
        assert v.run(left, ahead, deletions) == 0
        got = v.results()
        for name, ref in want.items():
            ref = ref.reshape(-1).view(np.uint32)
            assert got[name].size == ref.size + GUARD
            assert np.array_equal(got[name][:ref.size], ref), name      # every word is written: no marker is left
            assert (got[name][ref.size:] == MARK).all(), name           # ... and nothing behind the output
        runs.append(got)
    assert all(np.array_equal(runs[0][name], runs[1][name]) for name in want)


def test_variant_windows_argument_errors():
    """KL_ERR_ARG before any launch: the outputs keep their markers"""
    S, K, left, ahead, T, n_ctx = 37, 3, 5, 4, 9, 2
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = suspects_for(corpus, offsets, S, K)
    v = Variants(corpus, offsets, text_ctx, pos, alts, T, K + 2)
    names = ("corpus", "offsets", "text_ctx", "sel_pos", "sel_alt_id", "idx", "ctx", "tgt", "valid")
    cases = [{name: None} for name in names]                                    # (text_ctx and ctx: null while n_ctx > 0)
    cases += [dict(S=0), dict(n_texts=0), dict(K=0), dict(K=9), dict(left=0), dict(ahead=-1), dict(T=left + ahead - 1),
              dict(T=1025), dict(n_ctx=-1), dict(n_ctx=9), dict(deletions=-1), dict(deletions=2)]
    cases += [dict(n_corpus=2 ** 40 + 1), dict(S=2 ** 22 // (K + 2) + 1)]      # (beyond what the header allows: more than 2^22 rows)
    cases += [dict(shift={name: 4 if name in ("offsets", "sel_pos") else 2}) for name in names]
    for case in cases:
        assert v.run(**dict(dict(left=left, ahead=ahead, deletions=1), **case)) == KL_ERR_ARG, case
        assert v.untouched(), case
    assert v.run(left, ahead, 1) == 0 and not v.untouched()


def test_engine_variant_windows():
    from tests.test_rate_window_gpu import make_model
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 2)
    S, K, left, ahead, T = 37, 3, 5, 4, 12
    corpus, offsets, text_ctx = variant_corpus(2)
    pos, alts = suspects_for(corpus, offsets, S, K)
    up = lambda a: torch.from_numpy(a).to(dev)
    src = [up(corpus), up(offsets), up(text_ctx), up(pos), up(alts)]
    for deletions in (False, True):
        want = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, int(deletions), T)
        got = lm.variant_windows(*src, left=left, ahead=ahead, deletions=deletions, T=T)
        assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
        for g, r in zip(got, want):
            assert tuple(g.shape) == r.shape and np.array_equal(g.cpu().numpy(), r)
        # a slice of the selection, as `Rater.corrections` passes its chunks; no contexts
        part = lm.variant_windows(src[0], src[1], None, src[3][5:9], src[4][5:9], left, ahead, deletions, T)
        R = K + 1 + int(deletions)
        assert tuple(part[1].shape) == (4 * R, T, 0)
        for g, r in zip((part[0], part[2], part[3]), (want[0], want[2], want[3])):
            assert np.array_equal(g.cpu().numpy(), r[5 * R:9 * R])
    # rate_bits_take_all: every stream's bits at once, the accumulators zeroed
    lm.rate_bits = torch.arange(1, 8, dtype=torch.float64, device=dev)
    taken = lm.rate_bits_take_all()
    assert taken.is_cuda and taken.cpu().numpy().tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert tuple(lm.rate_bits.shape) == (7,) and not lm.rate_bits.cpu().numpy().any()
    assert np.array_equal(lm.rate_bits_read(), np.zeros(7))
    from ocrd_keraslm_amd.lib import hipabi
    with pytest.raises(hipabi.KlError):
        lm.variant_windows(src[0], src[1], src[2], src[3], src[4].to(torch.int64), left, ahead, False, T)
    with pytest.raises(hipabi.KlError):
        lm.variant_windows(*src, left=left, ahead=ahead, deletions=False, T=left + ahead - 1)


# ---------------------------------------------------------------------------------------------- Rater
def global_suspects(rater, texts, found):
    """(corpus, offsets, pos [S], alt_ids [S, k]) of a call's suspects in corpus order"""
    ids = [windows.encode(windows.normalize(t), rater.mapping[0]) for t in texts]
    offsets = np.concatenate([[0], np.cumsum([len(a) for a in ids])]).astype(np.int64)
    pos = np.concatenate([f.positions + offsets[i] for i, f in enumerate(found)])
    return np.concatenate(ids).astype(np.int32), offsets, pos, np.concatenate([f.alt_ids for f in found])


def test_corrections_bf16_is_rate_window_bulk_on_the_host_windows():
    """every predicted character a suspect: first one chunk of more than 512 rows (run as 1024 at width 512), then chunks of 60
    rows with a shorter last one"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    texts = texts + [texts[4][::-1], texts[6][::-1]]
    contexts = contexts + [[175], [190]]
    hip = wide_rater(hip_factory)
    lm = hip.model
    assert hasattr(lm, "variant_windows") and lm.pwidth == 512
    k, left, ahead, deletions = 3, 6, 3, True
    R = k + 2
    T = max(left + ahead, ratebulk.MIN_T)
    text_ctx = np.asarray([windows.clamp_context(c) for c in contexts], dtype=np.int32)
    hip.model.reset_states(1)
    before = np.asarray(hip.rate(texts[4], contexts[4]), dtype=np.float64)
    for streams, min_gain in ((1024, 0.5), (64, -np.inf)):
        args = dict(k=k, streams=streams, max_prob=1.0, min_rank=0, precision="bf16")
        found, bits = hip.corrections(texts, contexts, left=left, ahead=ahead, deletions=deletions, min_gain=min_gain, **args)
        assert lm.states.shape[0] == 1 and not lm.states.cpu().numpy().any()
        want, want_bits = hip.suspects(texts, contexts, **args)
        assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
        same_suspects(found, want)
        corpus, offsets, pos, alts = global_suspects(hip, texts, found)
        S = len(pos)
        assert S == sum(max(len(t) - 1, 0) for t in texts)
        chunk = max(1, streams // R)
        assert (S * R > 512 and chunk >= S) if streams == 1024 else (S > chunk and S % chunk)
        cost, valid = [], []
        for a in range(0, S, chunk):
            x, z, y, ok = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos[a:a + chunk], alts[a:a + chunk], left,
                                                        ahead, 1, T)
            lm.reset_states(len(x))
            lm.rate_bits_read(reset=True)
            lm.rate_window_bulk(x, z, y, want_probs=False)
            cost.append(lm.rate_bits_read(reset=True))
            valid.append(ok)
        cost, valid = np.concatenate(cost).reshape(S, R), np.concatenate(valid).reshape(S, R)
        assert (cost[valid == 0] == 0.0).all() and (cost[valid == 1] > 0.0).all()      # (a dummy stream takes no bits)
        cost, best, gain = ratebulk.variant_pick_host(cost, valid)
        got = np.concatenate([f.cost for f in found])
        assert got.shape == (S, R) and np.array_equal(got.view(np.uint64), cost.view(np.uint64))
        best_id = np.where(best == 0, -1, np.where(best == k + 1, -2, alts[np.arange(S), np.clip(best - 1, 0, k - 1)]))
        drop = (best == 0) | ~(gain >= min_gain)
        best_id[drop], gain[drop] = -1, 0.0
        assert np.array_equal(np.concatenate([f.best_id for f in found]), best_id)
        assert np.array_equal(np.concatenate([f.gain for f in found]).view(np.uint64), gain.view(np.uint64))
        assert (best_id >= 0).any() and ((best_id == -1).any() or min_gain == -np.inf)
        lm.reset_states(1)
    # afterwards: a split-precision rate as before the bulk calls
    after = np.asarray(hip.rate(texts[4], contexts[4]), dtype=np.float64)
    assert np.abs(after - before).max() < 1e-6
    # nothing but texts without a prediction; no suspects
    for some, kw in ((["", "a"], {}), (texts[:5], dict(max_prob=0.0))):
        found, b = hip.corrections(some, k=k, deletions=True, **kw)
        assert [len(f) for f in found] == [0] * len(some)
        assert all(f.cost.shape == (0, R) and f.best_id.dtype == np.int32 and f.gain.dtype == np.float64 for f in found)


def test_corrections_split_against_the_double():
    """the texts, seed and settings test_split_contract_texts_keep_the_oracle_within_the_cap checks on the CPU.  The double's
    costs are taken over the HIP run's own suspects and alternatives (the same hypotheses on both sides); that the double's
    rater finds the same suspects is asserted apart from that.
    Measured on an MI355X: 18 suspects, none too close to call, largest |cost - cost_oracle| 0.0055 of its bound."""
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    oracle = wide_rater(OracleLM)
    hip = wide_rater(hip_factory)
    rated, _ = oracle.rate_alternatives(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"])
    max_prob, gap = gap_threshold(np.concatenate([r.probs[1:] for r in rated]))
    assert gap >= 1e-4
    found, bits = hip.corrections(texts, contexts, max_prob=max_prob, precision="split", **SPLIT)
    from ocrd_keraslm_amd.lib import hipabi
    assert hip.model.precision == hipabi.KL_PREC_SPLIT and hip.model.states.shape[0] == 1
    want, want_bits = hip.suspects(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"], max_prob=max_prob,
                                   min_rank=SPLIT["min_rank"], precision="split")
    same_suspects(found, want)
    assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
    ref, _ = oracle.corrections(texts, contexts, max_prob=max_prob, precision="split", **SPLIT)
    total = sum(len(f) for f in found)
    assert total >= 10
    for one, r in zip(found, ref):
        assert np.array_equal(one.positions, r.positions)
    costs = oracle_costs(oracle, texts, contexts, found, SPLIT["left"], SPLIT["ahead"], SPLIT["deletions"])
    k = SPLIT["k"]
    worst, open_ = 0.0, 0
    for one, (cost, bound) in zip(found, costs):
        assert np.array_equal(np.isinf(one.cost), np.isinf(cost))
        fin = np.isfinite(cost)
        if fin.any():
            ratio = np.abs(one.cost[fin] - cost[fin]) / bound[fin]
            worst = max(worst, float(ratio.max()))
        sure = decided(cost, bound)
        open_ += int((~sure).sum())
        _, best, _ = ratebulk.variant_pick_host(cost, fin)
        _, got, _ = ratebulk.variant_pick_host(one.cost, np.isfinite(one.cost))
        assert np.array_equal(got[sure], best[sure])
        # what the call returned follows from its own costs (min_gain 0.0: a proposal that does not read worse)
        _, b, g = ratebulk.variant_pick_host(one.cost, np.isfinite(one.cost))
        keep = (b > 0) & (g >= SPLIT["min_gain"])
        ids = np.where(b == k + 1, -2, one.alt_ids[np.arange(len(one)), np.clip(b - 1, 0, k - 1)]) if len(one) else b
        assert np.array_equal(one.best_id, np.where(keep, ids, -1)) and np.array_equal(one.gain, np.where(keep, g, 0.0))
    print("suspects %d, too close to call %d, max |cost - cost_oracle| / bound = %.3g" % (total, open_, worst))
    assert open_ <= 0.1 * total
    assert worst <= 1.0, worst
