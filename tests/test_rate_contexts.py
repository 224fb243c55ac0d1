"""Rating under candidate contexts on the CPU: `ratebulk.plan_candidates`, the numpy statements `scatter_planes_host` and
`context_mix_host`, `Rater.rate_contexts` -- its fallback on the oracle-backed engine double and its device path on a HostLM
with the two device calls written ONLY from those statements -- and `keraslm-rate contexts`.

`context_mix_host` is held to an independent statement in exact rational arithmetic: with pi_c the prior and q_c[j] the
floored probabilities, the mixture's probability of character j is
    r[j] = sum_c pi_c prod_{j' <= j} q_c[j'] / sum_c pi_c prod_{j' < j} q_c[j'],
the posterior is pi_c prod_j q_c[j] normalised, and the r[j] telescope: prod_j r[j] = sum_c pi_c 2**-bits_c / sum_c pi_c.
The device kernels are held to the same statements in test_rate_contexts_gpu.py."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import random_text, small_rater
from tests.test_rate_driver import F64_RTOL, P_RTOL, HostLM, _a, _t, rater_on
from tests.test_rate_suspects import LENGTH, contract_texts

STREAMS = 4


class HostCtxLM(HostLM):
    """HostLM plus the two device calls of rating under candidate contexts, each one the numpy statement"""

    def rate_scatter_planes(self, tprob, plan, plane, n_ctx, out):
        self.seen["calls"].add("rate_scatter_planes")
        assert plan.shape[1] == 4 + n_ctx
        ratebulk.scatter_planes_host(_a(tprob), _a(plan), _a(plane), out.numpy())      # (in place)
        return out

    def context_mix(self, planes, offsets, log2prior=None, mix=None):
        self.seen["calls"].add("context_mix")
        self.seen["mixes"] = self.seen.get("mixes", 0) + 1
        return tuple(_t(a) for a in ratebulk.context_mix_host(_a(planes), _a(offsets), None if log2prior is None else _a(log2prior),
                                                               None if mix is None else mix.numpy()))


# ---------------------------------------------------------------------------------------------- plan_candidates
@pytest.mark.parametrize("seed", range(6))
def test_plan_candidates_covers_every_pair_once(seed):
    rng = np.random.default_rng(seed)
    for _ in range(8):
        n, C = int(rng.integers(1, 12)), int(rng.integers(1, 6))
        length, streams = int(rng.integers(3, 10)), int(rng.integers(1, 9))
        sizes = rng.integers(0, 4 * length, n)
        cand = [[int(v) for v in rng.integers(0, 200, 2)] for _ in range(C)]
        plan, planes = ratebulk.plan_candidates(sizes, cand, length, streams)
        assert np.array_equal(plan.sizes, sizes) and plan.total == sizes.sum() and plan.n_ctx == 2
        assert len(planes) == plan.n_calls and len(plan.row) == n * C
        total = plan.total
        cover = np.zeros((C, total + 1), dtype=np.int64)
        text_of = np.repeat(np.arange(n), sizes)
        owner = None      # per row: the (text, candidate, next position) it is working on
        for call, plane in zip(plan.calls, planes):
            assert call.B <= streams and plane.dtype == np.int32 and plane.shape == (call.B,)
            if owner is None or len(owner) != call.B:
                assert call.reset.all()      # (another number of rows: every row starts from zero)
                owner = [None] * call.B
            for b in range(call.B):
                start, vlen = int(call.rows[b, 0]), int(call.rows[b, 1])
                if vlen <= 0:
                    assert plane[b] == -1
                    owner[b] = None
                    continue
                c = int(plane[b])
                assert 0 <= c < C and call.rows[b, 4:].tolist() == cand[c] and 0 < vlen <= call.T
                i = int(text_of[start])
                assert text_of[start + vlen] == i      # (the window and its last target lie in one text)
                if call.reset[b]:
                    assert start == plan.offsets[i]      # a new virtual text begins at a call boundary, from a zero state
                else:
                    assert owner[b] == (i, c, start)     # ... and otherwise the row goes on where it stopped
                owner[b] = (i, c, start + vlen)
                cover[c, start + 1:start + 1 + vlen] += 1
        want = np.ones(total + 1, dtype=np.int64)
        want[plan.offsets] = 0      # (first characters, and the end)
        assert (cover == want[None, :]).all()


def test_plan_candidates_with_one_candidate_is_plan():
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 40, 13)
    for streams in (1, 4, 64):
        got, planes = ratebulk.plan_candidates(sizes, [[171, 5]], 8, streams)
        want = ratebulk.plan(sizes, [[171, 5]] * len(sizes), 8, streams)
        assert got.n_calls == want.n_calls > 0
        for a, b, plane in zip(got.calls, want.calls, planes):
            assert a.T == b.T and np.array_equal(a.rows, b.rows) and np.array_equal(a.reset, b.reset)
            assert np.array_equal(plane, np.where(b.rows[:, 1] > 0, 0, -1))
        assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.row, want.row)
    for bad in ([], [[1]] * 257):
        with pytest.raises(ValueError):
            ratebulk.plan_candidates(sizes, bad, 8, 4)


def test_documented_constants_agree():
    """the most candidates: header, binding and plan"""
    import os
    import re
    from ocrd_keraslm_amd.lib import hipabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "keraslm_hip.h")).read()
    assert [int(v) for v in re.findall(r"^#define KL_CTX_CAND_MAX (\d+)$", text, flags=re.M)] == [hipabi.KL_CTX_CAND_MAX]
    assert hipabi.KL_CTX_CAND_MAX == ratebulk.CTX_CAND_MAX == 256 and ratebulk.PLANE_BYTES == 1 << 30


def test_text_chunks():
    assert ratebulk.text_chunks([5, 5, 5, 20, 1, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 6)]
    assert ratebulk.text_chunks([], 10) == [] and ratebulk.text_chunks([0, 0], 1) == [(0, 2)]
    assert ratebulk.text_chunks([7], 3) == [(0, 1)]


# ---------------------------------------------------------------------------------------------- the numpy statements
def test_scatter_planes_host_against_a_loop():
    rng = np.random.default_rng(1)
    B, T, C, n_ctx = 9, 5, 3, 1
    tprob = rng.random((B, T)).astype(np.float32)
    rows = np.zeros((B, 4 + n_ctx), dtype=np.int64)
    rows[:, 0] = (np.arange(B) // C) * (T + 2) + 1      # (rows of different planes share their positions)
    rows[:, 1] = [0, 1, T, T + 3, -2, T, 2, T, T]
    plane = np.array([0, 1, 2, 0, 1, 2, -1, C, 1], dtype=np.int32)
    ld = int(rows[-1, 0]) + 1 + T + 4
    n_out = int(rows[-1, 0]) + 1 + T // 2               # the last row ends beyond n_out
    out = np.full((C, ld), -5.0, dtype=np.float32)
    assert ratebulk.scatter_planes_host(tprob, rows, plane, out, n_out) is out
    want = np.full((C, ld), -5.0, dtype=np.float32)
    for b in range(B):
        for t in range(T):
            g = int(rows[b, 0]) + 1 + t
            if t < rows[b, 1] and 0 <= plane[b] < C and g < n_out:
                want[plane[b], g] = tprob[b, t]
    assert np.array_equal(out, want)
    assert (out[:, n_out:] == -5.0).all() and (out != -5.0).sum() == 1 + T + T + T + T // 2
    # one plane: scatter_host
    one = ratebulk.scatter_planes_host(tprob, rows, np.zeros(B, dtype=np.int32), np.full((1, ld), -5.0, dtype=np.float32))
    assert np.array_equal(one[0], ratebulk.scatter_host(tprob, rows, np.full(ld, -5.0, dtype=np.float32)))


def exact_mix(planes, offsets, prior):
    """the independent statement, in fractions: per text (r [m] floats, post [C] floats, bits [C], lw [C] exact log2 weights)"""
    C = planes.shape[0]
    out = []
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]) + 1, int(offsets[i + 1])
        w = [Fraction(p) for p in prior]
        r = []
        for j in range(a, b):
            q = [Fraction(float(np.fmax(np.float64(planes[c, j]), 1e-99))) for c in range(C)]
            below = sum(w)
            w = [wc * qc for wc, qc in zip(w, q)]
            r.append(sum(w) / below)
        log2 = lambda f: math.log2(f.numerator) - math.log2(f.denominator) if f else -math.inf
        bits = [-(log2(wc) - log2(Fraction(p))) if p else None for wc, p in zip(w, prior)]
        out.append(([float(x) for x in r], [float(wc / sum(w)) for wc in w], bits, [log2(wc) for wc in w]))
    return out


@pytest.mark.parametrize("C", [1, 2, 5])
def test_context_mix_host_against_fractions(C):
    rng = np.random.default_rng(10 + C)
    sizes = [0, 1, 2, 9, 17, 0, 5]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    planes = (rng.random((C, n + 3)) ** 4 * np.linspace(0.5, 1.0, C)[:, None]).astype(np.float32)
    for weights in (None, rng.random(C) + 0.1):
        prior = np.ones(C) if weights is None else weights
        mix = np.full(n + 3, 7.0, dtype=np.float32)
        log2prior = None if weights is None else np.log2(weights / weights.sum())
        cand_bits, mix_bits, post, best, margin = ratebulk.context_mix_host(planes, offsets, log2prior, mix)
        assert cand_bits.shape == post.shape == (len(sizes), C) and best.dtype == np.int32
        written = np.zeros(n + 3, dtype=bool)
        for i, (r, p, bits, lw) in enumerate(exact_mix(planes, offsets, [float(x) for x in prior])):
            a, b = int(offsets[i]) + 1, int(offsets[i + 1])
            written[a:b] = True
            np.testing.assert_allclose(mix[a:b], np.asarray(r, dtype=np.float64), rtol=2.0 ** -23, atol=0)
            np.testing.assert_allclose(cand_bits[i], bits, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(post[i], p, rtol=1e-10, atol=0)
            assert abs(post[i].sum() - 1.0) < 1e-12
            assert abs(mix_bits[i] + sum(math.log2(x) for x in r)) <= 1e-12 * max(1.0, abs(mix_bits[i]))
            # the telescoping identity, as a log-sum-exp over the candidates
            lp = np.log2(prior / prior.sum()) - cand_bits[i]
            lse = lp.max() + np.log2(np.exp2(lp - lp.max()).sum())
            assert abs(mix_bits[i] + lse) <= 1e-11 * max(1.0, abs(mix_bits[i]))
            order = np.argsort(-np.asarray(lw), kind="stable")
            assert best[i] == order[0]
            if C == 1:
                assert margin[i] == np.inf and post[i, 0] == 1.0
                assert np.array_equal(mix[a:b].view(np.uint32), planes[0, a:b].view(np.uint32))      # the plane, bit for bit
            else:
                assert abs(margin[i] - (lw[order[0]] - lw[order[1]])) <= 1e-11 * max(1.0, abs(lw[order[0]]))
            if b <= a:      # a text of 0 or 1 characters returns the prior
                np.testing.assert_allclose(post[i], prior / prior.sum(), rtol=1e-15)
                assert mix_bits[i] == 0.0 and not cand_bits[i].any()
        assert (mix[~written] == 7.0).all() and (mix[written] != 7.0).all()
        # mix is optional
        again = ratebulk.context_mix_host(planes, offsets, log2prior, None)
        assert all(np.array_equal(x, y) for x, y in zip(again, (cand_bits, mix_bits, post, best, margin)))


def test_context_mix_host_edges():
    rng = np.random.default_rng(2)
    offsets = np.array([0, 12], dtype=np.int64)
    base = (rng.random(12) ** 2).astype(np.float32)
    worse = (base * np.float32(0.5)).astype(np.float32)
    # duplicate planes tie exactly and the smaller index wins
    cand_bits, mix_bits, post, best, margin = ratebulk.context_mix_host(np.stack([worse, base, base]), offsets)
    assert best[0] == 1 and margin[0] == 0.0 and cand_bits[0, 1] == cand_bits[0, 2] and post[0, 1] == post[0, 2]
    assert abs(cand_bits[0, 0] - cand_bits[0, 1] - 11.0) < 1e-9      # (eleven predictions at half the probability)
    # a -inf prior entry is never best, takes no posterior and leaves the mixture alone -- its bits are still delivered
    mix = np.ones(12, dtype=np.float32)
    got = ratebulk.context_mix_host(np.stack([base, worse]), offsets, np.array([-np.inf, 0.0]), mix)
    assert got[3][0] == 1 and got[2][0].tolist() == [0.0, 1.0] and got[4][0] == np.inf
    assert np.array_equal(mix[1:], worse[1:]) and got[1][0] == got[0][0, 1] and got[0][0, 0] == cand_bits[0, 1]
    # a zero and a NaN probability count as 1e-99
    holes = base.copy()
    holes[3], holes[7] = 0.0, np.nan
    floor = base.astype(np.float64)
    floor[[3, 7]] = 1e-99
    mix = np.ones(12, dtype=np.float32)
    got = ratebulk.context_mix_host(holes[None, :], offsets, None, mix)
    assert abs(got[0][0, 0] + np.log2(floor[1:]).sum()) <= 1e-12 * got[0][0, 0] and got[0][0, 0] > 2 * 328.0
    assert mix[3] == 0.0 and mix[7] == 0.0 and np.array_equal(np.delete(mix, [0, 3, 7]), np.delete(base, [0, 3, 7]))
    # without a finite prior entry (the caller's promise broken): NaN where the weights are used
    got = ratebulk.context_mix_host(np.stack([base, worse]), offsets, np.array([-np.inf, -np.inf]))
    assert np.isnan(got[1][0]) and np.isnan(got[2][0]).all() and got[3][0] == 0 and got[4][0] == np.inf
    assert np.isfinite(got[0]).all()


# ---------------------------------------------------------------------------------------------- the Rater on the double
CANDIDATES = [[171], [185], [0]]


@pytest.fixture(scope="module")
def fallback():
    """small_rater on OracleLM over the contract texts: (rater, texts, rate_contexts' result, rate_batch per candidate)"""
    r = small_rater(OracleLM, length=LENGTH)
    texts, _ = contract_texts()
    found = r.rate_contexts(texts, CANDIDATES, streams=STREAMS, precision="split")
    per = [r.rate_batch(texts, c, streams=STREAMS) for c in CANDIDATES]
    return r, texts, found, per


def test_rate_contexts_fallback_is_rate_batch_per_candidate(fallback):
    r, texts, found, per = fallback
    assert len(found) == len(texts)
    for i, (one, text) in enumerate(zip(found, texts)):
        assert isinstance(one, ratebatch.ContextRating) and len(one) == len(CANDIDATES)
        assert one.bits.dtype == one.posterior.dtype == np.float64 and one.bits.shape == one.posterior.shape == (3,)
        assert one.probs.dtype == np.float32 and one.probs.shape == (len(text),) and (len(text) == 0 or one.probs[0] == 1.0)
        want = np.array([per[c][1][i] for c in range(3)])
        np.testing.assert_allclose(one.bits, want, rtol=1e-12, atol=0)
        # the posterior agrees with the bits; best and margin with the posterior
        lp = -want
        np.testing.assert_allclose(one.posterior, np.exp2(lp - lp.max()) / np.exp2(lp - lp.max()).sum(), rtol=1e-9)
        assert one.best == int(np.argmax(-one.bits)) and isinstance(one.best, int)
        assert abs(one.margin - np.diff(np.sort(one.bits)[:2])[0]) < 1e-9
        assert abs(one.mix_bits - ratebatch.bits_of(one.probs)) <= 1e-6 * max(1.0, one.mix_bits)      # (probs are f32)
    # texts without a prediction: the uniform prior
    assert found[0].posterior.tolist() == found[1].posterior.tolist() == [1 / 3] * 3 and found[1].probs.tolist() == [1.0]
    assert found[0].best == 0 and found[0].margin == 0.0 and found[0].mix_bits == 0.0 and len(found[0].probs) == 0


def test_rate_contexts_with_one_candidate_is_rate_batch(fallback):
    r, texts, _, per = fallback
    found = r.rate_contexts(texts, [CANDIDATES[1]], streams=STREAMS, precision="split")
    for one, probs, bits in zip(found, *per[1]):
        assert np.array_equal(one.probs.view(np.uint32), probs.view(np.uint32))
        assert one.best == 0 and one.margin == np.inf and one.posterior.tolist() == [1.0]
        assert abs(one.bits[0] - bits) <= 1e-12 * max(1.0, bits) and abs(one.mix_bits - bits) <= 1e-12 * max(1.0, bits)
    bare = r.rate_contexts(texts, [CANDIDATES[1]], streams=STREAMS, precision="split", want_probs=False)
    assert all(b.probs is None and np.array_equal(b.bits, f.bits) for b, f in zip(bare, found))


def same_ratings(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for name in ("bits", "posterior"):
            a, b = getattr(g, name), getattr(w, name)
            assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
            np.testing.assert_allclose(a, b, rtol=F64_RTOL, atol=0, err_msg=name)
        assert g.best == w.best
        np.testing.assert_allclose([g.margin, g.mix_bits], [w.margin, w.mix_bits], rtol=F64_RTOL, atol=1e-12)
        if w.probs is None:
            assert g.probs is None
        else:
            assert g.probs.dtype == np.float32 and g.probs.shape == w.probs.shape
            np.testing.assert_allclose(g.probs, w.probs, rtol=P_RTOL, atol=0)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_device_path_equals_the_fallback(fallback, precision):
    r, texts, want, _ = fallback
    dev = small_rater(HostCtxLM, length=LENGTH)
    prior = [0.5, 0.0, 2.0]
    for kwargs in (dict(), dict(prior=prior), dict(want_probs=False)):
        got = dev.rate_contexts(texts, CANDIDATES, streams=STREAMS, precision=precision, **kwargs)
        ref = want if not kwargs else r.rate_contexts(texts, CANDIDATES, streams=STREAMS, precision=precision, **kwargs)
        same_ratings(got, ref)
    seen = dev.model.seen
    assert seen["calls"] == {"rate_window_bulk" if precision == "bf16" else "rate_window", "rate_scatter_planes", "context_mix"}
    assert seen["reset_where"] > 0 and max(seen["B"]) <= STREAMS      # (rows are reused)
    assert dev.model.states[0].shape[0] == 1                          # (a freshly reset single row)
    # the zero prior rules its candidate out
    ruled = dev.rate_contexts(texts, CANDIDATES, prior=prior, streams=STREAMS, precision=precision)
    assert all(one.posterior[1] == 0.0 and one.best != 1 for one in ruled)


def test_small_plane_bytes_gives_the_same(fallback, monkeypatch):
    r, texts, want, _ = fallback
    dev = small_rater(HostCtxLM, length=LENGTH)
    sizes = [len(windows.normalize(t)) for t in texts]
    limit = 60      # characters per chunk: [0, 1, 2, 16, 17] [53] [33, 7] [40] -- and a text larger than the limit is not there
    monkeypatch.setattr(ratebulk, "PLANE_BYTES", 4 * len(CANDIDATES) * limit)
    chunks = ratebulk.text_chunks(sizes, limit)
    assert len(chunks) >= 3
    same_ratings(dev.rate_contexts(texts, CANDIDATES, streams=STREAMS), want)
    assert dev.model.seen["mixes"] == len(chunks)
    # a single text larger than the limit is a chunk of its own
    monkeypatch.setattr(ratebulk, "PLANE_BYTES", 4 * len(CANDIDATES) * 20)
    dev.model.seen["mixes"] = 0
    same_ratings(dev.rate_contexts(texts, CANDIDATES, streams=STREAMS), want)
    assert dev.model.seen["mixes"] == len(ratebulk.text_chunks(sizes, 20)) > len(chunks)


def test_no_predictions_and_no_texts():
    for factory in (OracleLM, HostCtxLM):
        r = small_rater(factory, length=LENGTH)
        assert r.rate_contexts([], CANDIDATES) == []
        found = r.rate_contexts(["", "a", ""], CANDIDATES, prior=[1, 1, 2])
        assert [f.probs.tolist() for f in found] == [[], [1.0], []]
        for f in found:
            assert f.posterior.tolist() == [0.25, 0.25, 0.5] and f.best == 2 and f.margin == 1.0 and f.mix_bits == 0.0
            assert not f.bits.any()


def test_errors():
    r = small_rater(OracleLM, length=LENGTH)
    for bad in (dict(candidates=[]), dict(candidates=[[1]] * 257), dict(candidates=[[1, 2]]), dict(candidates=[[]]),
                dict(prior=[1.0]), dict(prior=[1.0, -1.0, 1.0]), dict(prior=[0.0, 0.0, 0.0]), dict(prior=[1.0, np.nan, 1.0]),
                dict(prior=[1.0, np.inf, 1.0]), dict(precision="fp8")):
        kwargs = dict(candidates=CANDIDATES, precision="split")
        kwargs.update(bad)
        with pytest.raises(ValueError):
            r.rate_contexts(["abc"], **kwargs)
    r.rate_contexts(["abc"], [[1]] * 256, precision="split")      # (256 candidates are allowed, and so are duplicates)
    assert r.rate_contexts(["abc"], [[5000]], precision="split")[0].bits[0] == r.rate_batch(["abc"], [199])[1][0]      # clamped
    r.stateful = False
    with pytest.raises(ValueError):
        r.rate_contexts(["abc"], CANDIDATES, precision="bf16")


def test_stateless_rater_rates_through_rate_batch():
    """a stateless rater's windows are `rate`'s own: no bulk plan, whatever the engine offers"""
    r = small_rater(HostCtxLM, length=LENGTH)
    r.stateful = False
    text = "abc de fgh ab"
    found = r.rate_contexts([text], CANDIDATES, precision="split")
    assert not {"rate_scatter_planes", "context_mix"} & r.model.seen["calls"]
    want = [r.rate_batch([text], c)[1][0] for c in CANDIDATES]
    np.testing.assert_allclose(found[0].bits, want, rtol=1e-12, atol=0)
    assert found[0].best == int(np.argmin(want))


# ---------------------------------------------------------------------------------------------- a planted context
PLANTED = [[12], [171], [185], [60]]
TRUE = 2
CTX_SCALE = 4.0      # the context table of the seeded double times this: the context moves the distributions


def planted_rater(factory):
    r = rater_on(factory, 1)
    w = r.model.get_weights()
    w["Ctx0"] = CTX_SCALE * w["Ctx0"]
    r.model.set_weights(w, 3)
    return r


def test_planted_context_is_found():
    """texts sampled from the double under PLANTED[TRUE]: separate rate_batch calls show that candidate ahead by more than a
    bit on every text, so `best` must name it -- on both paths -- and the posterior is what the bits say"""
    ref = planted_rater(OracleLM)
    rng = np.random.default_rng(8)
    alphabet = sorted(ref.mapping[0], key=ref.mapping[0].get)
    texts = []
    for size in (30, 45, 60, 25):
        ref.model.reset_states(1)
        ids = [int(rng.integers(1, ref.voc_size))]
        for _ in range(size - 1):
            p = np.asarray(ref.model.forward_window(np.array([[ids[-1]]]), np.array([[PLANTED[TRUE]]])), dtype=np.float64)[0, 0]
            p[0] = 0.0      # (the unmapped id has no character)
            ids.append(int(rng.choice(len(p), p=p / p.sum())))
        texts.append("".join(alphabet[k - 1] for k in ids))
    bits = np.stack([ref.rate_batch(texts, c, streams=STREAMS)[1] for c in PLANTED], axis=1)      # [texts, candidates]
    lead = np.delete(bits, TRUE, axis=1).min(axis=1) - bits[:, TRUE]
    print("lead of the planted candidate in bits:", lead)
    assert (lead > 1.0).all(), lead
    for r in (ref, planted_rater(HostCtxLM)):
        found = r.rate_contexts(texts, PLANTED, streams=STREAMS, precision="split")
        for one, b, gap in zip(found, bits, lead):
            assert one.best == TRUE and abs(one.margin - gap) <= 1e-9 * max(1.0, gap)
            np.testing.assert_allclose(one.posterior, np.exp2(b.min() - b) / np.exp2(b.min() - b).sum(), rtol=1e-9)
            assert one.posterior[TRUE] > 0.5 and one.mix_bits <= b[TRUE] + 2.0 + 1e-9      # (the mixture costs at most log2 C more)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_contexts(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("contexts") == run.COMMAND_ORDER.index("rescore") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(3)
    files, texts = [], []
    for i, size in enumerate((45, 1, 70)):
        name = tmp_path / ("scan%d.txt" % i)
        texts.append(random_text(rng, size).replace("\n", " "))
        name.write_text(texts[-1])
        files.append(str(name))
    ref = small_rater(OracleLM, length=LENGTH)
    # --years: 1700, 1710, 1720, 1725 would fold; FROM:TO:STEP 1695:1725:5 gives the decades 170 .. 173 once each
    assert run._year_candidates("1695:1725:5") == [[170], [171], [172], [173]]
    assert run._year_candidates("1784:1784") == [[179]]
    cands = [[170], [171], [172], [173]]
    want = ref.rate_contexts(texts, cands + [[0]], prior=[1, 1, 1, 1, 0], streams=8, precision="split")
    res = CliRunner().invoke(run.cli, ["contexts", "-m", str(model), "-s", "8", "--precision", "split", "--years", "1695:1725:5",
                                       "--top", "2"] + files)
    assert res.exit_code == 0, res.output
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    for line, text, one in zip(lines, texts, want):
        preds = max(len(text) - 1, 1)
        assert line["chars"] == len(text) and line["best"] == cands[one.best] and line["margin_bits"] == one.margin
        assert len(line["top"]) == 2 and line["top"][0][0] == cands[one.best] and line["top"][0][1] >= line["top"][1][1]
        assert line["top"][0][1] == one.posterior[one.best] and one.posterior[4] == 0.0
        assert line["bits_per_char"] == one.bits[one.best] / preds and line["bits_per_char_mixture"] == one.mix_bits / preds
        assert line["bits_per_char_context0"] == one.bits[4] / preds
    # --candidates: a file of tuples in `apply -c`'s notation; context 0 among them is not rated twice
    listing = tmp_path / "candidates.txt"
    listing.write_text("1705\n\n  1850 \n0\n")
    want = ref.rate_contexts(texts, [[171], [185], [0]], streams=8, precision="split")
    res = CliRunner().invoke(run.cli, ["contexts", "-m", str(model), "-s", "8", "--precision", "split", "--candidates", str(listing)]
                             + files)
    assert res.exit_code == 0, res.output
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    for line, one in zip(lines, want):
        assert line["best"] == [[171], [185], [0]][one.best] and "bits_per_char_context0" not in line
        assert len(line["top"]) == 3 and abs(sum(p for _, p in line["top"]) - 1.0) < 1e-12
    # neither or both options, and --years on a model of two variables
    for args in ([], ["--years", "1700:1800", "--candidates", str(listing)], ["--years", "1800:1700"], ["--years", "17oo:1800"]):
        assert CliRunner().invoke(run.cli, ["contexts", "-m", str(model)] + args + files).exit_code != 0
    r.n_ctx = 2
    assert CliRunner().invoke(run.cli, ["contexts", "-m", str(model), "--years", "1700:1800"] + files).exit_code != 0
