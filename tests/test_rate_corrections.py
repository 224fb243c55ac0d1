"""`ratebulk.variant_windows_host`, `ratebulk.variant_pick_host`, `Rater.corrections`, `ratebatch.Corrections.apply` and
`keraslm-rate correct` on the CPU.

The oracle-backed engine double has no `variant_windows`, so the Rater runs `suspects`, the numpy statement of the hypothesis
windows and whole softmaxes summed on the host; the definition is held to brute force here -- every row built on its own
from Python lists, every cost from a fresh one-row window over the hypothesis.  kl_variant_windows and the device path are
held to the same statements in test_rate_corrections_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import random_text, small_rater
from tests.test_rate_suspects import contract_texts

LENGTH = 16
SIZES = [0, 1, 2, 1, 0, 7, 50, 3]
LONG = 6              # the text of 50 characters
DEEP = 20             # a position of it deeper than the `left` these tests use on the CPU (at most 7)


def variant_corpus(n_ctx, seed=5, tail=3):
    """texts of SIZES characters end to end (ids 1 .. 9) and `tail` ids behind the last text, so that n_corpus and offsets[-1]
    differ; per-text contexts"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    corpus = rng.integers(1, 10, int(offsets[-1]) + tail).astype(np.int32)
    text_ctx = rng.integers(1, 200, (len(SIZES), n_ctx)).astype(np.int32) if n_ctx else None
    return corpus, offsets, text_ctx


def variant_suspects(corpus, offsets, count=None, K=3, seed=9):
    """suspects at every position of the texts of up to 7 characters (first characters included), at the last character of the
    long text, at a position of it deeper than `left` and near its start, and at -1, n_corpus and offsets[-1]; per suspect one
    alternative of -1, one equal to the character written and one ordinary one (K = 3) -- for other K, and beyond the listed
    suspects (count), drawn at random from those kinds"""
    rng = np.random.default_rng(seed)
    pos = []
    for i, size in enumerate(SIZES):
        if size <= 7:
            pos += list(range(int(offsets[i]), int(offsets[i + 1])))
    lo, hi = int(offsets[LONG]), int(offsets[LONG + 1])
    pos += [hi - 1, lo + DEEP, lo + 3, lo + 47, -1, len(corpus), int(offsets[-1])]
    pos = np.array(pos, dtype=np.int64)
    if count is not None:
        more = rng.integers(-2, len(corpus) + 2, max(count - len(pos), 0))
        pos = np.concatenate([pos, more])[:count]
    inside = (pos >= 0) & (pos < len(corpus))
    w = np.where(inside, corpus[np.where(inside, pos, 0)], 4).astype(np.int32)
    other = (w % 9 + 1).astype(np.int32)
    assert (other != w).all()
    if K == 3:
        alts = np.stack([np.full(len(pos), -1, dtype=np.int32), w, other], axis=1)
    else:
        kinds = np.stack([np.full(len(pos), -1, dtype=np.int32), w, other, (other % 9 + 1).astype(np.int32)], axis=1)
        alts = np.take_along_axis(kinds, rng.integers(0, 4, (len(pos), K)), axis=1)
    return pos, np.ascontiguousarray(alts, dtype=np.int32)


def brute_row(corpus, offsets, text_ctx, g, alts, v, left, ahead, T):
    """one row from Python lists: (idx [T], ctx [T][n_ctx], tgt [T], valid, L, A)"""
    x, off = [int(c) for c in corpus], [int(o) for o in offsets]
    n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
    K = len(alts)
    dummy = ([0] * T, [[0] * n_ctx for _ in range(T)], [-1] * T, 0)
    if not 0 <= g < min(len(x), off[-1]):
        return dummy + (None, None)
    texts = [i for i in range(len(off) - 1) if off[i] <= g < off[i + 1]]
    if not texts:
        return dummy + (None, None)
    i = texts[0]
    L, A = min(left, g - off[i]), min(ahead, off[i + 1] - 1 - g)
    if L == 0:
        return dummy + (L, A)
    before, after = x[g - L:g], x[g + 1:g + 1 + A]
    if v == 0:
        q = before + [x[g]] + after
    elif v <= K:
        a = int(alts[v - 1])
        if a < 0 or a == x[g]:
            return dummy + (L, A)
        q = before + [a] + after
    else:
        if A == 0:
            return dummy + (L, A)
        q = before + after
    fed = len(q) - 1
    idx = q[:fed] + [0] * (T - fed)
    tgt = [-1] * T
    for t in range(L - 1, fed):
        tgt[t] = q[t + 1]
    ctx = [[int(c) for c in text_ctx[i]] if n_ctx else [] for _ in range(fed)] + [[0] * n_ctx for _ in range(T - fed)]
    return idx, ctx, tgt, 1, L, A


# ---------------------------------------------------------------------------------------------- the numpy statements
@pytest.mark.parametrize("n_ctx", [0, 2, 3])
@pytest.mark.parametrize("deletions", [0, 1])
def test_variant_windows_host_against_brute_force(deletions, n_ctx):
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = variant_suspects(corpus, offsets)
    assert len(corpus) != offsets[-1] and {-1, len(corpus), int(offsets[-1])} <= set(pos.tolist())
    K = alts.shape[1]
    R = K + 1 + deletions
    for left, ahead, T in ((5, 4, 9), (5, 4, 12), (1, 0, 3), (7, 0, 7)):
        seen = set()
        idx, ctx, tgt, valid = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T)
        assert idx.shape == tgt.shape == (len(pos) * R, T) and ctx.shape == (len(pos) * R, T, n_ctx) and valid.shape == (len(pos) * R,)
        assert idx.dtype == ctx.dtype == tgt.dtype == valid.dtype == np.int32
        for s, g in enumerate(pos):
            for v in range(R):
                b = s * R + v
                want = brute_row(corpus, offsets, text_ctx, int(g), alts[s], v, left, ahead, T)
                assert idx[b].tolist() == want[0], (left, ahead, T, s, v)
                assert ctx[b].tolist() == want[1], (left, ahead, T, s, v)
                assert tgt[b].tolist() == want[2], (left, ahead, T, s, v)
                assert int(valid[b]) == want[3]
                L, A = want[4], want[5]
                seen.add("valid" if want[3] else "invalid")
                if want[3]:
                    seen.add("L<left" if L < left else "L==left")
                    if ahead:
                        seen.add("A<ahead" if A < ahead else "A==ahead")
                    seen.add("A==0" if A == 0 else "A>0")
                    # the targets are the variant's character, if it has one, and the A characters after it
                    assert (tgt[b] >= 0).sum() == A + (0 if v > K else 1)
        assert {"valid", "invalid", "L==left", "A==0"} <= seen, seen
        if left > 1:      # (L >= 1 in every valid row)
            assert "L<left" in seen, seen
        if ahead:
            assert {"A<ahead", "A==ahead", "A>0"} <= seen, seen
        # per suspect: the alternative of -1 and the one equal to the character are no variants; the ordinary one is
        ok = valid.reshape(len(pos), R)
        assert not ok[:, 1].any() and not ok[:, 2].any() and (ok[:, 3] == ok[:, 0]).all()
        if deletions:
            assert (ok[:, 4] <= ok[:, 0]).all()
    for bad in (dict(left=0), dict(ahead=-1), dict(T=8), dict(T=1025), dict(deletions=2)):
        a = dict(dict(left=5, ahead=4, deletions=0, T=9), **bad)
        with pytest.raises(ValueError):
            ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, a["left"], a["ahead"], a["deletions"], a["T"])


def test_variant_pick_host():
    inf = np.inf
    cost = np.array([[5.0, 3.0, 3.0, 4.0],      # an exact tie: the smallest v
                     [5.0, 9.0, 1.0, 0.5],      # the last variant is invalid: its cost does not count
                     [5.0, 7.0, 6.0, 8.0],      # every variant reads worse: the least bad, a negative gain
                     [5.0, 1.0, 1.0, 1.0],      # no valid variant beside the text as written
                     [5.0, 1.0, 2.0, 3.0],      # v = 0 invalid (and so is everything else)
                     [5.0, 1.0, 2.0, 3.0]])     # v = 0 marked invalid alone: still no proposal
    valid = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 1]], dtype=np.int32)
    before = cost.copy()
    out, best, gain = ratebulk.variant_pick_host(cost, valid)
    assert np.array_equal(cost, before)                      # (the input is not written to)
    assert out.dtype == np.float64 and best.dtype == np.int32 and gain.dtype == np.float64
    assert best.tolist() == [1, 2, 2, 0, 0, 0]
    assert gain.tolist() == [2.0, 4.0, -1.0, 0.0, 0.0, 0.0]
    assert np.array_equal(out == inf, valid == 0) and np.array_equal(out[valid == 1], before[valid == 1])
    out, best, gain = ratebulk.variant_pick_host(np.zeros((0, 4)), np.zeros((0, 4), dtype=np.int32))
    assert out.shape == (0, 4) and best.shape == gain.shape == (0,)


# ---------------------------------------------------------------------------------------------- Corrections.apply
def test_corrections_apply():
    mapping = ({"a": 1, "b": 2, "c": 3}, {1: "a", 2: "b", 3: "c"})
    k = 2
    one = ratebatch.Corrections(np.array([1, 3, 4, 6], dtype=np.int64), np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.int32),
                                np.zeros((4, k), dtype=np.int32), np.zeros((4, k), dtype=np.float32),
                                np.zeros((4, k + 2)), np.array([3, -2, -1, 0], dtype=np.int32), np.array([2.0, 1.5, 0.0, 3.0]))
    assert isinstance(one, ratebatch.Suspects) and len(one) == 4
    assert one.proposals(mapping) == ["c", "", None, None] == one.proposals(mapping[1])
    #       0123456
    text = "abacaba"
    # position 1 'b' -> 'c'; position 3 'c' dropped; position 4 keeps its 'a'; the unmapped id 0 at position 6 writes nothing
    assert one.apply(text, mapping) == "acaaba"
    none = ratebatch.Corrections(*([a[:0] for a in (one.positions, one.probs, one.rank, one.alt_ids, one.alt_probs, one.cost,
                                                    one.best_id, one.gain)]))
    assert none.apply(text, mapping) == text and none.apply("", mapping) == ""


# ---------------------------------------------------------------------------------------------- the Rater on the double
def fresh_cost(r, ids, ctx, j, alts, v, left, ahead):
    """the cost of variant v of the suspect at position j of one text, by definition: a one-row window from a zero state over
    the hypothesis, nothing padded; None where there is no such variant"""
    K = len(alts)
    n = len(ids)
    L, A = min(left, j), min(ahead, n - 1 - j)
    if L == 0:
        return None
    before, after = list(ids[j - L:j]), list(ids[j + 1:j + 1 + A])
    if v == 0:
        q = before + [int(ids[j])] + after
    elif v <= K:
        if alts[v - 1] < 0 or alts[v - 1] == ids[j]:
            return None
        q = before + [int(alts[v - 1])] + after
    else:
        if A == 0:
            return None
        q = before + after
    x = np.array([q[:-1]], dtype=np.int32)
    z = np.tile(np.asarray(windows.clamp_context(ctx), dtype=np.int32)[None, None, :], (1, x.shape[1], 1))
    r.model.reset_states(1)
    full = np.asarray(r.model.forward_window(x, z, want_probs=True), dtype=np.float64)[0]
    return float(-sum(np.log2(max(full[t, q[t + 1]], 1e-99)) for t in range(L - 1, len(q) - 1)))


def check_against_definition(r, ref, texts, contexts, found, k, left, ahead, deletions, min_gain):
    R = k + 1 + deletions
    seen = {"proposal": 0, "none": 0, "invalid": 0, "valid": 0, "deep": 0}
    for text, ctx, one in zip(texts, contexts, found):
        ids = windows.encode(windows.normalize(text), r.mapping[0])
        assert one.cost.shape == (len(one), R) and one.cost.dtype == np.float64
        assert one.best_id.shape == one.gain.shape == (len(one),) and one.best_id.dtype == np.int32 and one.gain.dtype == np.float64
        for m, j in enumerate(one.positions):
            want = [fresh_cost(ref, ids, ctx, int(j), one.alt_ids[m], v, left, ahead) for v in range(R)]
            seen["deep"] += int(j) > left
            for v in range(R):
                if want[v] is None:
                    assert one.cost[m, v] == np.inf
                    seen["invalid"] += 1
                else:
                    assert abs(one.cost[m, v] - want[v]) <= 1e-9 * abs(want[v]), (m, v)
                    seen["valid"] += 1
            # best_id and gain follow from the costs the call returned
            _, best, gain = ratebulk.variant_pick_host(one.cost[m:m + 1], np.isfinite(one.cost[m:m + 1]))
            best, gain = int(best[0]), float(gain[0])
            if best == 0 or not gain >= min_gain:
                assert one.best_id[m] == -1 and one.gain[m] == 0.0
                seen["none"] += 1
            else:
                assert one.best_id[m] == (-2 if best == k + 1 else one.alt_ids[m, best - 1]) and one.gain[m] == gain
                assert one.gain[m] >= min_gain
                seen["proposal"] += 1
    return seen


def same_suspects(found, ref):
    assert len(found) == len(ref)
    for one, want in zip(found, ref):
        assert isinstance(one, ratebatch.Corrections)
        for name in ("positions", "probs", "rank", "alt_ids", "alt_probs"):
            a, b = getattr(one, name), getattr(want, name)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


def test_corrections_on_the_double_follow_the_definition():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    ref = small_rater(OracleLM, length=LENGTH)
    rated, _ = ref.rate_alternatives(texts, contexts, k=3, streams=4)
    median = float(np.median(np.concatenate([x.probs[1:] for x in rated])))
    k, left, ahead = 3, 5, 3
    # the suspects below the median probability with deletions; then every predicted character (the model's first choices among
    # them: an alternative equal to the character written is no variant) without
    for deletions, streams, precision, min_gain, max_prob, min_rank in ((True, 16, "bf16", 0.25, median, 1),
                                                                        (False, 7, "split", -np.inf, 1.0, 0)):
        want, want_bits = ref.suspects(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank,
                                       precision=precision)
        found, bits = r.corrections(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank, left=left,
                                    ahead=ahead, deletions=deletions, min_gain=min_gain, precision=precision)
        assert np.array_equal(bits, want_bits)
        same_suspects(found, want)
        seen = check_against_definition(r, ref, texts, contexts, found, k, left, ahead, int(deletions), min_gain)
        assert seen["valid"] and seen["invalid"] and seen["proposal"] and seen["deep"], seen
        assert seen["none"] or min_gain == -np.inf, seen
        # afterwards: a freshly reset single row
        assert r.model.states[0].shape[0] == 1 and not any(np.asarray(st).any() for st in r.model.states)
    # min_gain = inf: no proposal is kept; the costs stay
    none, _ = r.corrections(texts, contexts, k=k, streams=16, max_prob=median, min_rank=1, left=left, ahead=ahead,
                            deletions=True, min_gain=np.inf)
    same_suspects(none, ref.suspects(texts, contexts, k=k, streams=16, max_prob=median, min_rank=1)[0])
    assert sum(len(f) for f in none) > 0
    for one in none:
        assert (one.best_id == -1).all() and (one.gain == 0.0).all() and one.cost.shape == (len(one), k + 2)


def test_corrections_edge_inputs_and_errors():
    r = small_rater(OracleLM, length=LENGTH)
    # texts without a prediction, and no suspects at all: empty arrays of the right shapes and dtypes
    for texts, kw in ((["", "a"], {}), (["abcabc", "", "b"], dict(max_prob=0.0))):
        found, bits = r.corrections(texts, k=2, deletions=True, **kw)
        want, want_bits = r.suspects(texts, k=2, **kw)
        assert np.array_equal(bits, want_bits) and len(found) == len(texts)
        same_suspects(found, want)
        for one in found:
            assert len(one) == 0 and one.cost.shape == (0, 4) and one.cost.dtype == np.float64
            assert one.best_id.shape == (0,) and one.best_id.dtype == np.int32
            assert one.gain.shape == (0,) and one.gain.dtype == np.float64
            assert one.apply("abc", r.mapping) == "abc"
    for bad in (dict(left=0), dict(ahead=-1), dict(left=1000, ahead=25), dict(precision="f32"), dict(min_rank=-1),
                dict(max_prob=float("nan"))):
        with pytest.raises(ValueError):
            r.corrections(["abc"], **bad)
    r.corrections(["abcabcabc"], left=1000, ahead=24, max_prob=1.0, min_rank=0)      # (1024 is allowed)
    for k in (0, 9):
        with pytest.raises(AssertionError):
            r.corrections(["abc"], k=k)
    r.stateful = False
    for precision in ("bf16", "split"):
        with pytest.raises(ValueError):
            r.corrections(["abc"], precision=precision)


# ---------------------------------------------------------------------------------------------- the split-precision contract
SPLIT_BOUND = 2e-5      # the project's split-precision bound on a probability (test_rate_window_against_the_oracle)
SPLIT = dict(k=3, streams=64, left=6, ahead=3, deletions=True, min_gain=0.0, min_rank=0)


def wide_rater(factory, length=LENGTH, seed=11):
    """`small_rater` at width 512: depth 2 over the ten-character alphabet, the same recipe for the weights"""
    from oracle import lstm_oracle as O
    from ocrd_keraslm_amd.lib import Rater
    from tests.test_rate_bulk_gpu import ALPHABET
    r = Rater(engine_factory=factory)
    r.width, r.depth, r.length = 512, 2, length
    r.stateful = True
    r.mapping = (dict((c, i) for i, c in enumerate(sorted(ALPHABET), 1)), dict((i, c) for i, c in enumerate(sorted(ALPHABET), 1)))
    r.voc_size = len(ALPHABET) + 1
    r.configure()
    r.model.set_weights(O.init_weights(O.ModelConfig(2, 512, r.voc_size, 1), seed=seed, emb_std=0.3, dtype=np.float32), 3)
    r.status = 2
    return r


def wide_texts(seed=21):
    rng = np.random.default_rng(seed)
    texts = [random_text(rng, s) for s in (0, 1, 2, LENGTH + 1, 40, 7, 33)]
    return texts, [[(171 if i % 2 else 185)] for i in range(len(texts))]


def gap_threshold(probs):
    """a max_prob no position sits on: the middle of the widest gap of the sorted probabilities between their 15 % and 45 %
    quantiles (a share of the characters that keeps the double's windows few)"""
    flat = np.sort(np.asarray(probs, dtype=np.float64))
    lo, hi = int(0.15 * len(flat)), max(int(0.45 * len(flat)), int(0.15 * len(flat)) + 2)
    g = lo + int(np.argmax(np.diff(flat[lo:hi])))
    return 0.5 * (flat[g] + flat[g + 1]), float(flat[g + 1] - flat[g])


def oracle_costs(oracle, texts, contexts, found, left, ahead, deletions):
    """for the suspects and alternatives of `found` (any engine's): the double's cost of every variant and the first-order
    bound on a split-precision cost, 2 * sum over the scored positions of SPLIT_BOUND / (p_oracle * ln 2).  The hypotheses
    come from variant_windows_host, every text on its own; all rows of a text share one window call from zero states.
    Returns per text (cost [m, R] with +inf where invalid, bound [m, R])."""
    out = []
    for text, ctx, one in zip(texts, contexts, found):
        k = one.alt_ids.shape[1]
        R = k + 1 + int(deletions)
        m = len(one)
        if not m:
            out.append((np.zeros((0, R)), np.zeros((0, R))))
            continue
        ids = windows.encode(windows.normalize(text), oracle.mapping[0])
        x, z, y, ok = ratebulk.variant_windows_host(ids, [0, len(ids)], np.asarray([windows.clamp_context(ctx)], dtype=np.int32),
                                                    one.positions, one.alt_ids, left, ahead, int(deletions),
                                                    max(left + ahead, ratebulk.MIN_T))
        oracle.model.reset_states(len(x))
        full = np.asarray(oracle.model.forward_window(x, z, want_probs=True), dtype=np.float64)
        p = np.take_along_axis(full, np.maximum(y, 0)[:, :, None], axis=2)[:, :, 0]
        scored = y >= 0
        cost = -np.where(scored, np.log2(np.maximum(p, 1e-99)), 0.0).sum(axis=1)
        bound = 2.0 * np.where(scored, SPLIT_BOUND / (np.maximum(p, 1e-99) * np.log(2.0)), 0.0).sum(axis=1)
        cost[ok == 0] = np.inf
        out.append((cost.reshape(m, R), bound.reshape(m, R)))
    oracle.model.reset_states(1)
    return out


def decided(cost, bound):
    """per suspect: do the oracle's two least costs among the variants v >= 1 differ by more than twice the (largest) bound --
    then a split-precision run within the bound picks the same one.  A suspect with fewer than two variants is decided."""
    rest = np.sort(cost[:, 1:], axis=1)
    if rest.shape[1] < 2:
        return np.ones(len(cost), dtype=bool)
    with np.errstate(invalid="ignore"):
        gap = rest[:, 1] - rest[:, 0]                      # (inf - inf = nan: no variant at all)
    return ~np.isfinite(rest[:, 1]) | (gap > 2.0 * np.where(np.isfinite(cost), bound, 0.0).max(axis=1))


def test_split_contract_texts_keep_the_oracle_within_the_cap():
    """the texts and seed of test_rate_corrections_gpu's split-precision test: on the double alone at most 10 % of the suspects
    have two best variants too close to call"""
    texts, contexts = wide_texts()
    oracle = wide_rater(OracleLM)
    rated, _ = oracle.rate_alternatives(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"])
    max_prob, gap = gap_threshold(np.concatenate([r.probs[1:] for r in rated]))
    assert gap >= 1e-4, gap      # (4e-5 between two split-precision routes: test_rater_bf16_alternatives_and_suspects)
    found, _ = oracle.corrections(texts, contexts, max_prob=max_prob, precision="split", **SPLIT)
    total = sum(len(f) for f in found)
    assert 10 <= total < sum(max(len(t) - 1, 0) for t in texts)
    costs = oracle_costs(oracle, texts, contexts, found, SPLIT["left"], SPLIT["ahead"], SPLIT["deletions"])
    open_ = 0
    for one, (cost, bound) in zip(found, costs):
        assert np.array_equal(np.isinf(cost), np.isinf(one.cost))
        fin = np.isfinite(cost)
        assert (np.abs(one.cost[fin] - cost[fin]) <= 1e-9 * np.abs(cost[fin])).all()
        open_ += int((~decided(cost, bound)).sum())
    print("suspects %d, too close to call %d" % (total, open_))
    assert open_ <= 0.1 * total


# ---------------------------------------------------------------------------------------------- command line
def test_cli_correct(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("correct") == run.COMMAND_ORDER.index("suspects") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(3)
    files, texts = [], []
    for i, size in enumerate((45, 1, 70)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size).replace("\n", " "))
        name.write_text(texts[-1])
        files.append(str(name))
    contexts = [[170], [174], [178]]
    ref = small_rater(OracleLM, length=LENGTH)
    rated, _ = ref.rate_alternatives(texts, contexts, k=2, streams=2)
    median = float(np.median(np.concatenate([x.probs[1:] for x in rated])))
    args = ["correct", "-m", str(model), "-s", "12", "--precision", "split", "-k", "2", "--max-prob", repr(median), "--min-rank", "1",
            "--left", "6", "--ahead", "3", "--deletions", "--min-gain", "0.1"]
    found, bits = ref.corrections(texts, contexts, k=2, streams=12, max_prob=median, min_rank=1, left=6, ahead=3, deletions=True,
                                  min_gain=0.1, precision="split")
    assert sum((f.best_id != -1).sum() for f in found) > 0
    for extra in ([], ["--apply"]):
        res = CliRunner().invoke(run.cli, args + extra + files)
        assert res.exit_code == 0, res.output
        lines = [json.loads(l) for l in res.output.strip().split("\n")]
        assert [l["file"] for l in lines] == files
        for line, text, one, total in zip(lines, texts, found, bits):
            assert line["chars"] == len(text) and line["bits_per_char"] == float(total) / max(len(text) - 1, 1)
            assert [row[0] for row in line["suspects"]] == one.positions.tolist()
            assert len(line["corrections"]) == len(one)
            for (pos, written, new, gain), j, b, g in zip(line["corrections"], one.positions, one.best_id, one.gain):
                assert pos == int(j) and written == text[pos] and gain == float(g)
                assert new == (None if b == -1 else "" if b == -2 else ref.mapping[1][int(b)])
            assert ("corrected" in line) == bool(extra)
            if extra:
                assert line["corrected"] == one.apply(text, ref.mapping)
        assert len(lines[1]["corrections"]) == 0
    assert any(l["corrected"] != t for l, t in zip(lines, texts))
    for bad in (["-k", "0"], ["--left", "0"], ["--ahead", "-1"], ["--left", "1000", "--ahead", "30"], ["--precision", "f32"]):
        assert CliRunner().invoke(run.cli, ["correct", "-m", str(model)] + bad + files).exit_code != 0
