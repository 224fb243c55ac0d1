"""`ratebulk.prefix_windows_host`, `ratebulk.fan_states_host`, `Rater.corrections(share_left=True)` and `keraslm-rate correct
--share-left` on the CPU.

A suspect's left context read once for all its variants: the prefix rows are held to brute force from Python lists, the cut
of a hypothesis in two windows to the one-window hypothesis by index arithmetic alone, and on the f64 double the shared call
to the unshared one -- the split changes no arithmetic there, only where the state passes through an array.
kl_prefix_windows, kl_state_fanout and the device path are held to the same statements in test_rate_share_left_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebulk
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import random_text, small_rater
from tests.test_rate_corrections import LENGTH, LONG, SIZES, same_suspects, variant_corpus, variant_suspects
from tests.test_rate_suspects import contract_texts


def prefix_suspects(corpus, offsets, left, count=None):
    """`variant_suspects`, and in the long text the first position with the whole of `left` characters in front of it and the
    one before: (pos, alts, lo) -- lo the start of the long text"""
    pos, alts = variant_suspects(corpus, offsets, count=count)
    lo = int(offsets[LONG])
    assert SIZES[LONG] > left + 1
    more = np.array([lo + left, lo + left - 1], dtype=np.int64)
    return np.concatenate([more, pos]), np.concatenate([alts[:2], alts]), lo


def brute_prefix_row(corpus, offsets, text_ctx, g, left, T):
    """one row from Python lists: (idx [T], ctx [T][n_ctx], tgt [T], valid)"""
    x, off = [int(c) for c in corpus], [int(o) for o in offsets]
    n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
    dummy = ([0] * T, [[0] * n_ctx for _ in range(T)], [-1] * T, 0)
    if not 0 <= g < min(len(x), off[-1]):
        return dummy
    texts = [i for i in range(len(off) - 1) if off[i] <= g < off[i + 1]]
    if not texts or g - off[texts[0]] < left:
        return dummy
    fed = x[g - left:g - 1]
    assert len(fed) == left - 1
    ctx = [[int(c) for c in text_ctx[texts[0]]] if n_ctx else [] for _ in fed] + [[0] * n_ctx for _ in range(T - len(fed))]
    return fed + [0] * (T - len(fed)), ctx, [-1] * T, 1


# ---------------------------------------------------------------------------------------------- the numpy statements
@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("left", [2, 4, 7])
def test_prefix_windows_host_against_brute_force(left, n_ctx):
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, _, lo = prefix_suspects(corpus, offsets, left)
    have = set(pos.tolist())
    first = int(offsets[5])      # (the first character of the text of 7)
    assert len(corpus) != offsets[-1] and {-1, len(corpus), int(offsets[-1]), first, lo + left, lo + left - 1} <= have
    for T in (left - 1, left + 2):
        idx, ctx, tgt, valid = ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos, left, T)
        assert idx.shape == tgt.shape == (len(pos), T) and ctx.shape == (len(pos), T, n_ctx) and valid.shape == (len(pos),)
        assert idx.dtype == ctx.dtype == tgt.dtype == valid.dtype == np.int32
        for s, g in enumerate(pos):
            want = brute_prefix_row(corpus, offsets, text_ctx, int(g), left, T)
            assert idx[s].tolist() == want[0], (T, s)
            assert ctx[s].tolist() == want[1], (T, s)
            assert tgt[s].tolist() == want[2], (T, s)
            assert int(valid[s]) == want[3], (T, s)
        ok = dict(zip(pos.tolist(), valid.tolist()))
        assert ok[lo + left] == 1 and ok[lo + left - 1] == 0 and ok[first] == 0
        assert ok[-1] == ok[len(corpus)] == ok[int(offsets[-1])] == 0
        assert 0 < valid.sum() < len(pos)
        # the valid rows are the suspects whose hypothesis rows have the whole left context: `left_groups`' full group
        full, short = ratebulk.left_groups(pos, offsets, left)
        assert np.array_equal(full, np.nonzero(valid)[0]) and np.array_equal(short, np.nonzero(valid == 0)[0])
    for bad in (dict(left=1), dict(T=left - 2), dict(T=1025)):
        a = dict(dict(left=left, T=left + 2), **bad)
        with pytest.raises(ValueError):
            ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos, a["left"], a["T"])


def test_fan_states_host_and_prefix_batches():
    rng = np.random.default_rng(2)
    parent = np.array([0, 0, 3, -1, 4, 4, 4, 7])
    one = rng.standard_normal((5, 4, 6)).astype(np.float32)
    out = ratebulk.fan_states_host(one, parent)
    assert out.shape == (8, 4, 6) and out.dtype == np.float32
    for b, p in enumerate(parent):
        assert np.array_equal(out[b], one[p] if 0 <= p < 5 else np.zeros((4, 6), dtype=np.float32))
    many = [rng.standard_normal((5, 3)) for _ in range(4)]
    outs = ratebulk.fan_states_host(many, parent)
    assert isinstance(outs, list) and len(outs) == 4
    for a, o in zip(many, outs):
        assert o.dtype == np.float64 and np.array_equal(o, ratebulk.fan_states_host(a, parent))
        o[0] = 9.0
        assert not (a == 9.0).any()      # (copies)
    # streams 12, R = 5: chunks of 2 suspects (10 rows), prefix batches of 12
    assert ratebulk.prefix_batches(27, 12, 5) == [(0, 12, [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 12)]),
                                                  (12, 24, [(12, 14), (14, 16), (16, 18), (18, 20), (20, 22), (22, 24)]),
                                                  (24, 27, [(24, 26), (26, 27)])]
    assert ratebulk.prefix_batches(0, 12, 5) == []
    assert ratebulk.prefix_batches(3, 4, 5) == [(0, 3, [(0, 1), (1, 2), (2, 3)])]      # (fewer streams than variants: one suspect per chunk)
    for n, streams, R in ((1000, 1024, 5), (41, 64, 8), (7, 1, 2)):
        chunk = max(1, streams // R)
        batches = ratebulk.prefix_batches(n, streams, R)
        assert [b - a for a, b, _ in batches[:-1]] == [(streams // chunk) * chunk] * (len(batches) - 1)
        flat = [cd for _, _, chunks in batches for cd in chunks]
        assert flat == [(c, min(c + chunk, n)) for c in range(0, n, chunk)]      # (the chunks of the unshared route)
        assert all(a <= c and d <= b for a, b, chunks in batches for c, d in chunks)
        assert all((b - a) <= streams and (d - c) * R <= max(streams, R) for a, b, chunks in batches for c, d in chunks)


@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("deletions,insertions", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("left", [2, 4, 7])
def test_two_windows_feed_what_one_window_feeds(left, deletions, insertions, n_ctx):
    """index arithmetic, no model: for every suspect with L == left, the prefix row's fed ids followed by the short row
    (left = 1) are the one-window row (left), ids, contexts and targets, for all R variants"""
    ahead = 3
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts, _ = prefix_suspects(corpus, offsets, left)
    K = alts.shape[1]
    R = K + 1 + deletions + K * insertions
    short_T = 1 + ahead + insertions
    pidx, pctx, ptgt, pok = ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos, left, left - 1)
    sidx, sctx, stgt, sok = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, 1, ahead, deletions, short_T,
                                                          insertions)
    idx, ctx, tgt, ok = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions,
                                                      left - 1 + short_T, insertions)
    full, _ = ratebulk.left_groups(pos, offsets, left)
    assert len(full) >= 3 and (ptgt == -1).all()
    seen = {0: 0, 1: 0}
    for s in full:
        assert pok[s] == 1
        for v in range(R):
            b = s * R + v
            assert sok[b] == ok[b]
            seen[int(ok[b])] += 1
            if not ok[b]:
                continue      # (no hypothesis: the cost is +inf whatever the rows hold)
            assert np.array_equal(np.concatenate([pidx[s], sidx[b]]), idx[b]), (s, v)
            assert np.array_equal(np.concatenate([pctx[s], sctx[b]]), ctx[b]), (s, v)
            assert np.array_equal(np.concatenate([ptgt[s], stgt[b]]), tgt[b]), (s, v)
    assert seen[0] and seen[1], seen


# ---------------------------------------------------------------------------------------------- the Rater on the double
def streams_for(n_full, R):
    """the first number of streams from 12 on with which the full group is no whole number of prefix batches, a batch feeds
    several suffix chunks and the last chunk is short"""
    for streams in range(12, 40):
        batches = ratebulk.prefix_batches(n_full, streams, R)
        chunk = max(1, streams // R)
        a, b, chunks = batches[-1]
        if len(batches) > 1 and (b - a) < batches[0][1] and len(batches[0][2]) > 1 and chunks[-1][1] - chunks[-1][0] < chunk:
            return streams
    raise AssertionError("no such number of streams")


@pytest.mark.parametrize("deletions,insertions", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("left", [5, 7])
def test_share_left_on_the_double_is_the_unshared_call(left, deletions, insertions):
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    k, ahead = 3, 3
    R = k + 1 + int(deletions) + k * int(insertions)
    n_full = sum(max(len(t) - left, 0) for t in texts)      # (every predicted character a suspect)
    streams = streams_for(n_full, R)
    args = dict(k=k, streams=streams, max_prob=1.0, min_rank=0, left=left, ahead=ahead, deletions=deletions,
                insertions=insertions, min_gain=0.25, precision="split")
    want, want_bits = r.corrections(texts, contexts, **args)
    assert r.shared_left is None
    found, bits = r.corrections(texts, contexts, share_left=True, **args)
    stats = r.shared_left
    assert stats["shared"] == n_full and 0 < stats["shared"] < stats["suspects"] == sum(len(f) for f in found)
    batches = ratebulk.prefix_batches(n_full, streams, R)
    assert stats["prefix_windows"] == len(batches) > 1 and stats["suffix_windows"] == sum(len(c) for _, _, c in batches)
    assert stats["unshared_windows"] >= 1
    assert np.array_equal(bits, want_bits)
    same_suspects(found, want)
    worst, proposals = 0.0, 0
    for one, ref in zip(found, want):
        assert one.cost.shape == ref.cost.shape == (len(one), R)
        assert np.array_equal(np.isinf(one.cost), np.isinf(ref.cost))
        fin = np.isfinite(ref.cost)
        if fin.any():
            worst = max(worst, float(np.abs(one.cost[fin] - ref.cost[fin]).max()))
        assert np.array_equal(one.best_id, ref.best_id) and np.array_equal(one.best_op, ref.best_op)
        assert (np.abs(one.gain - ref.gain) <= 1e-9).all()
        proposals += int((one.best_id != -1).sum())
    print("largest |cost_shared - cost_unshared| = %.3g bits" % worst)
    assert worst <= 1e-9 and proposals > 0
    # afterwards: a freshly reset single row
    assert r.model.states[0].shape[0] == 1 and not any(np.asarray(st).any() for st in r.model.states)


def test_share_left_below_four_characters_is_the_unshared_route():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    args = dict(k=3, streams=12, max_prob=1.0, min_rank=0, left=3, ahead=3, deletions=True, min_gain=0.25, precision="split")
    want, want_bits = r.corrections(texts, contexts, **args)
    found, bits = r.corrections(texts, contexts, share_left=True, **args)
    assert r.shared_left is None
    assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
    same_suspects(found, want)
    for one, ref in zip(found, want):
        for name in ("cost", "best_id", "gain", "best_op"):
            a, b = getattr(one, name), getattr(ref, name)
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    # no suspects, and texts without a prediction: nothing to share
    for some, kw in ((["", "a"], {}), (["abcabcabc", "", "b"], dict(max_prob=0.0))):
        found, _ = r.corrections(some, k=2, left=5, deletions=True, share_left=True, **kw)
        assert [len(f) for f in found] == [0] * len(some) and r.shared_left is None
        assert all(f.cost.shape == (0, 4) for f in found)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_correct_share_left(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(3)
    files = []
    for i, size in enumerate((45, 1, 70)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        name.write_text(random_text(rng, size).replace("\n", " "))
        files.append(str(name))
    args = ["correct", "-m", str(model), "-s", "12", "--precision", "split", "-k", "2", "--max-prob", "1.0", "--min-rank", "0",
            "--left", "6", "--ahead", "3", "--deletions", "--min-gain", "0.1", "--apply"]
    calls = []
    plain = r.corrections
    monkeypatch.setattr(r, "corrections", lambda *a, **kw: calls.append(kw.get("share_left")) or plain(*a, **kw))
    lines = []
    for extra in ([], ["--share-left"]):
        res = CliRunner().invoke(run.cli, args + extra + files)
        assert res.exit_code == 0, res.output
        lines.append([json.loads(l) for l in res.output.strip().split("\n")])
        assert (r.shared_left is not None) == bool(extra)
    assert calls == [False, True]
    assert r.shared_left["shared"] == 39 + 64
    assert sum(new is not None for l in lines[0] for _, _, new, _ in l["corrections"]) > 0
    for a, b in zip(*lines):
        assert a["file"] == b["file"] and a["suspects"] == b["suspects"] and a["corrected"] == b["corrected"]
        assert [c[:3] for c in a["corrections"]] == [c[:3] for c in b["corrections"]]
        assert all(abs(x[3] - y[3]) <= 1e-9 for x, y in zip(a["corrections"], b["corrections"]))
