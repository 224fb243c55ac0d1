"""`ratebulk.lexicon_channel_host`, `ratebatch.Channel`, `Rater.channel`, `Rater.lexicon_neighbours(channel=..)`,
`Rater.rescore(prior=..)`, `Rater.correct_words(channel=..)` and `keraslm-rate lexicon --channel` on the CPU.

The statement of the weighted look-up is held to an independent shortest path over the cells of a (query, entry) pair --
Dijkstra, pushing along the edges where the statement pulls, over ALL entries where the statement walks the length classes its
prices open -- and to distances worked by hand.  The oracle-backed engine double has no `lexicon_channel`, so the Rater runs the
statement; the device kernel is held to the statement in test_lexicon_channel_gpu.py."""
import heapq
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.oracle_engine import OracleLM
from tests.test_lexicon import brute_neighbours, lexicon_words, mutate, pooled, random_lexicon, same_rescored
from tests.test_rate_bulk_gpu import random_text, small_rater
from tests.test_rate_suspects import contract_texts

LENGTH = 16


# ---------------------------------------------------------------------------------------------- the statement
def records(rules):
    """[(src ids, tgt ids, cost)] as (rules int32 [R, 10], rule_cost int32 [R]): the layout kl_confusion_counts writes"""
    table = np.zeros((len(rules), 10), dtype=np.int32)
    for r, (src, tgt, _) in enumerate(rules):
        table[r, 0], table[r, 1] = len(src), len(tgt)
        table[r, 2:2 + len(src)] = src
        table[r, 6:6 + len(tgt)] = tgt
    return table, np.asarray([c for _, _, c in rules], dtype=np.int32).reshape(-1)


def shortest(q, e, V, rules, unit):
    """the cheapest way from (0, 0) to (len(q), len(e)): Dijkstra over the cells, an edge per plain edit, per match and per
    rule that stands at the cell; two ids are equal iff they are the same number within [0, V)"""
    same = lambda a, b: len(a) == len(b) and all(x == y and 0 <= x < V for x, y in zip(a, b))
    m, n = len(q), len(e)
    done, heap = {}, [(0, 0, 0)]
    while heap:
        d, i, j = heapq.heappop(heap)
        if (i, j) in done:
            continue
        done[i, j] = d
        if (i, j) == (m, n):
            return d
        if i < m:
            heapq.heappush(heap, (d + unit, i + 1, j))
        if j < n:
            heapq.heappush(heap, (d + unit, i, j + 1))
        if i < m and j < n:
            heapq.heappush(heap, (d + (0 if same(q[i:i + 1], e[j:j + 1]) else unit), i + 1, j + 1))
        for src, tgt, cost in rules:
            s, t = len(src), len(tgt)
            if i + s <= m and j + t <= n and same(q[i:i + s], src) and same(e[j:j + t], tgt):
                heapq.heappush(heap, (d + cost, i + s, j + t))
    return done[m, n]


def brute_channel(queries, entries, V, rules, unit, max_cost, K):
    """every query against EVERY entry of 1 .. 64 ids: no window of length classes"""
    kept = [(list(s), list(t), c) for s, t, c in rules
            if 1 <= len(s) <= 4 and len(t) <= 4 and 0 <= c <= 4095 and all(0 <= x < V for x in list(s) + list(t))]
    exact = np.full(len(queries), -1, dtype=np.int32)
    found = np.zeros(len(queries), dtype=np.int32)
    cand = np.full((len(queries), K), -1, dtype=np.int32)
    cost = np.full((len(queries), K), -1, dtype=np.int32)
    for q, word in enumerate(queries):
        if not 1 <= len(word) <= 64:
            continue
        near, same = [], []
        for e, entry in enumerate(entries):
            if 1 <= len(entry) <= 64:
                if len(entry) == len(word) and all(x == y and 0 <= x < V for x, y in zip(word, entry)):
                    same.append(e)
                else:
                    w = shortest(word, entry, V, kept, unit)
                    if w <= max_cost:
                        near.append((w, e))
        if same:
            exact[q] = min(same)
        near.sort()
        found[q] = len(near)
        for place, (w, e) in enumerate(near[:K]):
            cand[q, place], cost[q, place] = e, w
    return exact, found, cand, cost


def random_rules(rng, V, per_shape, cost_max):
    """rules of every (src_len, tgt_len) in 1 .. 4 x 0 .. 4 over [0, V)"""
    rules = []
    for s in range(1, 5):
        for t in range(5):
            for _ in range(per_shape):
                rules.append((rng.integers(0, V, s).tolist(), rng.integers(0, V, t).tolist(), int(rng.integers(0, cost_max + 1))))
    return [rules[i] for i in rng.permutation(len(rules))]


def statement(queries, entries, V, rules, unit, max_cost, K, raw=None):
    table, costs = records(rules) if raw is None else raw
    return ratebulk.lexicon_channel_host(*pooled(queries), *ratebulk.lexicon_layout_host(*pooled(entries)), V, table, costs, unit,
                                         max_cost, K)


def same_outputs(got, want):
    for g, w, name in zip(got, want, ("exact", "found", "cand", "cost")):
        assert g.dtype == np.int32 and np.array_equal(g, w), name


def test_lexicon_channel_host_against_a_shortest_path():
    """random words of 1 .. 12 ids over V = 4 (ids -1 and V among them), rules of every shape -- zero costs among them --; the
    budgets around one unit, so that the window of classes is open on one side, on both and on neither"""
    rng = np.random.default_rng(40)
    V = 4
    entries = random_lexicon(rng, V, 90, list(range(1, 13)))
    some = [e for e in entries if 1 <= len(e) <= 12]
    queries = [mutate(rng, some[int(rng.integers(0, len(some)))], V, int(rng.integers(0, 3))) for _ in range(14)]
    queries += [[], [1] * 65, list(some[5])]
    seen, most = set(), 0
    for unit, cost_max, max_cost, per_shape in ((5, 9, 7, 1), (7, 3, 4, 2), (3, 20, 9, 1), (4, 0, 0, 1)):
        rules = random_rules(rng, V, per_shape, cost_max)
        want = brute_channel(queries, entries, V, rules, unit, max_cost, 6)
        same_outputs(statement(queries, entries, V, rules, unit, max_cost, 6), want)
        most = max(most, int(want[1].max()))
        seen.update(want[3].reshape(-1).tolist())
    assert most > 6 and len(seen) > 5 and 0 in seen


def test_the_distances_worked_by_hand():
    ids = dict((c, i + 1) for i, c in enumerate("abcdefghijklmnopqrstuvwxyz"))
    enc = lambda w: [ids[c] for c in w]
    rules = [(enc(s), enc(t), c) for s, t, c in (("m", "rn", 40), ("rn", "m", 35), ("f", "s", 20), ("a", "", 30), ("li", "h", 60),
                                                 ("c", "e", 50))]
    for q, e, w in (("modem", "modern", 40), ("modern", "modem", 35), ("fafe", "sase", 40), ("mm", "rnrn", 80), ("cat", "et", 80),
                    ("lilt", "hlt", 60), ("xxx", "yyy", 384)):
        exact, found, cand, cost = statement([enc(q)], [enc(e)], 27, rules, 128, 4095, 2)
        assert (exact[0], found[0], cand[0].tolist(), cost[0].tolist()) == (-1, 1, [0, -1], [w, -1]), (q, e)
        assert shortest(enc(q), enc(e), 27, rules, 128) == w


def test_without_rules_and_at_unit_one_it_is_lexicon_neighbours_host():
    rng = np.random.default_rng(41)
    V = 3
    entries = random_lexicon(rng, V, 120, [1, 2, 3, 4, 5, 6, 7, 12])
    queries = [rng.integers(-1, V + 1, int(rng.integers(1, 9))).tolist() for _ in range(20)] + [[], [2] * 64, [2] * 65]
    layout = ratebulk.lexicon_layout_host(*pooled(entries))
    for max_dist in range(9):
        want = ratebulk.lexicon_neighbours_host(*pooled(queries), *layout, V, max_dist, 7)
        same_outputs(ratebulk.lexicon_channel_host(*pooled(queries), *layout, V, None, None, 1, max_dist, 7), want)
    same_outputs(want, brute_neighbours(queries, entries, V, 8, 7))


def test_ignored_rules_change_nothing_and_the_order_of_the_rules_neither():
    rng = np.random.default_rng(42)
    V = 4
    entries = random_lexicon(rng, V, 60, list(range(1, 9)))
    queries = [rng.integers(0, V, int(rng.integers(1, 9))).tolist() for _ in range(10)]
    rules = random_rules(rng, V, 1, 6)
    table, costs = records(rules)
    want = statement(queries, entries, V, rules, 5, 8, 5)
    assert not np.array_equal(want[3], statement(queries, entries, V, [], 5, 8, 5)[3])      # (the rules do something)
    # every kind of ignored rule, each of them cheap and wide open were it not ignored; fields behind the used ones are garbage
    bad = np.array([[0, 1, 9, 9, 9, 9, 1, 9, 9, 9], [5, 1, 1, 1, 1, 1, 1, 9, 9, 9], [-1, 0, 1, 9, 9, 9, 9, 9, 9, 9],
                    [1, 5, 1, 9, 9, 9, 1, 1, 1, 1], [1, -1, 1, 9, 9, 9, 9, 9, 9, 9], [1, 1, V, 0, 0, 0, 1, 0, 0, 0],
                    [1, 1, 1, 0, 0, 0, -1, 0, 0, 0], [2, 1, 1, 2 ** 31 - 1, 0, 0, 1, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 0, 0, 0],
                    [1, 0, 2, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    bad_cost = np.array([0, 0, 0, 0, 0, 0, 0, 0, -1, 4096], dtype=np.int32)
    assert ratebulk.channel_rules_kept(bad, bad_cost, V) == []
    mixed = np.concatenate([bad[:5], table, bad[5:]]), np.concatenate([bad_cost[:5], costs, bad_cost[5:]])
    same_outputs(statement(queries, entries, V, None, 5, 8, 5, raw=mixed), want)
    # used ids behind src_len and tgt_len are not looked at
    noisy = table.copy()
    for r in range(len(noisy)):
        noisy[r, 2 + noisy[r, 0]:6] = -7
        noisy[r, 6 + noisy[r, 1]:] = 2 ** 31 - 1
    same_outputs(statement(queries, entries, V, None, 5, 8, 5, raw=(noisy, costs)), want)
    for _ in range(3):
        perm = rng.permutation(len(mixed[1]))
        same_outputs(statement(queries, entries, V, None, 5, 8, 5, raw=(mixed[0][perm], mixed[1][perm])), want)
    for wrong in (dict(V=0), dict(unit=0), dict(unit=4096), dict(max_cost=-1), dict(max_cost=4096), dict(K=0), dict(K=17)):
        a = dict(dict(V=V, unit=5, max_cost=8, K=5), **wrong)
        with pytest.raises(ValueError):
            statement(queries, entries, a["V"], rules, a["unit"], a["max_cost"], a["K"])


def test_the_window_of_classes_is_a_bound_only():
    """rules that lengthen by 3 and shorten by 4, a budget below one unit: the entries 3 and 6 ids longer and 4 and 8 shorter
    are found, a zero-cost rule opens every class"""
    V = 6
    q = [1, 2, 3, 4] * 3
    rules = [([1], [5, 5, 5, 1], 30), ([1, 2, 3, 4], [], 40)]
    entries = [[5, 5, 5, 1, 2, 3, 4] + q[4:], [5, 5, 5, 1, 2, 3, 4] * 2 + q[8:], q[4:], q[8:], q + [0], q[:-1], [5] * 12]
    exact, found, cand, cost = statement([q], entries, V, rules, 100, 99, 8)
    assert (exact[0], found[0]) == (-1, 4) and cand[0, :4].tolist() == [0, 2, 1, 3] and cost[0, :4].tolist() == [30, 40, 60, 80]
    same_outputs((exact, found, cand, cost), brute_channel([q], entries, V, rules, 100, 99, 8))
    free = rules + [([4], [], 0)]
    want = brute_channel([q], entries + [[1, 2, 3]], V, free, 100, 99, 8)
    same_outputs(statement([q], entries + [[1, 2, 3]], V, free, 100, 99, 8), want)
    assert 7 in want[2][0].tolist()


# ---------------------------------------------------------------------------------------------- Channel
def test_rater_channel_costs_drops_and_the_cut():
    r = small_rater(OracleLM, length=LENGTH)
    table = [("ab", "c", 8, 32), ("a", "", 3, 3), ("b", "d", 1, 1000), ("", "a", 5, 5), ("c", "c", 9, 9), ("a?", "b", 5, 5),
             ("abcde", "a", 5, 5), ("a", "bcdef", 5, 5), ("ab", "c", 4, 8), ("d", "e", 2, 100), ("e", "f", 1, 4), ("f", "g", 5, 0),
             ("g", "h", 9, 3)]
    ch = r.channel(iter(table), unit_bits=6.5, min_count=2, min_rate=0.01)
    assert type(ch) is ratebatch.Channel and ch.unit == 104 and len(ch) == 4
    assert ch.dropped == dict(count=2, rate=1, empty=1, same=1, unmapped=1, long=2, duplicate=1, cut=0)
    assert (ch.sources, ch.targets) == (["ab", "a", "d", "g"], ["c", "", "e", "h"])
    # round(16 * -log2(count / occ)): 4 / 8 is one bit (the cheaper of the duplicates), 3 / 3 none, 2 / 100 5.64 bits; a rate
    # above one costs nothing
    assert ch.cost.tolist() == [16, 0, int(round(16 * -np.log2(0.02))), 0] and ch.cost.dtype == np.int32
    ids = r.mapping[0]
    assert ch.rules.dtype == np.int32 and ch.rules.tolist() == [[2, 1, ids["a"], ids["b"], 0, 0, ids["c"], 0, 0, 0],
                                                                [1, 0, ids["a"], 0, 0, 0, 0, 0, 0, 0],
                                                                [1, 1, ids["d"], 0, 0, 0, ids["e"], 0, 0, 0],
                                                                [1, 1, ids["g"], 0, 0, 0, ids["h"], 0, 0, 0]]
    assert ch.same_mapping(r.mapping[0]) and not ch.same_mapping(dict(r.mapping[0]))
    rare = r.channel([("a", "b", 1, 10 ** 90)], min_count=0)
    assert rare.cost.tolist() == [16 * 255]                                # the ceiling of 255 bits
    # beyond 1024 rules: those of largest count, the first among equal ones, in the order given
    letters = "abcdefgh"
    many = [(x + y, z + w, 2 + (n % 3), 50) for n, (x, y, z, w) in
            enumerate((x, y, z, w) for x in letters for y in letters for z in letters[:5] for w in letters[:4]) if x + y != z + w]
    cut = r.channel(many)
    assert len(many) > 1024 == len(cut) and cut.dropped["cut"] == len(many) - 1024
    order = sorted(range(len(many)), key=lambda i: (-many[i][2], i))[:1024]
    assert list(zip(cut.sources, cut.targets)) == [many[i][:2] for i in sorted(order)]
    # a Confusions is read through its own fields
    table = ratebatch.Confusions(np.array([[1, 1, ord("a"), 0, 0, 0, ord("b"), 0, 0, 0], [2, 0, ord("c"), ord("d"), 0, 0, 0, 0, 0, 0]]),
                                 [4, 2], [16, 2], [0, 6, 0, 0], [1], [10])
    got = r.channel(table)
    assert (got.sources, got.targets, got.cost.tolist()) == (["a", "cd"], ["b", ""], [32, 0])
    for wrong in (0.0, 0.03, 256.0):
        with pytest.raises(ValueError):
            r.channel(table, unit_bits=wrong)


def test_lexicon_neighbours_with_a_channel_on_the_double():
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(43)
    lex = r.lexicon(lexicon_words(rng, 300) + ["abed", "ached"])
    ch = r.channel([("e", "c", 10, 40), ("h", "b", 5, 10), ("cl", "d", 3, 4), ("a", "", 2, 64)], unit_bits=6.0)
    words = lexicon_words(rng, 30) + [lex.words[3], "ahed", "", "ab" * 40, lex.words[3]]
    words += words[:7]
    near = r.lexicon_neighbours(iter(words), lex, per_word=5, channel=ch, max_bits=9.0)
    pool, off = pooled([[r.mapping[0].get(c, 0) for c in w] for w in words])
    want = ratebulk.lexicon_channel_host(pool, off, lex.chars, lex.order, lex.class_first, r.voc_size, ch.rules, ch.cost, 96, 144, 5)
    same_outputs((near.exact, near.found, near.index, near.dist), want)
    assert near.bits.dtype == np.float64 and np.array_equal(near.bits[near.dist >= 0], near.dist[near.dist >= 0] / 16.0)
    assert np.isnan(near.bits[near.dist < 0]).all() and near.found.max() > 5
    at = len(words) - 12
    assert near.exact[at] == 3 and near.strings(at + 1)[0] == "abed" and near.dist[at + 1, 0] == 16      # h -> b at 5 / 10: one bit
    assert r.lexicon_neighbours(words, lex).bits is None
    # max_dist is not used with a channel, and the unit budget is the unit's: 6 bits buy one plain edit, not two
    wide = r.lexicon_neighbours(words[:9], lex, max_dist=0, per_word=5, channel=ch, max_bits=9.0)
    assert np.array_equal(wide.index, near.index[:9])
    empty = r.channel([], unit_bits=6.0)
    plain = r.lexicon_neighbours(words, lex, per_word=5, channel=empty, max_bits=6.0)
    unit = r.lexicon_neighbours(words, lex, per_word=5, max_dist=1)
    assert len(empty) == 0 and np.array_equal(plain.index, unit.index) and np.array_equal(plain.dist, np.where(unit.dist < 0, -1, unit.dist * 96))
    none = r.lexicon_neighbours([], lex, per_word=3, channel=ch)
    assert len(none) == 0 and none.bits.shape == (0, 3)
    other = small_rater(OracleLM, length=LENGTH)
    for wrong in (dict(channel=ch, max_bits=-0.1), dict(channel=ch, max_bits=256.0), dict(channel=other.channel([("a", "b", 2, 2)])),
                  dict(channel=[("a", "b", 2, 2)])):
        with pytest.raises(ValueError):
            r.lexicon_neighbours(["ab"], lex, **wrong)


# ---------------------------------------------------------------------------------------------- rescore, correct_words
def flat_rows(rescored):
    """cost [S + C] in `span_windows_host`'s numbering, and span_first, from a call's `Rescored`s"""
    rows, count = [], []
    for one in rescored:
        for s in range(len(one)):
            a, b = int(one.first[s]), int(one.first[s + 1])
            rows += [one.cost0[s]] + one.cost[a:b].tolist()
            count.append(b - a)
    return np.asarray(rows, dtype=np.float64), np.concatenate([[0], np.cumsum(count)]).astype(np.int64)


def prior_is_added(r, texts, edits, contexts, prior, rescoring):
    """`rescore(prior=..)` against the prior-less call on the same edits: the costs are the sums, best and gain
    `span_pick_host`'s over them"""
    plain = r.rescore(texts, edits, contexts, **rescoring)
    same_rescored(r.rescore(texts, edits, contexts, prior=None, **rescoring), plain)
    got = r.rescore(texts, edits, contexts, prior=prior, **rescoring)
    cost, span_first = flat_rows(plain)
    S = len(span_first) - 1
    add = np.zeros(len(cost))
    add[np.arange(int(span_first[-1])) + np.repeat(np.arange(S), np.diff(span_first)) + 1] = np.concatenate([np.asarray(p, dtype=np.float64)
                                                                                                      for p in prior])
    best, gain, total = ratebulk.span_pick_host(cost + add, np.isfinite(cost), span_first, rescoring.get("min_gain", 1.0))
    got_cost, _ = flat_rows(got)
    assert np.array_equal(got_cost, total)
    assert np.array_equal(np.concatenate([one.best for one in got]), best)
    assert np.array_equal(np.concatenate([one.gain for one in got]), gain)
    for one, ref in zip(got, plain):
        assert one.candidates == ref.candidates and np.array_equal(one.cost0, ref.cost0)
    return plain, got


def test_rescore_with_a_prior_on_the_double():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(44)
    edits = []
    for i, text in enumerate(texts):
        for start in range(1, len(text) - 2, 5):
            edits.append((i, start, start + 2, [random_text(rng, int(n)).replace("\n", "a") for n in rng.integers(0, 4, 3)]))
    assert len(edits) > 8
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.5)
    for precision in ("bf16", "split"):
        prior = [rng.integers(0, 80, len(e[3])) / 16.0 for e in edits]
        plain, got = prior_is_added(r, texts, edits, contexts, prior, dict(rescoring, precision=precision))
        changed = sum(int((a.best != b.best).sum()) for a, b in zip(plain, got))
        assert changed > 0                                            # the prior changes choices
    zero = r.rescore(texts, edits, contexts, prior=[[0.0] * len(e[3]) for e in edits], **rescoring)
    same_rescored(zero, r.rescore(texts, edits, contexts, **rescoring))
    bare = r.rescore(texts, edits, contexts, prior=prior, want_costs=False, **rescoring)
    assert all(np.array_equal(a.best, b.best) and a.cost is None for a, b in zip(bare, got))
    assert [len(one) for one in r.rescore(texts, [], contexts, prior=[])] == [0] * len(texts)
    good = [[0.0] * len(e[3]) for e in edits]
    for wrong in (good[:-1], good[:-1] + [good[-1] + [0.0]], [[-0.5] * len(p) for p in good], [[np.inf] * len(p) for p in good],
                  [[np.nan] * len(p) for p in good]):
        with pytest.raises(ValueError):
            r.rescore(texts, edits, contexts, prior=wrong, **rescoring)


def test_word_edits_returns_the_priors_beside_the_edits():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    found, _ = r.suspect_words(texts, contexts, k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    words = sorted(set(w for one, t in zip(found, texts) for w in one.strings(t)))
    table = dict((w, [w + "a", w[::-1]][:n % 3]) for n, w in enumerate(words))
    weights = dict((w, [float(n), n + 0.5][:n % 3]) for n, w in enumerate(words))
    plain = ratebatch.word_edits(found, texts, table)
    edits, prior = ratebatch.word_edits(found, texts, table, priors=weights)
    assert edits == plain and len(prior) == len(edits) > 3
    assert all(p == weights[texts[i][a:b]] for (i, a, b, _), p in zip(edits, prior))
    assert ratebatch.word_edits(found, texts, table, priors=lambda w: weights[w]) == (edits, prior)
    with pytest.raises(ValueError):
        ratebatch.word_edits(found, texts, table, priors={})


def composed_channel(r, texts, contexts, lex, ch, max_bits, per_word, known, weight, rule, rescoring):
    """suspect_words + the weighted statement + word_edits with priors + rescore(prior=..)"""
    found, bits = r.suspect_words(texts, contexts, **rule)
    words = sorted(set(w for one, t in zip(found, texts) for w in one.strings(t)))
    pool, off = pooled([[r.mapping[0].get(c, 0) for c in w] for w in words])
    exact, _, cand, cost = ratebulk.lexicon_channel_host(pool, off, lex.chars, lex.order, lex.class_first, r.voc_size, ch.rules, ch.cost,
                                                         ch.unit, int(round(16 * max_bits)), per_word)
    take = lambda q: known or exact[q] < 0
    table = dict((w, [lex.words[i] for i in cand[q] if i >= 0] if take(q) else []) for q, w in enumerate(words))
    weights = dict((w, [weight * c / 16.0 for c in cost[q] if c >= 0] if take(q) else []) for q, w in enumerate(words))
    edits, prior = ratebatch.word_edits(found, texts, table, priors=weights)
    return found, edits, prior, r.rescore(texts, edits, contexts, prior=prior, **rescoring), bits


def channel_case(r, rng, texts):
    """a lexicon that holds confused forms of the texts' words, and the channel of these confusions"""
    table = [("a", "b", 30, 60), ("c", "ef", 5, 50), ("gh", "d", 4, 8), ("b", "", 3, 90), ("e", "h", 2, 4)]
    ch = r.channel(table, unit_bits=7.0)
    words = sorted(set(w for t in texts for w in t.split() if len(w) > 1))
    entries = []
    for w in words:
        for source, target, _, _ in table:
            if source in w:
                entries.append(w.replace(source, target, 1))
    return r.lexicon(words[::4] + entries + lexicon_words(rng, 200)), ch


def winner_changes(r, texts, lex, contexts, ch, kind):
    """the spans at which the channel's bits change which candidate wins: with no least gain asked, the best candidate of a span
    is the cheapest one, under the model alone (weight 0) and under the sums (weight 2.5) -- the same candidates in both"""
    kind = dict(kind, min_gain=-1e9, per_word=4, channel=ch, max_bits=8.0)
    alone = r.correct_words(texts, lex, contexts, channel_weight=0.0, **kind)[1]
    both = r.correct_words(texts, lex, contexts, channel_weight=2.5, **kind)[1]
    assert all(a.candidates == b.candidates for a, b in zip(alone, both))
    return sum(int(((a.best != b.best) & (a.best >= 0) & (b.best >= 0)).sum()) for a, b in zip(alone, both))


def test_correct_words_with_a_channel_is_the_composed_call():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(45)
    lex, ch = channel_case(r, rng, texts)
    rule = dict(k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.5)
    picks = {}
    for known, weight, precision in ((False, 1.0, "bf16"), (True, 1.0, "split"), (False, 0.0, "bf16"), (False, 2.5, "bf16")):
        found, rescored, bits = r.correct_words(texts, lex, contexts, per_word=4, known=known, precision=precision, channel=ch,
                                                max_bits=8.0, channel_weight=weight, max_dist=0, **dict(rule, **rescoring))
        ref_found, edits, prior, ref_rescored, ref_bits = composed_channel(
            r, texts, contexts, lex, ch, 8.0, 4, known, weight, dict(rule, precision=precision), dict(rescoring, precision=precision))
        assert np.array_equal(bits, ref_bits) and sum(len(one) for one in rescored) == len(edits) > 3
        for one, ref in zip(found, ref_found):
            assert one.spans() == ref.spans()
        same_rescored(rescored, ref_rescored)
        assert (max(max(p) for p in prior) > 0.0) == (weight > 0.0)
        picks[known, weight] = np.concatenate([one.best for one in rescored])
    # the channel's bits enter the choice: with weight 0 the model alone chooses among the same candidates
    assert picks[False, 0.0].shape == picks[False, 2.5].shape and not np.array_equal(picks[False, 0.0], picks[False, 2.5])
    assert winner_changes(r, texts, lex, contexts, ch, dict(rule, **rescoring)) > 0
    for wrong in (dict(channel_weight=-1.0), dict(channel_weight=np.nan), dict(max_bits=300.0)):
        with pytest.raises(ValueError):
            r.correct_words(texts, lex, contexts, channel=ch, **wrong)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_lexicon_with_a_channel(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(46)
    files, texts = [], []
    for i, size in enumerate((60, 80)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
    contexts = [[170], [174]]
    ref = small_rater(OracleLM, length=LENGTH)
    lex, _ = channel_case(ref, rng, texts)
    listing = tmp_path / "words.tsv"
    listing.write_text("".join("%s\n" % w for w in lex.words))
    table = [("a", "b", 30, 60), ("c", "ef", 5, 50), ("gh", "d", 4, 8), ("b", "", 3, 90), ("e", "h", 1, 4)]
    counts = tmp_path / "counts.jsonl"
    counts.write_text("".join(json.dumps({"source": s, "target": t, "count": c, "occ": o, "rate": c / o}) + "\n" for s, t, c, o in table)
                      + "\n")
    options = ["-s", "4", "-k", "2", "--max-prob", "1", "--min-rank", "0", "--min-suspects", "0", "--per-word", "4", "--left", "10",
               "--ahead", "2", "--min-gain", "0.25", "--delimiters", " \n"]
    weighted = ["--channel", str(counts), "--unit-bits", "7", "--max-bits", "8", "--channel-weight", "1.5", "--min-count", "1"]
    base = ["lexicon", "-m", str(model), "--lexicon", str(listing), "--apply"]
    res = CliRunner().invoke(run.cli, base + options + weighted + files)
    assert res.exit_code == 0, res.output
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    ch = ref.channel(table, unit_bits=7.0, min_count=1)
    assert len(ch) == 5
    kind = dict(per_word=4, delimiters=" \n", k=2, max_prob=1.0, min_rank=0, min_suspects=0, left=10, ahead=2, min_gain=0.25, streams=4)
    _, found, _ = ref.correct_words(texts, lex, contexts, channel=ch, max_bits=8.0, channel_weight=1.5, **kind)
    assert sum(len(f) for f in found) > 0
    for line, text, one in zip(lines, texts, found):
        assert line["corrected"] == one.apply(text)
        assert line["rescored"] == [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                                    for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
    # without --channel the command is what it was
    plain = CliRunner().invoke(run.cli, base + options + files)
    _, unweighted, _ = ref.correct_words(texts, lex, contexts, **kind)
    assert plain.exit_code == 0
    assert [json.loads(l)["corrected"] for l in plain.output.strip().split("\n")] == [one.apply(t) for one, t in zip(unweighted, texts)]
    assert plain.output != res.output
    broken = tmp_path / "broken.jsonl"
    broken.write_text('{"source": "a"}\n')
    for wrong in (["--channel", str(tmp_path / "none.jsonl")], ["--channel", str(broken)], ["--channel", str(counts), "--unit-bits", "0"],
                  ["--channel", str(counts), "--max-bits", "256"], ["--channel", str(counts), "--channel-weight", "-1"]):
        assert CliRunner().invoke(run.cli, base + options + wrong + files).exit_code != 0, wrong
