"""`ratebulk.witness_clusters_host`, `ratebulk.witness_pool_host`, `ratebatch.Consensus`, `Rater.consensus` and `keraslm-rate
consensus` on the CPU.

The statement of the clustering is held to a brute force written out here -- covered boundaries painted per text, every witness
read by walking its alignment, a dictionary for equal readings -- and to four invariants on a random corpus; the device kernels
are held to the statement in test_consensus_gpu.py.  The oracle-backed engine double has no `witness_clusters`, so the Rater runs
the numpy statements: normalising, encoding, the rating, the votes, the results and the command are the product's."""
import functools
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_lexicon import pooled
from tests.test_rate_bulk_gpu import random_text, small_rater
from tests.test_witnesses import LENGTH, edited, noisy

NAMES = ("span_text", "span_start", "span_len", "span_first", "cand_src", "cand_off", "votes", "stats")


# ---------------------------------------------------------------------------------------------- inputs
def aligned_host(A, B, max_len, max_dist, join):
    return ratebulk.align_pairs_host(*pooled(A), *pooled(B), max_len, max_dist, join)


def inputs_of(texts, witnesses, max_dist, join, align=aligned_host, base=0):
    """the arguments of `witness_clusters_host` for texts (lists of symbols) and their witnesses (a list of lists of symbols per
    text): every pair aligned by `align`, text i at base + the sizes before it"""
    pairs = [(i, w) for i, readings in enumerate(witnesses) for w in range(len(readings))]
    A, B = [texts[i] for i, _ in pairs], [witnesses[i][w] for i, w in pairs]
    dist, n_spans, spans = align(A, B, max([len(t) for t in A + B] + [0]), max_dist, join)
    pair_first = np.concatenate([[0], np.cumsum([len(readings) for readings in witnesses])]).astype(np.int64)
    text_off = base + np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    return list(pooled(B)) + [dist, n_spans, spans, pair_first, text_off, join]


def syms(string):
    return [ord(c) for c in string]


# ---------------------------------------------------------------------------------------------- the brute force
def read_over(b, spans, u0, u1):
    """what the witness b wrote for text[u0:u1], by walking its alignment: a match copies, a span inside the cluster gives its
    side b.  Returns (the symbols, whether a span lay inside)."""
    out, inside = [], False
    i = j = 0
    for a0, a1, b0, b1 in spans:
        out += [b[j + k] for k in range(a0 - i) if u0 <= i + k < u1]
        assert j + a0 - i == b0
        if u0 <= a0 and a1 <= u1:
            out += b[b0:b1]
            inside = True
        else:
            assert a1 <= u0 or a0 >= u1      # a span lies in one cluster, whole
        i, j = a1, b1
    out += [b[j + k] for k in range(u1 - i) if u0 <= i + k]
    return out, inside


def brute_clusters(texts, witnesses, b_pool, b_off, dist, n_spans, spans, pair_first, text_off, join):
    """per text its clusters [(u0, u1, written votes, [(reading, votes, position of the first in the pool)], dropped as)], all of
    them, and the pairs that are no readings"""
    found, different = [], 0
    for i, text in enumerate(texts):
        n = len(text)
        paint = np.zeros(2 * (n + join + 1) + 1, dtype=bool)      # boundary k at 2 k, character k at 2 k + 1
        mine = []
        for w in range(len(witnesses[i])):
            q = int(pair_first[i]) + w
            if dist[q] < 0:
                different += 1
                continue
            mine.append((w, q, spans[q, :n_spans[q]].tolist()))
            for a0, a1, _, _ in mine[-1][2]:
                paint[2 * a0:2 * (a1 + join) + 1] = True
        edges = np.flatnonzero(np.diff(np.concatenate([[False], paint, [False]]).astype(np.int8)))
        clusters = []
        for lo, hi in zip(edges[::2].tolist(), edges[1::2].tolist()):      # a painted run [lo, hi) in doubled places
            inside = [(a0, a1) for _, _, rows in mine for a0, a1, _, _ in rows if lo <= 2 * a0 < hi]
            u0, u1 = min(a for a, _ in inside), max(a for _, a in inside)
            assert 2 * u0 == lo
            table, agree = {}, 1
            for w, q, rows in mine:
                reading, has = read_over(witnesses[i][w], rows, u0, u1)
                if not has:
                    assert reading == text[u0:u1]
                    agree += 1
                    continue
                first = [r for r in rows if u0 <= r[0] and r[1] <= u1][0]
                table.setdefault(tuple(reading), [0, int(b_off[q]) + first[2] - (first[0] - u0)])[0] += 1
            why = "first" if u0 == 0 else "long" if u1 - u0 > 64 or max(len(r) for r in table) > 64 else None
            clusters.append((u0, u1, agree, [(list(r), v, at) for r, (v, at) in table.items()], why))
        found.append(clusters)
    return found, different


def brute_outputs(found, different, text_off, R):
    span_text, span_len = np.full(R, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32)
    span_start, cand_src = np.full(R, -1, dtype=np.int64), np.full(R, -1, dtype=np.int64)
    span_first, cand_off = np.zeros(R + 1, dtype=np.int64), np.zeros(R + 1, dtype=np.int64)
    votes = np.zeros(2 * R, dtype=np.int32)
    S = C = n_pool = longest = 0
    for i, clusters in enumerate(found):
        for u0, u1, agree, readings, why in clusters:
            if why:
                continue
            span_text[S], span_start[S], span_len[S], span_first[S], votes[S + C] = i, text_off[i] + u0, u1 - u0, C, agree
            for reading, count, at in readings:
                cand_src[C], cand_off[C], votes[S + C + 1] = at, n_pool, count
                n_pool += len(reading)
                C += 1
            S += 1
            longest = max([longest, u1 - u0] + [len(r) for r, _, _ in readings])
    span_first[S], cand_off[C] = C, n_pool
    dropped = [why for clusters in found for _, _, _, _, why in clusters]
    stats = np.array([S, C, n_pool, longest, different, dropped.count("first"), dropped.count("long"), 0], dtype=np.int64)
    return span_text, span_start, span_len, span_first, cand_src, cand_off, votes, stats


def same_outputs(got, want):
    assert [g.dtype for g in got] == [np.int32, np.int64, np.int32, np.int64, np.int64, np.int64, np.int32, np.int64]
    for g, w, name in zip(got, want, NAMES):
        assert g.shape == w.shape and np.array_equal(g, w), name


@functools.lru_cache(maxsize=None)
def random_corpus():
    """the issue's trial: 3000 random texts in batches of one (join, max_dist) each.  Returns [(texts, witnesses, inputs)]."""
    rng = np.random.default_rng(11)
    batches = []
    for join in range(3):
        for max_dist in range(1, 6):
            texts = [rng.integers(0, 3, int(rng.integers(0, 15))).tolist() for _ in range(200)]
            witnesses = [[edited(rng, t, 3, int(rng.integers(0, 5))) for _ in range(int(rng.integers(1, 5)))] for t in texts]
            batches.append((texts, witnesses, inputs_of(texts, witnesses, max_dist, join, base=int(rng.integers(0, 50)))))
    return batches


def test_witness_clusters_host_against_the_brute_force():
    clusters = multi = first = 0
    statuses = set()
    for texts, witnesses, inputs in random_corpus():
        found, different = brute_clusters(texts, witnesses, *inputs)
        got = ratebulk.witness_clusters_host(*inputs)
        same_outputs(got, brute_outputs(found, different, inputs[6], inputs[4].shape[0] * inputs[4].shape[1]))
        every = [c for per in found for c in per]
        clusters += len(every)
        multi += sum(len(c[3]) >= 2 for c in every)
        first += sum(c[4] == "first" for c in every)
        statuses.update(inputs[2].tolist())
    # (the corpus must hold what the test is about)
    assert clusters >= 1000 and multi >= 300 and first >= 300 and statuses == set(range(-1, 5))


def test_the_invariants_on_the_random_corpus():
    """every text and witness behind a symbol of its own -- the alignment is the same one place on, and no cluster is dropped as
    `first` --, and every witness' symbols made its own: each reading is a candidate of its own whose cand_src names the witness,
    so the outputs alone say what every witness reads"""
    checked = 0
    for texts, witnesses, (b_pool, b_off, dist, n_spans, spans, pair_first, text_off, join) in random_corpus():
        texts = [[9] + t for t in texts]
        witnesses = [[[9] + b for b in readings] for readings in witnesses]
        b_pool, b_off = pooled([b for readings in witnesses for b in readings])
        spans = np.where(spans >= 0, spans + 1, spans)
        text_off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
        tag = np.repeat(np.arange(len(b_off) - 1) - np.repeat(pair_first[:-1], np.diff(pair_first)), np.diff(b_off))
        tagged = b_pool + 100 * (tag + 1).astype(np.int32)
        plain = ratebulk.witness_clusters_host(b_pool, b_off, dist, n_spans, spans, pair_first, text_off, join)
        own = ratebulk.witness_clusters_host(tagged, b_off, dist, n_spans, spans, pair_first, text_off, join)
        assert plain[7][5] == plain[7][6] == own[7][5] == own[7][6] == 0
        for name in ("span_text", "span_start", "span_len"):      # the clusters do not depend on the symbols
            assert np.array_equal(plain[NAMES.index(name)], own[NAMES.index(name)])
        S = int(own[7][0])
        for i, text in enumerate(texts):
            accepted = [w for w in range(len(witnesses[i])) if dist[pair_first[i] + w] >= 0]
            mine = [s for s in range(S) if own[0][s] == i]
            u0 = [int(own[1][s] - text_off[i]) for s in mine]
            u1 = [a + int(own[2][s]) for a, s in zip(u0, mine)]
            # 1. ascending with gaps above join, every span in exactly one
            assert all(b0 > a1 + join for a1, b0 in zip(u1, u0[1:]))
            for w in accepted:
                for a0, a1, _, _ in spans[pair_first[i] + w, :n_spans[pair_first[i] + w]].tolist():
                    assert sum(x <= a0 and a1 <= y for x, y in zip(u0, u1)) == 1
            # 2. the text with every cluster replaced by a witness' reading is the witness
            reads = {w: {} for w in accepted}
            for k, s in enumerate(mine):
                by_witness, empty = {}, 0
                for c in range(int(own[3][s]), int(own[3][s + 1])):
                    at, size = int(own[4][c]), int(own[5][c + 1] - own[5][c])
                    if size:
                        by_witness[int(tagged[at]) // 100 - 1] = b_pool[at:at + size].tolist()
                        assert own[6][c + s + 1] == 1
                    else:                                  # (empty readings are equal whoever gives them)
                        empty = int(own[6][c + s + 1])
                with_run = [w for w in accepted if any(u0[k] <= a0 and a1 <= u1[k] for a0, a1, _, _ in
                                                       spans[pair_first[i] + w, :n_spans[pair_first[i] + w]].tolist())]
                for w in with_run:
                    reads[w][k] = by_witness.get(w, [])
                assert set(by_witness) <= set(with_run) and sum(w not in by_witness for w in with_run) == empty
                assert own[6][own[3][s] + s] == 1 + len(accepted) - len(with_run)
            for w in accepted:
                out = list(text)
                for k in reversed(range(len(mine))):
                    if k in reads[w]:
                        out[u0[k]:u1[k]] = reads[w][k]
                assert out == witnesses[i][w], (i, w)
                checked += 1
        # 3. candidates are distinct and none is the written string; 4. the votes sum to 1 plus the accepted witnesses
        for s in range(int(plain[7][0])):
            i = int(plain[0][s])
            at = int(plain[1][s] - text_off[i])
            cands = [tuple(b_pool[plain[4][c]:plain[4][c] + plain[5][c + 1] - plain[5][c]].tolist())
                     for c in range(int(plain[3][s]), int(plain[3][s + 1]))]
            assert len(set(cands)) == len(cands) >= 1 and tuple(texts[i][at:at + plain[2][s]]) not in cands
            accepted = int((dist[pair_first[i]:pair_first[i + 1]] >= 0).sum())
            assert plain[6][plain[3][s] + s:plain[3][s + 1] + s + 1].sum() == 1 + accepted
    assert checked > 4000


# ---------------------------------------------------------------------------------------------- edges by hand
BASE = "abcdefghij"


def edge_cases():
    """[(name, texts, witnesses, max_dist, join)] in symbols: what the device is held to as well"""
    long = list(range(1000, 1070))
    swap = lambda a, b, new: long[:a] + list(range(2000, 2000 + new)) + long[b:]
    many = lambda count: [syms(BASE[:1 + w % 8] + "X" + BASE[2 + w % 8:]) for w in range(count)]
    return [
        ("chain", [syms(BASE)], [[syms("abXXefghij"), syms("abcdYYghij"), syms("abcdefZhij")]], 4, 0),
        ("gaps", [syms(BASE)], [[syms("abXdefghij"), syms("abcdYfghij"), syms("abcdefgZij")]], 4, 1),
        ("same insertion", [syms("abcdef")], [[syms("abcXdef"), syms("abcXdef")]], 2, 0),
        ("other insertion", [syms("abcdef")], [[syms("abcXdef"), syms("abcYdef"), syms("abcdef")]], 2, 0),
        ("at the end", [syms("abcdef")], [[syms("abcdefX")]], 2, 1),
        ("at character 0", [syms("abcdef")], [[syms("Xbcdef"), syms("abcdeY")]], 2, 1),
        ("64 and 65", [long] * 4, [[swap(1, 65, 64)], [swap(1, 66, 65)], [swap(1, 65, 65)], [swap(1, 65, 0), swap(1, 65, 64)]], 70, 0),
        ("all rejected", [syms(BASE), syms("abc")], [[syms("zyxwvu"), syms("zzzzzzzzzz")], [syms("abd")]], 2, 1),
        ("no witnesses", [syms("abc"), syms("abcdef"), []], [[], [syms("abXdef")], []], 2, 1),
        ("64 witnesses", [syms(BASE), syms(BASE)], [many(64), many(3)], 2, 1),
    ]


def run_edge(name):
    case = [c for c in edge_cases() if c[0] == name][0]
    inputs = inputs_of(*case[1:])
    out = ratebulk.witness_clusters_host(*inputs)
    S, C = int(out[7][0]), int(out[7][1])
    spans = [(int(out[0][s]), int(out[1][s] - inputs[6][out[0][s]]), int(out[2][s]), int(out[6][out[3][s] + s])) for s in range(S)]
    cands = [["".join(chr(x) if x < 500 else "?" for x in inputs[0][out[4][c]:out[4][c] + out[5][c + 1] - out[5][c]]), int(out[6][c + s + 1])]
             for s in range(S) for c in range(int(out[3][s]), int(out[3][s + 1]))]
    return spans, cands, out[3][:S + 1].tolist(), out[7].tolist(), inputs, out


def test_edges_by_hand():
    # touching spans of three witnesses chain at join 0: one cluster, every witness read over all of it
    spans, cands, first, stats, _, _ = run_edge("chain")
    assert spans == [(0, 2, 5, 1)] and cands == [["XXefg", 1], ["cdYYg", 1], ["cdefZ", 1]] and stats == [1, 3, 15, 5, 0, 0, 0, 0]
    # a gap of exactly join is one cluster, of join + 1 two
    spans, cands, first, stats, _, _ = run_edge("gaps")
    assert spans == [(0, 2, 3, 2), (0, 7, 1, 3)] and cands == [["Xde", 1], ["cdY", 1], ["Z", 1]] and first == [0, 2, 3]
    # two witnesses insert at the same place: one candidate with two votes, or two
    spans, cands, first, stats, _, out = run_edge("same insertion")
    assert spans == [(0, 3, 0, 1)] and cands == [["X", 2]] and out[4][0] == 3 and stats[:4] == [1, 1, 1, 1]
    spans, cands, first, stats, _, _ = run_edge("other insertion")
    assert spans == [(0, 3, 0, 2)] and cands == [["X", 1], ["Y", 1]]            # (the third witness agrees with the text)
    spans, cands, first, stats, _, _ = run_edge("at the end")
    assert spans == [(0, 6, 0, 1)] and cands == [["X", 1]]
    # a cluster at a text's first character holds no prediction: dropped, the other kept
    spans, cands, first, stats, _, _ = run_edge("at character 0")
    assert spans == [(0, 5, 1, 2)] and cands == [["Y", 1]] and stats == [1, 1, 1, 1, 0, 1, 0, 0]
    # 64 characters as written and read are kept, 65 on either side are long; an empty reading is a candidate
    spans, cands, first, stats, _, _ = run_edge("64 and 65")
    assert spans == [(0, 1, 64, 1), (3, 1, 64, 1)] and [c[1] for c in cands] == [1, 1, 1] and cands[1][0] == ""
    assert stats == [2, 3, 128, 64, 0, 0, 2, 0]
    spans, cands, first, stats, inputs, out = run_edge("all rejected")
    assert inputs[2].tolist() == [-1, -1, 1] and spans == [(1, 2, 1, 1)] and stats[4] == 2
    spans, cands, first, stats, inputs, out = run_edge("no witnesses")
    assert spans == [(1, 2, 1, 1)] and cands == [["X", 1]] and inputs[5].tolist() == [0, 0, 1, 1]
    # behind the used places: -1, and 0 in votes and the offsets
    assert out[0][1:].tolist() == out[2][1:].tolist() == [-1] and out[1][1] == out[4][1] == -1 and out[6].tolist() == [1, 1, 0, 0]
    assert out[3].tolist() == [0, 1, 0] and out[5].tolist() == [0, 1, 0]
    # 64 witnesses are the most: their eight distinct readings in order of the first witness, eight votes each
    spans, cands, first, stats, inputs, out = run_edge("64 witnesses")
    assert spans[0] == (0, 1, 8, 1) and [c[1] for c in cands[:8]] == [8] * 8 and stats[7] == 0 and stats[0] == 2
    assert out[4][:8].tolist() == [10 * w + 1 for w in range(8)]
    # ... and with 65 the text is counted and nothing of it read; its neighbour is as before
    case = edge_cases()[-1]
    more = inputs_of(case[1], [case[2][0] + case[2][0][:1], case[2][1]], 2, 1)
    got = ratebulk.witness_clusters_host(*more)
    assert got[7].tolist()[:2] == [1, 3] and got[7][7] == 1 and got[0][0] == 1 and got[7][4] == 0
    bad = list(more)
    for wrong in ([0, 68, 67], [0, -1, 68], [2, 65, 69]):      # descending, negative, outside: bad texts, never an error
        bad[5] = np.array(wrong, dtype=np.int64)
        assert ratebulk.witness_clusters_host(*bad)[7][7] >= 1


def test_pairs_that_fail_a_check_are_different():
    """spans outside the texts, descending slots, a span count outside 0 .. max_dist, offsets outside the pool: the pair is
    rejected, and its neighbours read as before"""
    rng = np.random.default_rng(12)
    texts = [rng.integers(0, 3, 12).tolist() for _ in range(20)]
    witnesses = [[edited(rng, t, 3, 2), edited(rng, t, 3, 3)] for t in texts]
    inputs = inputs_of(texts, witnesses, 4, 1)
    clean = ratebulk.witness_clusters_host(*inputs)
    dist, n_spans, spans = (x.copy() for x in inputs[2:5])
    assert (dist[::2] >= 0).all() and (n_spans[:16:2] >= 1).all()
    n_spans[0:16:2] = [2, 2, 2, 2, 5, -1, 2, 2]
    spans[0, :2] = [[1, 2, 1, 2], [1, 3, 2, 3]]            # a0 below the last a1
    spans[2, :2] = [[1, 13, 1, 2], [-1, -1, -1, -1]]      # beyond the text
    spans[4, :2] = [[1, 2, 1, 2], [3, 4, 2, 2]]            # b0 == the last b1 is fine, but
    spans[4, 1] = [3, 4, 1, 2]                             # ... below it is not
    spans[6, :2] = [[2, 3, 2, 1], [5, 5, 5, 5]]            # b1 < b0
    spans[12, :2] = [[1, 2, 1, 2], [3, 4, 3, 40]]          # beyond the witness
    spans[14, :2] = [[-2, 2, 1, 2], [3, 4, 3, 4]]
    got = ratebulk.witness_clusters_host(*(inputs[:2] + [dist, n_spans, spans] + inputs[5:]))
    assert got[7][4] == clean[7][4] + 8
    alone = ratebulk.witness_clusters_host(*inputs_of(texts, [[b] if i < 8 else [a, b] for i, (a, b) in enumerate(witnesses)], 4, 1))
    for name in ("span_text", "span_start", "span_len", "span_first", "cand_off"):
        assert np.array_equal(got[NAMES.index(name)][:alone[7][0]], alone[NAMES.index(name)][:alone[7][0]]), name
    off = inputs[1].copy()
    off[1] = off[2] + 1                                     # pair 0 reaches into pair 1, pair 1 descends
    assert ratebulk.witness_clusters_host(*([inputs[0], off] + inputs[2:]))[7][4] >= clean[7][4] + 1
    assert ratebulk.witness_clusters_host(*([inputs[0][:-1]] + inputs[1:]))[7][4] == clean[7][4] + 1
    for wrong in (dict(join=-1), dict(pair_first=inputs[5][:-1]), dict(dist=inputs[2][:-1]), dict(spans=inputs[4][:, :, :3])):
        a = dict(zip(("b_pool", "b_off", "dist", "n_spans", "spans", "pair_first", "text_off", "join"), inputs), **wrong)
        with pytest.raises(ValueError):
            ratebulk.witness_clusters_host(**a)


def test_witness_pool_host():
    b_ids = np.arange(100, 130, dtype=np.int32)
    src = np.array([3, 28, -2, 10, 40], dtype=np.int64)
    off = np.array([0, 2, 6, 9, 9, 11], dtype=np.int64)      # (candidate 3 is empty)
    pool = ratebulk.witness_pool_host(b_ids, src, off, 5, 11)
    assert pool.dtype == np.int32 and pool.tolist() == [103, 104, 128, 129, 0, 0, 0, 0, 100, 0, 0]      # outside reads as 0
    assert ratebulk.witness_pool_host(b_ids, src, off, 2, 6).tolist() == [103, 104, 128, 129, 0, 0]
    assert ratebulk.witness_pool_host(b_ids[:0], src, off, 5, 11).tolist() == [0] * 11
    assert len(ratebulk.witness_pool_host(b_ids, src, off * 0, 5, 0)) == 0
    with pytest.raises(ValueError):
        ratebulk.witness_pool_host(b_ids, src, off, 0, 0)
    with pytest.raises(ValueError):
        ratebulk.witness_pool_host(b_ids, src, off, 6, 11)


# ---------------------------------------------------------------------------------------------- the Rater on the double
RESCORING = dict(streams=4, left=12, ahead=3, min_gain=0.25)


def consensus_corpus(seed, count):
    """eight texts with `count` witnesses each (None: 0 .. 3): near ones, equal ones, one too far, an empty text"""
    rng = np.random.default_rng(seed)
    texts = [random_text(rng, size) for size in (40, 33, 0, 25, 60, 18, 30, 50)]
    witnesses = [[noisy(rng, t, int(rng.integers(0, 4))) if t else "" for _ in range(i % 4 if count is None else count)]
                 for i, t in enumerate(texts)]
    witnesses[5][0] = random_text(rng, 20)
    witnesses[6][0] = texts[6]
    return texts, witnesses, [[170 + i] for i in range(len(texts))]


def same_as_rescored(found, want, costs=True):
    assert len(found) == len(want)
    for one, ref in zip(found, want):
        assert type(one) is ratebatch.Consensus and isinstance(one, ratebatch.Rescored) and one.candidates == ref.candidates
        for name in ("starts", "ends", "first", "best", "gain") + (("cost0", "cost") if costs else ()):
            assert np.array_equal(getattr(one, name), getattr(ref, name)), name
        assert one.starts.dtype == one.first.dtype == np.int64 and one.best.dtype == one.votes.dtype == one.votes0.dtype == np.int32
        assert len(one.votes0) == len(one) and len(one.votes) == len(one.candidates)


def statement_edits(texts, witnesses, max_dist, join, align=aligned_host):
    """`rescore`'s edits, and the votes, from the statement on the normalised strings"""
    texts = [windows.normalize(t) for t in texts]
    witnesses = [[windows.normalize(w) for w in readings] for readings in witnesses]
    inputs = inputs_of([syms(t) for t in texts], [[syms(w) for w in readings] for readings in witnesses], max_dist, join, align=align)
    out = ratebulk.witness_clusters_host(*inputs)
    joined = "".join(w for readings in witnesses for w in readings)
    edits, votes0, votes = [], [], []
    for s in range(int(out[7][0])):
        i = int(out[0][s])
        at = int(out[1][s] - inputs[6][i])
        own = range(int(out[3][s]), int(out[3][s + 1]))
        edits.append((i, at, at + int(out[2][s]), [joined[out[4][c]:out[4][c] + out[5][c + 1] - out[5][c]] for c in own]))
        votes0.append(int(out[6][out[3][s] + s]))
        votes += [int(out[6][c + s + 1]) for c in own]
    return edits, votes0, votes, inputs[2], dict(different=int(out[7][4]), first=int(out[7][5]), long=int(out[7][6]))


def test_consensus_with_one_witness_is_merge_witnesses():
    r = small_rater(OracleLM, length=LENGTH)
    texts, witnesses, contexts = consensus_corpus(6, 1)
    for precision in ("bf16", "split"):
        alignments, rescored, skipped = r.merge_witnesses(texts, witnesses, contexts, max_dist=5, join=1, precision=precision, **RESCORING)
        found, dists, counts = r.consensus(iter(texts), iter(witnesses), contexts, max_dist=5, join=1, vote_bits=0.0, precision=precision,
                                           **RESCORING)
        same_as_rescored(found, rescored)
        assert counts == skipped and skipped["different"] == 1 and sum(len(one) for one in found) > 5
        assert [d.tolist() for d in dists] == [[one.dist for one in per] for per in alignments] and all(d.dtype == np.int32 for d in dists)
        assert all((one.votes0 == 1).all() and (one.votes == 1).all() for one in found)
    bare = r.consensus(texts, witnesses, contexts, max_dist=5, join=1, want_costs=False, **RESCORING)[0]
    same_as_rescored(bare, rescored, costs=False)
    assert all(one.cost0 is None and one.cost is None for one in bare)


def test_consensus_with_three_witnesses_is_rescore_on_the_statements_edits():
    r = small_rater(OracleLM, length=LENGTH)
    for count in (3, None):
        texts, witnesses, contexts = consensus_corpus(7, count)
        edits, votes0, votes, dist, skipped = statement_edits(texts, witnesses, 6, 1)
        assert len(edits) > 8 and (count is None or max(votes) >= 2 or max(votes0) >= 2)
        found, dists, counts = r.consensus(texts, witnesses, contexts, max_dist=6, join=1, **RESCORING)
        same_as_rescored(found, r.rescore(texts, edits, contexts, **RESCORING))
        assert counts == skipped and np.concatenate(dists).tolist() == dist.tolist()
        assert np.concatenate([one.votes0 for one in found]).tolist() == votes0
        assert np.concatenate([one.votes for one in found]).tolist() == votes
        assert [len(d) for d in dists] == [len(w) for w in witnesses]
    # votes: scores are the costs minus vote_bits per vote, the choice is made among the scores
    plain = r.consensus(texts, witnesses, contexts, max_dist=6, join=1, **RESCORING)[0]
    voted = r.consensus(texts, witnesses, contexts, max_dist=6, join=1, vote_bits=1.5, **RESCORING)[0]
    for one, ref in zip(voted, plain):
        assert np.array_equal(one.cost0, ref.cost0 - 1.5 * ref.votes0) and np.array_equal(one.cost, ref.cost - 1.5 * ref.votes)
        for j in range(len(one)):
            own = one.cost[one.first[j]:one.first[j + 1]]
            if np.isfinite(one.cost0[j]) and np.isfinite(own).any() and one.cost0[j] - own.min() >= 0.25:
                assert one.best[j] == int(np.argmin(own)) and one.gain[j] == one.cost0[j] - own.min()
            else:
                assert one.best[j] == -1 and one.gain[j] == 0.0


def test_votes_turn_a_choice():
    """a planted error whose repair the double's model does NOT prefer -- found by rating the repair directly --: three witnesses
    that hold the clean reading leave the text alone at vote_bits 0 and outvote it at 2 bits a vote"""
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(7)
    clean = random_text(rng, 48)
    rescoring = dict(streams=4, left=16, ahead=4, min_gain=0.25)
    planted = None
    for at in range(8, 40):
        wrong = [c for c in "abcdefgh" if c != clean[at]][at % 7]
        text = clean[:at] + wrong + clean[at + 1:]
        direct = r.rescore([text], [(0, at, at + 1, [clean[at]])], **rescoring)[0]
        if direct.best[0] == -1 and 0.0 < direct.cost[0] - direct.cost0[0] < 3.0:
            planted = (at, text, direct)
            break
    assert planted is not None
    at, text, direct = planted
    found, dists, skipped = r.consensus([text], [[clean, clean, text, clean]], **rescoring)
    one = found[0]
    assert dists[0].tolist() == [1, 1, 0, 1] and one.starts.tolist() == [at] and one.candidates == [clean[at]]
    assert one.votes0.tolist() == [2] and one.votes.tolist() == [3] and one.proposals() == [None] and one.apply(text) == text
    assert one.cost0[0] == direct.cost0[0] and one.cost[0] == direct.cost[0]
    one = r.consensus([text], [[clean, clean, text, clean]], vote_bits=3.5, **rescoring)[0][0]
    assert one.proposals() == [clean[at]] and one.apply(text) == clean
    assert one.gain[0] == (direct.cost0[0] - 3.5 * 2) - (direct.cost[0] - 3.5 * 3) >= 0.25


def test_consensus_empty_cases_and_errors(monkeypatch):
    r = small_rater(OracleLM, length=LENGTH)
    rated = []
    inner = r._span_row_costs
    monkeypatch.setattr(r, "_span_row_costs", lambda *args: rated.append(1) or inner(*args))
    found, dists, skipped = r.consensus(["ab", ""], [[], []])
    assert [len(one) for one in found] == [0, 0] and [d.tolist() for d in dists] == [[], []] and skipped == dict(different=0, first=0, long=0)
    assert found[0].first.tolist() == [0] and found[0].proposals() == [] and found[0].apply("ab") == "ab"
    assert r.consensus([], []) == ([], [], dict(different=0, first=0, long=0))
    # pairs, but no cluster to rate: equal readings, a difference at the first character, a witness that is another text
    found, dists, skipped = r.consensus(["abcdef", "abcdef", "abcdef"], [["abcdef"], ["xbcdef"], ["hgfhgfhgf"]], max_dist=3)
    assert [len(one) for one in found] == [0, 0, 0] and [d.tolist() for d in dists] == [[0], [1], [-1]]
    assert skipped == dict(different=1, first=1, long=0) and rated == []
    assert len(r.consensus(["abcdef"], [["abcdxf"]], **RESCORING)[0][0]) == 1 and rated == [1]
    for wrong in (dict(witnesses=[["abd"], []]), dict(max_dist=0), dict(max_dist=256), dict(join=-1), dict(left=0), dict(ahead=-1),
                  dict(precision="f32"), dict(witnesses=[["a" * 4097]]), dict(vote_bits=-0.5), dict(vote_bits=float("nan")),
                  dict(witnesses=[["abd"] * 65]), dict(left=1000, ahead=30), dict(witnesses=[]), dict(texts=["a" * 4097])):
        with pytest.raises(ValueError):
            r.consensus(**dict(dict(texts=["abc"], witnesses=[["abd"]]), **wrong))
    assert len(r.consensus(["abc"], [["abd"] * 64], **RESCORING)[1][0]) == 64
    r.stateful = False
    with pytest.raises(ValueError):
        r.consensus(["abc"], [["abd"]])


# ---------------------------------------------------------------------------------------------- command line
def cli_files(tmp_path, rng):
    dirs = [tmp_path / ("engine%d" % k) for k in range(3)]
    for d in dirs:
        d.mkdir()
    files, texts, readings = [], [], []
    for i, size in enumerate((60, 1, 80)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
        readings.append([])
        for d in (dirs if i != 1 else dirs[1:2]):          # file 1 has a witness in the second directory only
            readings[-1].append(noisy(rng, texts[-1], 3) if size > 1 else texts[-1])
            (d / name.name).write_text(readings[-1][-1])
    return dirs, files, texts, readings


def expected_lines(files, texts, found, dists, sources):
    lines = []
    for i, (name, text, one) in enumerate(zip(files, texts, found)):
        rows = [[int(a), int(b), text[int(a):int(b)], new, float(g), int(v0),
                 [[c, int(v)] for c, v in zip(one.candidates[one.first[j]:one.first[j + 1]], one.votes[one.first[j]:one.first[j + 1]])]]
                for j, (a, b, new, g, v0) in enumerate(zip(one.starts, one.ends, one.proposals(), one.gain, one.votes0))]
        lines.append({"file": name, "chars": len(text), "witnesses": [{"file": p, "dist": int(d)} for p, d in zip(sources[i], dists[i])],
                      "rescored": rows, "corrected": one.apply(text)})
    return lines


def test_cli_consensus(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("consensus") == run.COMMAND_ORDER.index("confusions") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    dirs, files, texts, readings = cli_files(tmp_path, np.random.default_rng(8))
    options = ["-s", "2", "--precision", "split", "--max-dist", "8", "--join", "1", "--left", "10", "--ahead", "2", "--min-gain", "0.25",
               "--vote-bits", "0.75"]
    base = ["consensus", "-m", str(model)]
    witness = [x for d in dirs for x in ("--witness", str(d))]
    res = CliRunner().invoke(run.cli, base + witness + ["--apply"] + options + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    ref = small_rater(OracleLM, length=LENGTH)
    found, dists, skipped = ref.consensus(texts, readings, [[170], [174], [178]], max_dist=8, join=1, vote_bits=0.75, left=10, ahead=2,
                                          min_gain=0.25, streams=2, precision="split")
    assert sum(len(one) for one in found) > 3
    sources = [[str(d / name.rsplit("/", 1)[1]) for d in (dirs if i != 1 else dirs[1:2])] for i, name in enumerate(files)]
    assert [json.loads(l) for l in res.stdout.strip().split("\n")] == expected_lines(files, texts, found, dists, sources)
    assert json.loads(res.stderr.strip().split("\n")[-1]) == skipped
    plain = CliRunner().invoke(run.cli, base + witness[:2] + options + files)
    assert plain.exit_code == 0 and "corrected" not in json.loads(plain.stdout.strip().split("\n")[0])
    assert CliRunner().invoke(run.cli, base + files).exit_code != 0                                         # no --witness
    for wrong in (["--max-dist", "0"], ["--max-dist", "256"], ["--join", "-1"], ["--precision", "f32"], ["--left", "0"], ["--ahead", "-1"],
                  ["--vote-bits", "-1"]):
        assert CliRunner().invoke(run.cli, base + witness[:2] + wrong + files).exit_code != 0, wrong
    long = tmp_path / "long_1800.txt"
    long.write_text("a" * 4097)
    (dirs[0] / long.name).write_text("a" * 4090)
    too_long = CliRunner().invoke(run.cli, base + witness[:2] + options + [str(long)])
    assert too_long.exit_code == 2 and "4096" in too_long.output
