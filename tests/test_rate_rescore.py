"""`ratebulk.span_windows_host`, `ratebulk.span_pick_host`, `Rater.rescore`, `ratebatch.Rescored`, `ratebatch.confusion_edits` and
`keraslm-rate rescore` on the CPU.

The oracle-backed engine double has no `span_windows`, so the Rater runs the numpy statements of the hypothesis windows and of
the choice, and whole softmaxes summed on the host; the statements are held to brute force here -- every row built on its own
from Python lists, every choice by a loop, every cost from a fresh one-row window over the hypothesis -- and, for spans of one
character with the model's own alternatives, to `Rater.corrections`.  kl_span_windows, kl_span_pick and the device path are held
to the same statements in test_rate_rescore_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import ALPHABET, random_text, small_rater
from tests.test_rate_corrections import LENGTH, SPLIT_BOUND, variant_corpus, wide_rater, wide_texts
from tests.test_rate_suspects import contract_texts

NAMES = ("idx", "ctx", "tgt", "valid")
BETWEEN, LONG, LAST = 5, 7, 8      # texts of `span_corpus`: 7 characters between two empty texts, 50 characters, the last one (3)


def span_corpus(n_ctx):
    """`variant_corpus` with one more empty text behind the text of 7 characters, which then lies between two empty texts:
    sizes 0, 1, 2, 1, 0, 7, 0, 50, 3 and three ids behind the last text"""
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    offsets = np.insert(offsets, 6, offsets[6])
    assert np.diff(offsets).tolist() == [0, 1, 2, 1, 0, 7, 0, 50, 3]
    if text_ctx is not None:
        text_ctx = np.insert(text_ctx, 6, (text_ctx[5] + 7) % 200, axis=0)
    return corpus, offsets, text_ctx


def pack(spans):
    """[(i, g, D, [candidate id lists])] -> the arrays of kl_span_windows: dict of span_text, span_start, span_len, span_first,
    pool, cand_off"""
    cands = [c for _, _, _, cs in spans for c in cs]
    return dict(span_text=np.array([s[0] for s in spans], dtype=np.int32),
                span_start=np.array([s[1] for s in spans], dtype=np.int64),
                span_len=np.array([s[2] for s in spans], dtype=np.int32),
                span_first=np.concatenate([[0], np.cumsum([len(s[3]) for s in spans])]).astype(np.int64),
                pool=np.array([x for c in cands for x in c], dtype=np.int32),
                cand_off=np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64))


def span_cases(corpus, offsets, left, ahead, M, S=None, max_cands=3, seed=3):
    """spans over `span_corpus` as [(i, g, D, candidates)]: every D and m of {0, 1, 2, 5} that M allows, a span without a
    candidate, one at a text's first character, one ending at its text's end with an empty candidate, an insertion at the
    text's end, spans that run past their text, lie in front of it, or name no text, D outside 0 .. M, a candidate longer than
    M, spans in the last text (beyond n_read once the corpus is cut short), spans in the text between two empty texts with a
    candidate equal to what is written and one holding -1, and a hypothesis as long as left, M and ahead allow; then spans
    drawn at random up to S (at most max_cands candidates each).  S = 1: one valid span at the long text's last character."""
    rng = np.random.default_rng(seed)
    x = [int(c) for c in corpus]
    lo5, lo7, hi7, lo8 = int(offsets[BETWEEN]), int(offsets[LONG]), int(offsets[LONG + 1]), int(offsets[LAST])
    other = lambda ids: [v % 9 + 1 for v in ids]
    if S == 1:
        return [(LONG, hi7 - 1, 1, [other(x[hi7 - 1:hi7])])]
    sizes = [d for d in (0, 1, 2, 5) if d <= M]
    spans = []
    for n, D in enumerate(sizes):
        g = lo7 + 9 + 6 * n
        spans.append((LONG, g, D, [other(x[g:g + m]) if m == D else [int(v) for v in rng.integers(1, 10, m)] for m in sizes]))
    two = min(2, M)
    deep = lo7 + min(left, 40) + 2
    spans += [
        (LONG, lo7 + 20, 1, []),                                                  # no candidate
        (BETWEEN, lo5, 1, [other(x[lo5:lo5 + 1])]),                               # at the text's first character
        (BETWEEN, lo5 + 7 - two, two, [[], other(x[lo5 + 7 - two:lo5 + 7])]),     # ends at its text's end: A = 0, m = 0 is none
        (BETWEEN, lo5 + 7, 0, [[3]]),                                             # an insertion at the text's end
        (BETWEEN, lo5 + 7 - two + 1, two, [[4]]),                                 # runs past its text
        (BETWEEN, lo5 - 1, 1, [[4]]), (-1, lo5 + 2, 1, [[4]]), (len(offsets) - 1, lo5 + 2, 1, [[4]]),
        (BETWEEN, lo5 + 2, M + 1, [[4]]), (BETWEEN, lo5 + 2, -1, [[4]]),
        (BETWEEN, lo5 + 2, 1, [[4] * (M + 1), other(x[lo5 + 2:lo5 + 3])]),         # a candidate longer than M
        (LAST, lo8 + 1, 1, [other(x[lo8 + 1:lo8 + 2])]), (LAST, lo8 + 1, 0, [[4]]),
        (BETWEEN, lo5 + 3, 1, [x[lo5 + 3:lo5 + 4], other(x[lo5 + 3:lo5 + 4])]),   # equal to what is written
        (BETWEEN, lo5 + 2, 1, [[-1] * two, [-1], [5] * two][:max_cands]),         # ids of -1
        (LONG, deep, 1, [[int(v) for v in rng.integers(1, 10, M)]]),              # L = left (up to 40), m = M, A = ahead (up to 7)
        (3, int(offsets[3]) + 1, 0, [[2]]), (1, int(offsets[1]), 1, [[2]]),        # texts of one character
    ]
    n_texts = len(offsets) - 1
    while S is not None and len(spans) < S:
        i = int(rng.integers(0, n_texts))
        g = int(rng.integers(int(offsets[i]) - 1, int(offsets[i + 1]) + 2))
        D = int(rng.integers(0, M + 1))
        cands = []
        for _ in range(int(rng.integers(0, max_cands + 1))):
            kind = int(rng.integers(0, 8))
            m = int(rng.integers(0, M + 1))
            cands.append(x[g:g + D] if kind == 0 and g >= 0 else [int(v) for v in rng.integers(-1 if kind == 1 else 1, 10, m)])
        spans.append((i, g, D, cands))
    return spans if S is None else spans[:S]


def brute_span_row(corpus, n_read, offsets, text_ctx, i, g, D, cand, left, ahead, M, T):
    """one row from Python lists (cand None: the text as written): (idx [T], ctx [T][n_ctx], tgt [T], valid, L, A, m)"""
    x, off = [int(c) for c in corpus], [int(o) for o in offsets]
    n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
    rd = lambda p: x[p] if 0 <= p < n_read else 0
    dummy = ([0] * T, [[0] * n_ctx for _ in range(T)], [-1] * T, 0, None, None, None)
    if not (0 <= i < len(off) - 1 and 0 <= D <= M):
        return dummy
    if not (off[i] <= g and g + D <= min(off[i + 1], n_read)):
        return dummy
    L, A = min(left, g - off[i]), min(ahead, off[i + 1] - g - D)
    if L < 1 or D + A < 1:
        return dummy
    w = [rd(g + k) for k in range(D)]
    r = w if cand is None else [int(v) for v in cand]
    if cand is not None and (len(r) > M or any(v < 0 for v in r) or len(r) + A < 1 or r == w):
        return dummy
    q = [rd(g - L + k) for k in range(L)] + r + [rd(g + D + k) for k in range(A)]
    fed = len(q) - 1
    idx = q[:fed] + [0] * (T - fed)
    tgt = [-1] * T
    for t in range(L - 1, fed):
        tgt[t] = q[t + 1]
    ctx = [[int(c) for c in text_ctx[i]] if n_ctx else [] for _ in range(fed)] + [[0] * n_ctx for _ in range(T - fed)]
    return idx, ctx, tgt, 1, L, A, len(r)


def rows_of(spans):
    """[(span, candidate or None)] in the global row order"""
    return [(s, c) for s in spans for c in [None] + list(s[3])]


# ---------------------------------------------------------------------------------------------- the numpy statements
@pytest.mark.parametrize("n_ctx", [0, 2, 3])
def test_span_windows_host_against_brute_force(n_ctx):
    corpus, offsets, text_ctx = span_corpus(n_ctx)
    short = corpus[:int(offsets[-1]) - 2]      # n_read = len(corpus) < offsets[-1]: the last text's end has no ids
    for left, ahead, M, T in ((5, 4, 5, 13), (5, 4, 5, 16), (1, 0, 1, 3), (7, 0, 2, 8), (40, 7, 5, 51)):
        spans = span_cases(corpus, offsets, left, ahead, M, S=60, max_cands=4)
        a = pack(spans)
        N = len(spans) + len(a["cand_off"]) - 1
        for ids in (corpus, short):
            n_read = min(len(ids), int(offsets[-1]))
            got = ratebulk.span_windows_host(ids, offsets, text_ctx, row0=0, rows=N, left=left, ahead=ahead, max_len=M, T=T, **a)
            idx, ctx, tgt, valid = got
            assert idx.shape == tgt.shape == (N, T) and ctx.shape == (N, T, n_ctx) and valid.shape == (N,)
            assert idx.dtype == ctx.dtype == tgt.dtype == valid.dtype == np.int32
            seen = set()
            for b, ((i, g, D, _), cand) in enumerate(rows_of(spans)):
                want = brute_span_row(ids, n_read, offsets, text_ctx, i, g, D, cand, left, ahead, M, T)
                assert idx[b].tolist() == want[0], (left, ahead, M, T, b)
                assert ctx[b].tolist() == want[1], (left, ahead, M, T, b)
                assert tgt[b].tolist() == want[2], (left, ahead, M, T, b)
                assert int(valid[b]) == want[3], (left, ahead, M, T, b)
                seen.add("valid" if want[3] else "invalid")
                if want[3]:
                    L, A, m = want[4:]
                    assert (tgt[b] >= 0).sum() == m + A      # the targets are r and the A characters after the span
                    seen.add("written" if cand is None else "m=%d" % m)
                    seen.add("D=%d" % D)
                    seen.add("L<left" if L < left else "L==left")
                    seen.add("A==0" if A == 0 else "A<ahead" if A < ahead else "A==ahead")
                    if L + m + A - 1 == T:
                        seen.add("full")
                    if i == BETWEEN:
                        seen.add("between")
            sizes = [d for d in (0, 1, 2, 5) if d <= M]
            assert {"valid", "invalid", "written", "L==left", "A==0", "between"} <= seen, seen
            assert set("D=%d" % d for d in sizes if d or ahead) <= seen and set("m=%d" % d for d in sizes if d or ahead) <= seen, seen
            if T == left + ahead + M - 1:
                assert "full" in seen, seen
        # the listed kinds, by the statement itself (the whole corpus): written row and candidates per span
        ok = ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=0, rows=N, left=left, ahead=ahead, max_len=M, T=T, **a)[3]
        at = a["span_first"][:-1] + np.arange(len(spans))
        n = len([d for d in (0, 1, 2, 5) if d <= M])
        assert ok[at[n]] == 1 and at[n + 1] - at[n] == 1                                        # no candidate: one row
        assert not ok[at[n + 1]:at[n + 2]].any()                                              # a text's first character
        assert ok[at[n + 2]] == 1 and ok[at[n + 2] + 1] == 0 and ok[at[n + 2] + 2] == 1          # A = 0: m = 0 is no hypothesis
        assert not ok[at[n + 3]:at[n + 10]].any()      # insertion at the end, past the text, in front of it, no text, bad D
        assert ok[at[n + 10]:at[n + 11]].tolist() == [1, 0, 1]                                  # a candidate longer than M
        assert ok[at[n + 11]:at[n + 13]].tolist() == [1, 1] + [int(ahead > 0)] * 2            # the last text
        cut = ratebulk.span_windows_host(short, offsets, text_ctx, row0=0, rows=N, left=left, ahead=ahead, max_len=M, T=T, **a)
        assert cut[3][at[n + 11]:at[n + 13]].tolist() == [0, 0] + [int(ahead > 0)] * 2         # ... beyond n_read; read as 0
        assert ahead == 0 or ((cut[2][at[n + 12] + 1] >= 0).sum() == 1 + min(ahead, 2) and 0 in cut[2][at[n + 12] + 1])
        assert ok[at[n + 13]:at[n + 14]].tolist() == [1, 0, 1]                                 # equal to what is written
        assert not ok[at[n + 14] + 1:at[n + 14] + 3].any()                                     # ids of -1
        # chunks: any part of the row space is that part of the whole
        whole = ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=0, rows=N, left=left, ahead=ahead, max_len=M, T=T, **a)
        for row0, rows in ((0, 1), (at[3] + 1, 17), (N - 1, 1)):
            part = ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=row0, rows=rows, left=left, ahead=ahead, max_len=M,
                                              T=T, **a)
            assert all(np.array_equal(p, w[row0:row0 + rows]) for p, w in zip(part, whole))
    a = pack(span_cases(corpus, offsets, 5, 4, 2, S=20))
    N = 20 + len(a["cand_off"]) - 1
    for bad in (dict(left=0), dict(ahead=-1), dict(T=9), dict(T=1025), dict(max_len=0), dict(max_len=65), dict(rows=0),
                dict(row0=-1), dict(row0=1), dict(rows=N + 1)):
        args = dict(dict(row0=0, rows=N, left=5, ahead=4, max_len=2, T=10), **bad)
        with pytest.raises(ValueError):
            ratebulk.span_windows_host(corpus, offsets, text_ctx, **dict(a, **args))


def pick_cases(seed=2):
    """ragged spans for the choice: (cost [S + C], valid [S + C], span_first [S + 1]) -- counts 0, 1, 2, 3, 7, 64, 65 and 300,
    ties (the smaller j), invalid written rows, invalid candidates of least cost, NaN and +-inf costs"""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, 3, 7, 64, 65, 300, 0, 5, 5, 5, 5, 4, 4, 3]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S, C = len(counts), int(first[-1])
    cost = np.round(rng.uniform(0.0, 40.0, S + C), 1)      # (one decimal: equal costs occur)
    valid = (rng.uniform(size=S + C) < 0.8).astype(np.int32)
    at = first[:-1] + np.arange(S)
    valid[at] = 1
    cost[at[7] + 1 + 299] = cost[at[7] + 1 + 17] = cost[at[7] + 1:at[8]].min() - 1.0      # a tie across lanes: j = 17
    valid[at[7] + 1 + 299] = valid[at[7] + 1 + 17] = 1
    cost[at[5] + 1 + 63], valid[at[5] + 1 + 63] = -3.0, 1                                   # the last lane alone
    valid[at[9]] = 0                                                                        # an invalid written row
    valid[at[10] + 1:at[11]] = 0                                                            # no valid candidate
    cost[at[11] + 1:at[12]], valid[at[11] + 1:at[12]] = [np.nan, 2.0, np.nan, 2.0, 1e9], 1   # NaN costs are never chosen
    cost[at[12] + 1:at[13]], valid[at[12] + 1:at[13]] = np.nan, 1                           # ... not even alone
    cost[at[13]:at[14]] = [np.nan, 1.0, 2.0, 3.0, 4.0]                                      # a NaN written cost: no gain
    cost[at[14]:at[15]], valid[at[14]:at[15]] = [3.0, np.inf, -np.inf, 0.0, -0.0], [1, 1, 1, 1, 1]
    cost[at[15]:], valid[at[15]:] = [7.0, 9.0, 9.0, 9.0], 1                                 # every candidate reads worse
    return cost, valid, first


def pick_loop(cost, valid, first, min_gain):
    S = len(first) - 1
    best, gain, out = [], [], [c if v else np.inf for c, v in zip(cost, valid)]
    for s in range(S):
        w = int(first[s]) + s
        b, bc = -1, None
        for j in range(int(first[s + 1] - first[s])):
            c = cost[w + 1 + j]
            if valid[w + 1 + j] and c == c and (b < 0 or c < bc):
                b, bc = j, c
        saved = cost[w] - bc if b >= 0 else 0.0
        if valid[w] and b >= 0 and saved >= min_gain:
            best.append(b)
            gain.append(saved)
        else:
            best.append(-1)
            gain.append(0.0)
    return np.array(best, dtype=np.int32), np.array(gain, dtype=np.float64), np.array(out, dtype=np.float64)


def test_span_pick_host_against_a_loop():
    cost, valid, first = pick_cases()
    before = cost.copy()
    with np.errstate(invalid="ignore"):
        for min_gain in (-np.inf, 0.0, 1.0, 12.5, np.inf, np.nan):
            best, gain, out = ratebulk.span_pick_host(cost, valid, first, min_gain)
            assert np.array_equal(cost, before, equal_nan=True)      # (the input is not written to)
            assert best.dtype == np.int32 and gain.dtype == out.dtype == np.float64
            want = pick_loop(cost, valid, first, min_gain)
            assert np.array_equal(best, want[0]), min_gain
            assert np.array_equal(gain.view(np.uint64), want[1].view(np.uint64)), min_gain
            assert np.array_equal(out.view(np.uint64), want[2].view(np.uint64))
            if min_gain == -np.inf:
                assert best[[0, 7, 5, 8, 9, 10, 11, 12, 13, 14, 15]].tolist() == [-1, 17, 63, -1, -1, -1, 1, -1, -1, 1, 0]
                assert gain[15] == -2.0 and gain[14] == np.inf
            if not min_gain < np.inf:      # (only an infinite gain reaches +inf; nothing reaches NaN)
                keeps = [14] if min_gain == np.inf else []
                assert np.nonzero(best != -1)[0].tolist() == keeps and np.nonzero(gain != 0.0)[0].tolist() == keeps
    one = ratebulk.span_pick_host([5.0, 3.0, 3.0], [1, 1, 1], [0, 2], 1.0)
    assert one[0].tolist() == [0] and one[1].tolist() == [2.0]
    for bad in (([1.0], [1], [0]), ([1.0, 2.0], [1, 1], [0, 2]), ([1.0, 2.0], [1, 1], [1, 2])):
        with pytest.raises(ValueError):
            ratebulk.span_pick_host(*bad, min_gain=0.0)


# ---------------------------------------------------------------------------------------------- the Rater on the double
def random_edits(texts, seed, per_text=6, sizes=(0, 1, 2, 3), alphabet=ALPHABET, deep=None):
    """edits over texts of the ten-character alphabet: per text up to per_text spans of 0 .. 3 characters at random places (the
    first character and the text's end among them), each with 0 .. 4 candidates of 0 .. 3 characters -- what is written and an
    unmapped character among them; `deep`: also a span at that position of every text long enough"""
    rng = np.random.default_rng(seed)
    edits = []
    for i, text in enumerate(texts):
        n = len(text)
        places = [0, n] + [int(p) for p in rng.integers(0, n + 1, per_text - 2)] if n else [0]
        if deep is not None and n > deep + 3:
            places.append(deep)
        for start in places:
            D = min(int(rng.choice(sizes)), n - start)
            cands = ["".join(alphabet[int(c)] for c in rng.integers(0, len(alphabet), int(rng.choice(sizes))))
                     for _ in range(int(rng.integers(0, 5)))]
            if cands and rng.uniform() < 0.3:
                cands[0] = text[start:start + D]
            if cands and rng.uniform() < 0.2:
                cands[-1] = cands[-1][:1] + "Z"
            edits.append((i, start, start + D, cands))
    order = rng.permutation(len(edits))      # (the spans of a text need not come together, or in order)
    return [edits[int(j)] for j in order]


def fresh_span_cost(r, text, ctx, start, end, cand, left, ahead):
    """the cost of one reading by definition: text[g-L:g] + r + text[g+D:g+D+A] as a one-row window from a zero state, the bits
    of its last m + A predictions; None where there is no such hypothesis"""
    n = len(text)
    L, A = min(left, start), min(ahead, n - end)
    enc = lambda s: [int(v) for v in windows.encode(s, r.mapping[0])]
    w = enc(text[start:end])
    new = w if cand is None else enc(cand)
    if L < 1 or (end - start) + A < 1 or (cand is not None and (len(new) + A < 1 or new == w)):
        return None
    q = enc(text[start - L:start]) + new + enc(text[end:end + A])
    x = np.array([q[:-1]], dtype=np.int32)
    z = np.tile(np.asarray(windows.clamp_context(ctx), dtype=np.int32)[None, None, :], (1, x.shape[1], 1))
    r.model.reset_states(1)
    full = np.asarray(r.model.forward_window(x, z, want_probs=True), dtype=np.float64)[0]
    return float(-sum(np.log2(max(full[t, q[t + 1]], 1e-99)) for t in range(L - 1, len(q) - 1)))


def check_rescored(found, texts, edits, min_gain, want_costs=True):
    """shapes, dtypes and order of the results; best and gain follow from the returned costs"""
    assert len(found) == len(texts)
    kept = 0
    for i, one in enumerate(found):
        own = [e for e in edits if e[0] == i]
        m = len(own)
        assert isinstance(one, ratebatch.Rescored) and len(one) == m
        assert one.starts.tolist() == [e[1] for e in own] and one.ends.tolist() == [e[2] for e in own]
        assert one.first.tolist() == np.concatenate([[0], np.cumsum([len(e[3]) for e in own])]).tolist()
        assert one.candidates == [windows.normalize(c) for e in own for c in e[3]]
        assert one.starts.dtype == one.ends.dtype == one.first.dtype == np.int64
        assert one.best.dtype == np.int32 and one.gain.dtype == np.float64 and one.best.shape == one.gain.shape == (m,)
        if not want_costs:
            assert one.cost0 is None and one.cost is None
            continue
        assert one.cost0.dtype == one.cost.dtype == np.float64
        assert one.cost0.shape == (m,) and one.cost.shape == (int(one.first[-1]),)
        for j in range(m):
            c = one.cost[int(one.first[j]):int(one.first[j + 1])]
            b, g, _ = pick_loop(np.concatenate([[one.cost0[j]], c]), np.isfinite(np.concatenate([[one.cost0[j]], c])),
                                [0, len(c)], min_gain)
            assert one.best[j] == b[0] and one.gain[j] == g[0]
            kept += int(b[0] >= 0)
        assert one.proposals() == [None if b < 0 else one.candidates[int(a) + int(b)] for a, b in zip(one.first, one.best)]
    return kept


def test_rescore_on_the_double_follows_the_definition():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    ref = small_rater(OracleLM, length=LENGTH)
    left, ahead = 5, 3
    edits = random_edits(texts, seed=4, deep=left + 6)
    assert max(len(e[3]) for e in edits) + 1 > 2      # (a span with more rows than the smallest `streams` below)
    # (streams 1000: everything in one chunk; 6: some spans together, some a chunk of their own; 2: every span alone)
    for streams, precision, min_gain in ((1000, "bf16", 0.25), (6, "split", -np.inf), (2, "bf16", np.inf)):
        found = r.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=min_gain, precision=precision)
        kept = check_rescored(found, texts, edits, min_gain)
        assert (kept > 0) == (min_gain < np.inf)
        seen = {"valid": 0, "invalid": 0, "deep": 0, "first": 0}
        for i, one in enumerate(found):
            for j in range(len(one)):
                start, end = int(one.starts[j]), int(one.ends[j])
                cands = one.candidates[int(one.first[j]):int(one.first[j + 1])]
                got = [one.cost0[j]] + one.cost[int(one.first[j]):int(one.first[j + 1])].tolist()
                seen["deep"] += start > left
                if start == 0:      # no prediction to be held against: all of it +inf, no proposal
                    assert all(c == np.inf for c in got) and one.best[j] == -1 and one.gain[j] == 0.0
                    seen["first"] += 1
                for cand, cost in zip([None] + cands, got):
                    want = fresh_span_cost(ref, texts[i], contexts[i], start, end, cand, left, ahead)
                    if want is None:
                        assert cost == np.inf
                        seen["invalid"] += 1
                    else:
                        assert abs(cost - want) <= 1e-9 * abs(want), (i, j, cand)
                        seen["valid"] += 1
        assert all(seen.values()), seen
        # afterwards: a freshly reset single row
        assert r.model.states[0].shape[0] == 1 and not any(np.asarray(st).any() for st in r.model.states)
    # without the costs: the same choice
    full = r.rescore(texts, edits, contexts, streams=6, left=left, ahead=ahead, min_gain=0.25)
    bare = r.rescore(texts, edits, contexts, streams=6, left=left, ahead=ahead, min_gain=0.25, want_costs=False)
    check_rescored(bare, texts, edits, 0.25, want_costs=False)
    for a, b in zip(full, bare):
        assert np.array_equal(a.best, b.best) and np.array_equal(a.gain, b.gain)


def corrections_as_edits(rater, texts, found):
    """every suspect of `Rater.corrections` as a span of one character with 2k + 1 candidates: the k substitutions, "", and the
    k strings alternative + written.  The unmapped id 0 is written as a character outside the mapping."""
    char = lambda a: rater.mapping[1].get(int(a), "Z")
    edits = []
    for i, (text, one) in enumerate(zip(texts, found)):
        text = windows.normalize(text)
        for j, alts in zip(one.positions, one.alt_ids):
            assert (alts >= 0).all()
            j = int(j)
            edits.append((i, j, j + 1, [char(a) for a in alts] + [""] + [char(a) + text[j] for a in alts]))
    return edits


def test_rescore_equals_corrections_on_the_double():
    """the settings of test_corrections_on_the_double_follow_the_definition, deletions and insertions on"""
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    rated, _ = r.rate_alternatives(texts, contexts, k=3, streams=4)
    median = float(np.median(np.concatenate([x.probs[1:] for x in rated])))
    k, left, ahead = 3, 5, 3
    for streams, precision, max_prob, min_rank in ((16, "bf16", median, 1), (7, "split", 1.0, 0)):
        want, _ = r.corrections(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank, left=left, ahead=ahead,
                                deletions=True, insertions=True, min_gain=-np.inf, precision=precision)
        edits = corrections_as_edits(r, texts, want)
        assert len(edits) >= 10
        found = r.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=-np.inf, precision=precision)
        inf = 0
        for one, cor in zip(found, want):
            cost = np.concatenate([one.cost0[:, None], one.cost.reshape(len(one), 2 * k + 1)], axis=1)
            assert np.array_equal(cost.view(np.uint64), cor.cost.view(np.uint64))
            inf += int(np.isinf(cost).sum())
            # the same choice: variant v >= 1 is candidate v - 1
            _, best, gain = ratebulk.variant_pick_host(cor.cost, np.isfinite(cor.cost))
            assert np.array_equal(one.best, best - 1) and np.array_equal(one.gain, gain)
        assert inf > 0


# ---------------------------------------------------------------------------------------------- helpers and surface
def test_rescored_apply_with_overlapping_proposals():
    #       0123456789
    text = "abcdefghij"
    starts = np.array([1, 2, 6, 6, 9, 4, 10, 10], dtype=np.int64)
    ends = np.array([3, 4, 6, 8, 10, 4, 10, 10], dtype=np.int64)
    first = np.arange(9, dtype=np.int64)
    cands = ["X", "YY", "+", "", "Z", "-", "!", "?"]
    best = np.array([0, 0, 0, 0, -1, 0, 0, 0], dtype=np.int32)
    gain = np.array([2.0, 3.0, 1.0, 1.0, 0.0, 0.5, 0.7, 0.7])
    one = ratebatch.Rescored(starts, ends, first, cands, None, None, best, gain)
    assert one.proposals() == ["X", "YY", "+", "", None, "-", "!", "?"]
    # [2,4) -> YY (gain 3) wins over [1,3); the insertion at 6 and [6,8) do not overlap, the insertion comes first; the insertion
    # at 4 touches [2,4) without overlapping it; of two insertions at 10 the earlier one given is kept
    assert one.apply(text) == "abYY-ef+ij!"
    none = ratebatch.Rescored(starts[:0], ends[:0], first[:1], [], None, None, best[:0], gain[:0])
    assert none.apply(text) == text and none.proposals() == [] and len(none) == 0
    # equal gains: the earlier start
    tie = ratebatch.Rescored(np.array([3, 2], dtype=np.int64), np.array([5, 4], dtype=np.int64), np.arange(3, dtype=np.int64),
                             ["P", "Q"], None, None, np.zeros(2, dtype=np.int32), np.array([1.0, 1.0]))
    assert tie.apply(text) == "abQefghij"


def test_confusion_edits():
    texts = ["aaa rn", "", "nrnrn", "clä"]      # (the last: a + combining diaeresis, one character once normalised)
    rules = [("aa", ["a"]), ("rn", ["m", ""]), ("ä", ["ä", "ae"])]
    edits = ratebatch.confusion_edits(texts, rules)
    assert edits == [(0, 0, 2, ["a"]), (0, 1, 3, ["a"]), (0, 4, 6, ["m", ""]), (2, 1, 3, ["m", ""]), (2, 3, 5, ["m", ""]),
                     (3, 2, 3, ["ä", "ae"])]
    at = [np.array([2, 5]), np.array([], dtype=np.int64), np.array([0, 3]), np.array([0])]
    assert ratebatch.confusion_edits(texts, rules, at=at) == [(0, 1, 3, ["a"]), (0, 4, 6, ["m", ""]), (2, 3, 5, ["m", ""])]
    assert ratebatch.confusion_edits(texts, []) == [] and ratebatch.confusion_edits([], rules) == []
    with pytest.raises(ValueError):
        ratebatch.confusion_edits(texts, [("", ["a"])])
    with pytest.raises(ValueError):
        ratebatch.confusion_edits(texts, rules, at=at[:2])


def test_rescore_edge_inputs_and_errors():
    r = small_rater(OracleLM, length=LENGTH)
    calls = []
    forward = r.model.forward_window
    r.model.forward_window = lambda *a, **k: calls.append(1) or forward(*a, **k)
    # no edits; only spans that cannot hold a prediction: results without a window call
    for texts, edits in ((["abc", ""], []), ([], []), (["", "a", "abc"], [(1, 0, 1, ["b"]), (1, 1, 1, ["c", ""]), (2, 0, 2, ["h"]),
                                                                          (0, 0, 0, ["a"])])):
        for want_costs in (True, False):
            found = r.rescore(texts, edits, want_costs=want_costs)
            check_rescored(found, texts, edits, 1.0, want_costs=want_costs)
            for one in found:
                assert (one.best == -1).all() and (one.gain == 0.0).all()
                assert not want_costs or (np.isinf(one.cost0).all() and np.isinf(one.cost).all())
                assert one.apply("abc") == "abc"
    assert not calls
    assert r.model.states[0].shape[0] == 1
    text = "abcabcabc" * 8
    ok = [(0, 3, 5, ["ab"])]
    for bad in (dict(left=0), dict(ahead=-1), dict(precision="f32"), dict(left=1000, ahead=24),
                dict(edits=[(1, 3, 5, ["a"])]), dict(edits=[(-1, 3, 5, ["a"])]), dict(edits=[(0, 3, 2, ["a"])]),
                dict(edits=[(0, -1, 2, ["a"])]), dict(edits=[(0, 70, 73, ["a"])]), dict(edits=[(0, 3, 68, ["a"])]),
                dict(edits=[(0, 3, 5, ["a" * 65])]), dict(edits=[(0, 3, 5, ["a" * 3])], left=1000, ahead=23)):
        with pytest.raises(ValueError):
            r.rescore([text], **dict(dict(edits=ok), **bad))
    r.rescore([text], [(0, 3, 5, ["ab"])], left=1000, ahead=23)               # (1024 = left + ahead + 2 - 1 is allowed)
    r.rescore([text], [(0, 3, 67, ["a" * 64])], left=8, ahead=2)              # (64 characters are allowed)
    assert calls
    r.stateful = False
    for precision in ("bf16", "split"):
        with pytest.raises(ValueError):
            r.rescore([text], ok, precision=precision)


def test_cli_rescore(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("rescore") == run.COMMAND_ORDER.index("correct") + 1
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
    common = ["rescore", "-m", str(model), "-s", "12", "--precision", "split", "--left", "6", "--ahead", "3", "--min-gain", "0.1"]
    settings = dict(streams=12, left=6, ahead=3, min_gain=0.1, precision="split")

    def check(args, edits):
        found = ref.rescore(texts, edits, contexts, **settings)
        assert sum((f.best != -1).sum() for f in found) > 0
        for extra in ([], ["--apply"]):
            res = CliRunner().invoke(run.cli, common + args + extra + files)
            assert res.exit_code == 0, res.output
            lines = [json.loads(l) for l in res.output.strip().split("\n")]
            assert [l["file"] for l in lines] == files
            for line, text, one in zip(lines, texts, found):
                assert line["chars"] == len(text) and len(line["rescored"]) == len(one)
                for (a, b, written, new, gain), s, e, p, g in zip(line["rescored"], one.starts, one.ends, one.proposals(), one.gain):
                    assert (a, b, written, new, gain) == (int(s), int(e), text[int(s):int(e)], p, float(g))
                assert ("corrected" in line) == bool(extra)
                if extra:
                    assert line["corrected"] == one.apply(text)
        assert any(l["corrected"] != t for l, t in zip(lines, texts))

    # per-file candidate lists
    edits = [e for e in random_edits(texts, seed=8) if e[3]]
    cand = tmp_path / "candidates.jsonl"
    cand.write_text("".join(json.dumps({"file": files[i], "start": a, "end": b, "candidates": c}) + "\n" for i, a, b, c in edits))
    check(["--candidates", str(cand)], edits)
    # a table of confusions, every occurrence; then gated by the suspects below the median probability
    rules = [("a", ["b", "ab", ""]), ("b ", ["d"]), ("cd", ["e", "dc"]), (" ", [""])]
    table = tmp_path / "confusions.tsv"
    table.write_text("".join("\t".join([s] + c) + "\n" for s, c in rules) + "\n")
    check(["--confusions", str(table), "--max-prob", "1", "--min-rank", "0"],
          [e for e in ratebatch.confusion_edits(texts, rules) if e[1] + len(texts[e[0]][e[1]:e[2]]) > 1 or e[2] > 1])
    rated, _ = ref.rate_alternatives(texts, contexts, k=2, streams=12)
    median = float(np.median(np.concatenate([x.probs[1:] for x in rated])))
    sus, _ = ref.suspects(texts, contexts, k=2, streams=12, max_prob=median, min_rank=1, precision="split")
    gated = ratebatch.confusion_edits(texts, rules, at=[s.positions for s in sus])
    assert 0 < len(gated) < len(ratebatch.confusion_edits(texts, rules))
    check(["--confusions", str(table), "-k", "2", "--max-prob", repr(median), "--min-rank", "1"], gated)
    # bad options
    broken = tmp_path / "broken.jsonl"
    broken.write_text(json.dumps({"file": "nowhere.txt", "start": 0, "end": 1, "candidates": ["a"]}) + "\n")
    outside = tmp_path / "outside.jsonl"
    outside.write_text(json.dumps({"file": files[1], "start": 0, "end": 5, "candidates": ["a"]}) + "\n")
    lonely = tmp_path / "lonely.tsv"
    lonely.write_text("a\n")
    for bad in ([], ["--candidates", str(cand), "--confusions", str(table)], ["--candidates", str(broken)],
                ["--candidates", str(outside)], ["--confusions", str(lonely)], ["--candidates", str(tmp_path / "missing")],
                ["--candidates", str(cand), "--left", "0"], ["--candidates", str(cand), "--ahead", "-1"],
                ["--candidates", str(cand), "--left", "1024", "--ahead", "30"], ["--candidates", str(cand), "--precision", "f32"],
                ["--confusions", str(table), "-k", "0"]):
        assert CliRunner().invoke(run.cli, ["rescore", "-m", str(model)] + bad + files).exit_code != 0, bad


# ---------------------------------------------------------------------------------------------- the split-precision contract
RESCORE_SPLIT = dict(streams=64, left=6, ahead=3, min_gain=-np.inf)


def wide_edits(texts):
    """the edits of test_rate_rescore_gpu's rescore tests over `wide_texts`"""
    return random_edits(texts, seed=31, per_text=8, deep=RESCORE_SPLIT["left"] + 5)


def edit_arrays(rater, texts, contexts, edits):
    """what `Rater.rescore` uploads, built on its own: (corpus, offsets, text_ctx, dict of the span arrays, M)"""
    texts = [windows.normalize(t) for t in texts]
    ids = [windows.encode(t, rater.mapping[0]) for t in texts]
    offsets = np.concatenate([[0], np.cumsum([len(a) for a in ids])]).astype(np.int64)
    spans = [(i, int(offsets[i]) + a, b - a, [[int(v) for v in windows.encode(windows.normalize(c), rater.mapping[0])] for c in cs])
             for i, a, b, cs in edits]
    M = max([1] + [s[2] for s in spans] + [len(c) for s in spans for c in s[3]])
    text_ctx = np.asarray([windows.clamp_context(c) for c in contexts], dtype=np.int32).reshape(len(texts), -1)
    return np.concatenate(ids).astype(np.int32), offsets, text_ctx, pack(spans), M


def oracle_span_costs(oracle, texts, contexts, edits, left, ahead):
    """per row of the global numbering: the double's cost (+inf where invalid) and the first-order bound on a split-precision
    cost, 2 * sum over the scored positions of SPLIT_BOUND / (p_oracle * ln 2); all rows in one window call from zero states.
    Returns (cost [N], bound [N], span_first)."""
    corpus, offsets, text_ctx, a, M = edit_arrays(oracle, texts, contexts, edits)
    N = len(edits) + len(a["cand_off"]) - 1
    x, z, y, ok = ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=0, rows=N, left=left, ahead=ahead, max_len=M,
                                             T=max(left + ahead + M - 1, ratebulk.MIN_T), **a)
    oracle.model.reset_states(N)
    full = np.asarray(oracle.model.forward_window(x, z, want_probs=True), dtype=np.float64)
    oracle.model.reset_states(1)
    p = np.take_along_axis(full, np.maximum(y, 0)[:, :, None], axis=2)[:, :, 0]
    scored = y >= 0
    cost = -np.where(scored, np.log2(np.maximum(p, 1e-99)), 0.0).sum(axis=1)
    bound = 2.0 * np.where(scored, SPLIT_BOUND / (np.maximum(p, 1e-99) * np.log(2.0)), 0.0).sum(axis=1)
    cost[ok == 0] = np.inf
    return cost, bound, a["span_first"]


def decided_spans(cost, bound, first):
    """per span: (has a valid candidate, the oracle's best candidate, is its margin over every other valid candidate larger than
    the two rows' bounds together -- then a run whose every cost is within its bound picks the same one)"""
    S = len(first) - 1
    has, best, sure = np.zeros(S, dtype=bool), np.full(S, -1), np.zeros(S, dtype=bool)
    for s in range(S):
        w = int(first[s]) + s
        c, b = cost[w + 1:int(first[s + 1]) + s + 1], bound[w + 1:int(first[s + 1]) + s + 1]
        if not np.isfinite(cost[w]) or not np.isfinite(c).any():
            continue
        has[s] = True
        j = int(np.argmin(c))
        best[s] = j
        others = np.isfinite(c) & (np.arange(len(c)) != j)
        sure[s] = bool((c[others] - c[j] > b[others] + b[j]).all())
    return has, best, sure


def test_rescore_split_contract_edits_keep_the_oracle_within_the_share():
    """the texts, edits and settings of test_rate_rescore_gpu's split-precision test: on the double alone at most a quarter of
    the spans that have a valid candidate have two best candidates too close to call"""
    texts, contexts = wide_texts()
    oracle = wide_rater(OracleLM)
    edits = wide_edits(texts)
    cost, bound, first = oracle_span_costs(oracle, texts, contexts, edits, RESCORE_SPLIT["left"], RESCORE_SPLIT["ahead"])
    has, best, sure = decided_spans(cost, bound, first)
    print("spans %d, with a valid candidate %d, too close to call %d" % (len(edits), has.sum(), (has & ~sure).sum()))
    assert has.sum() >= 15 and (has & ~sure).sum() <= 0.25 * has.sum()
    # the double's own rescore returns these costs
    found = oracle.rescore(texts, edits, contexts, precision="split", **RESCORE_SPLIT)
    got = flat_costs(found, edits)
    assert np.array_equal(np.isinf(got), np.isinf(cost))
    fin = np.isfinite(cost)
    assert (np.abs(got[fin] - cost[fin]) <= 1e-9 * np.abs(cost[fin])).all()


def flat_costs(found, edits):
    """the costs of a `Rater.rescore` result in the global row order of `edits`"""
    taken = [0] * len(found)
    out = []
    for i, _, _, cands in edits:
        one, j = found[i], taken[i]
        taken[i] += 1
        out += [one.cost0[j]] + one.cost[int(one.first[j]):int(one.first[j + 1])].tolist()
    return np.array(out, dtype=np.float64)
