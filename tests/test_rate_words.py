"""`ratebulk.word_bounds_host`, `segments_host`, `segment_select_host`, `Rater.suspect_words`, `Rater.rate_segments`,
`ratebatch.word_edits` and `keraslm-rate words` on the CPU.

The oracle-backed engine double has no `rate_segments`, so the Rater runs `rate_alternatives` / `rate_batch` and the numpy
statements -- argument checking, the per-text split and the command are the product's.  The device kernels are held to the
same statements in test_rate_words_gpu.py."""
import json
import math
import re

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import ALPHABET, random_text, small_rater
from tests.test_rate_suspects import contract_texts

LENGTH = 16


# ---------------------------------------------------------------------------------------------- the numpy statements
def brute_words(texts, delimiters):
    """the words of texts (lists of ids) by re.split on the delimiter class per text, positions mapped back to the corpus"""
    starts, ends, at = [], [], 0
    for ids in texts:
        string = "".join("|" if i in delimiters else "x" for i in ids)
        pos = 0
        for part in re.split(r"(\|+)", string):
            if part and part[0] == "x":
                starts.append(at + pos)
                ends.append(at + pos + len(part))
            pos += len(part)
        at += len(ids)
    return np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)


def test_word_bounds_host_against_re_split():
    V = 6
    delim = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint8)      # ids 1 and 4 separate words; 0 (unmapped) does not
    texts = [[2, 3, 1, 1, 1, 5, 2],        # a run of delimiters
             [1, 4, 2, 2, 4, 1],           # leading and trailing delimiters
             [],                           # an empty text
             [3],                          # single characters: a word, and a delimiter
             [4],
             [2, 5],                       # a text boundary between two non-delimiters: two words
             [5, 0, 3],
             [],
             [7, -1, 1, 600, 0],           # ids outside [0, V) are characters
             [1, 1]]
    corpus = np.asarray([i for t in texts for i in t], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    want = brute_words(texts, {1, 4})
    assert want[0].tolist() == [0, 5, 9, 13, 15, 17, 20, 23] and want[1].tolist() == [2, 7, 11, 14, 17, 20, 22, 25]
    got = ratebulk.word_bounds_host(corpus, offsets, delim)
    assert got[0].dtype == got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # random corpora, text boundaries anywhere
    rng = np.random.default_rng(0)
    for trial in range(20):
        sizes = rng.integers(0, 12, rng.integers(1, 9))
        texts = [rng.integers(-1, V + 2, s).tolist() for s in sizes]
        corpus = np.asarray([i for t in texts for i in t], dtype=np.int32)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        want = brute_words(texts, {1, 4})
        got = ratebulk.word_bounds_host(corpus, offsets, delim)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), trial
    # texts that cover a part of the corpus only: nothing outside [offsets[0], min(n, offsets[-1])) is a character
    corpus = np.full(10, 2, dtype=np.int32)
    got = ratebulk.word_bounds_host(corpus, np.array([3, 5, 14]), delim)
    assert got[0].tolist() == [3, 5] and got[1].tolist() == [5, 10]
    got = ratebulk.word_bounds_host(corpus[:0], np.array([0, 0]), delim)
    assert got[0].shape == got[1].shape == (0,)


def loop_segments(probs, rank, offsets, seg_start, seg_end, max_prob, min_rank):
    """the contract of kl_rate_segments as a plain Python loop per segment and position"""
    n, n_texts = len(probs), len(offsets) - 1
    out = []
    for a, b in zip(seg_start, seg_end):
        a, b = int(a), int(b)
        text = [i for i in range(n_texts) if offsets[i] <= a < offsets[i + 1]]
        count, bits, psum, least, worst, bad = 0, 0.0, 0.0, np.float32(np.inf), -1, 0
        if a >= 0 and b >= a and a < n and text:
            i = text[0]
            for j in range(max(a, int(offsets[i]) + 1), min(b, int(offsets[i + 1]), n)):
                p = probs[j]
                count += 1
                q = float(p)
                bits -= math.log2(q if q > 1e-99 else 1e-99)      # (C's fmax: a NaN compares false and counts as 1e-99)
                psum += q
                if p < least:
                    least, worst = p, j
                if rank is not None and rank[j] >= min_rank and p <= np.float32(max_prob):
                    bad += 1
        out.append((count, bits, psum, least, worst, bad))
    return out


def special_case_inputs():
    """three texts (8, 1 and 9 characters) and an empty one, with the special cases of the contract"""
    nan = np.float32("nan")
    probs = np.array([0.5, 0.25, nan, 0.0, 0.25, 0.125, 0.125, 0.75,      # text 0: a NaN, a 0.0, tied minima at 5 and 6
                      0.3,                                                  # text 1: one character
                      0.9, 0.2, 0.2, 0.7, nan, nan, 0.6, 0.05, 0.4],       # text 3 (text 2 is empty)
                     dtype=np.float32)
    rank = np.array([-1, 1, 2, 5, 0, 2, 1, 0, -1, -1, 3, 0, 1, 4, 2, 0, 2, 1], dtype=np.int32)
    offsets = np.array([0, 8, 9, 9, 18], dtype=np.int64)
    segments = [(1, 5),        # a NaN and a 0.0
                (5, 7),        # tied minima: the first position wins
                (4, 12),       # crosses the end of text 0: clipped to [4, 8)
                (0, 8),        # at the text's first character: n = len - 1
                (8, 9),        # a one-character text: n = 0, +inf, -1
                (13, 15),      # nothing but NaN: +inf, -1, psum NaN
                (9, 18), (10, 12), (11, 17),      # overlap
                (3, 3),        # empty
                (6, 2), (-2, 4), (18, 20), (40, 41)]      # b < a, a < 0, a in no text, a >= n
    seg_start = np.array([a for a, _ in segments], dtype=np.int64)
    seg_end = np.array([b for _, b in segments], dtype=np.int64)
    return probs, rank, offsets, seg_start, seg_end


def test_segments_host_against_a_loop():
    probs, rank, offsets, seg_start, seg_end = special_case_inputs()
    max_prob, min_rank = 0.25, 1
    for with_rank in (rank, None):
        want = loop_segments(probs, with_rank, offsets, seg_start, seg_end, max_prob, min_rank)
        got = ratebulk.segments_host(probs, with_rank, offsets, seg_start, seg_end, max_prob, min_rank)
        assert [a.dtype for a in got] == [np.int32, np.float64, np.float64, np.float32, np.int64, np.int32]
        for s, ref in enumerate(want):
            one = tuple(a[s] for a in got)
            assert one[0] == ref[0] and one[4] == ref[4] and one[5] == ref[5], s
            assert np.float32(one[3]).view(np.uint32) == np.float32(ref[3]).view(np.uint32), s
            assert one[1] == pytest.approx(ref[1], rel=1e-14, abs=0) and one[2] == pytest.approx(ref[2], rel=1e-14, nan_ok=True), s
    n, bits, psum, least, worst, bad = ratebulk.segments_host(probs, rank, offsets, seg_start, seg_end, max_prob, min_rank)
    assert n.tolist() == [4, 2, 4, 7, 0, 2, 8, 2, 6, 0, 0, 0, 0, 0]
    assert 2 * 328.8 < bits[0] < 2 * 329.0 + 5      # the NaN and the 0.0 both hit the 1e-99 clamp: 328.9 bits each
    assert np.isnan(psum[0]) and psum[1] == 0.25
    assert worst.tolist() == [3, 5, 5, 3, -1, -1, 16, 10, 16, -1, -1, -1, -1, -1]
    assert least[4] == np.inf and least[5] == np.inf and np.isnan(psum[5]) and bits[5] > 2 * 328.8
    assert least[1] == np.float32(0.125) and least[3] == 0.0
    assert bad.tolist() == [2, 2, 2, 4, 0, 0, 2, 1, 1, 0, 0, 0, 0, 0]
    assert (ratebulk.segments_host(probs, None, offsets, seg_start, seg_end)[5] == 0).all()
    for wrong in ((0.5, -1), (float("nan"), 0)):
        with pytest.raises(ValueError):
            ratebulk.segments_host(probs, rank, offsets, seg_start, seg_end, *wrong)


def test_segment_select_host_selects_on_equality():
    start = np.arange(8, dtype=np.int64) * 10
    end = start + 5
    n = np.array([3, 2, 3, 4, 0, 3, 3, 3], dtype=np.int32)
    bad = np.array([2, 2, 1, 2, 5, 2, 2, 2], dtype=np.int32)
    bits = np.array([4.5, 9.0, 9.0, 6.0, 9.0, np.nextafter(4.5, 0.0), np.nan, 100.0])
    psum = np.linspace(0, 1, 8)
    least = np.linspace(0, 1, 8).astype(np.float32)
    worst = start + 1
    got = ratebulk.segment_select_host(start, end, n, bits, psum, least, worst, bad, min_n=3, min_bad=2, min_bpc=1.5)
    # 0: equality on all three comparisons; 1: too short; 2: too few suspects; 3: 6.0 bits == 1.5 * 4; 5: one ulp short; 6: NaN
    assert got[0].dtype == np.int64 and got[0].tolist() == [0, 3, 7]
    for field, ref in zip(got[1:], (start, end, n, bits, psum, least, worst, bad)):
        assert field.dtype == ref.dtype and np.array_equal(field, ref[[0, 3, 7]])
    assert ratebulk.segment_select_host(start, end, n, bits, psum, least, worst, bad, 1, 0, 0.0)[0].tolist() == [0, 1, 2, 3, 5, 7]
    for wrong in (dict(min_n=0), dict(min_bad=-1), dict(min_bpc=-0.5), dict(min_bpc=float("nan"))):
        with pytest.raises(ValueError):
            ratebulk.segment_select_host(start, end, n, bits, psum, least, worst, bad, **wrong)


# ---------------------------------------------------------------------------------------------- the Rater on the double
def statements_over(rater, texts, rated, delimiters, max_prob, min_rank, min_suspects, min_bpc, min_chars):
    """the three statements applied to every text's RatedText: [(start, end, n, bits, psum, min, worst, bad)] and the number
    of words there are"""
    table = np.zeros(rater.voc_size, dtype=np.uint8)
    for c in delimiters:
        table[rater.mapping[0][c]] = 1
    out, words = [], 0
    for text, one in zip(texts, rated):
        ids = windows.encode(windows.normalize(text), rater.mapping[0])
        offsets = np.array([0, len(ids)], dtype=np.int64)
        start, end = ratebulk.word_bounds_host(ids, offsets, table)
        words += len(start)
        rec = ratebulk.segments_host(one.probs, one.rank, offsets, start, end, max_prob, min_rank)
        out.append(ratebulk.segment_select_host(start, end, *rec, min_n=min_chars, min_bad=min_suspects, min_bpc=min_bpc)[1:])
    return out, words


def same_words(found, want, exact=True):
    """found[i] is the Words of the records want[i]; returns the number of words"""
    total = 0
    for one, (start, end, n, bits, psum, least, worst, bad) in zip(found, want):
        assert type(one) is ratebatch.Words and len(one) == len(start)
        assert [getattr(one, f).dtype for f in ("start", "length", "n", "bits", "mean_prob", "min_prob", "worst", "suspects")] == \
            [np.int64, np.int32, np.int32, np.float64, np.float64, np.float32, np.int64, np.int32]
        assert np.array_equal(one.start, start) and np.array_equal(one.length, end - start) and np.array_equal(one.n, n)
        assert np.array_equal(one.min_prob.view(np.uint32), least.view(np.uint32))
        assert np.array_equal(one.worst, worst) and np.array_equal(one.suspects, bad)
        if exact:
            assert np.array_equal(one.bits, bits) and np.array_equal(one.mean_prob, psum / n)
        else:
            assert np.allclose(one.bits, bits, rtol=1e-12, atol=0) and np.allclose(one.mean_prob, psum / n, rtol=1e-12, atol=0)
        assert one.spans() == [(int(a), int(b)) for a, b in zip(start, end)]
        total += len(start)
    return total


def quantile_of(rated, q):
    return float(np.quantile(np.concatenate([r.probs[1:] for r in rated]), q))


def test_suspect_words_is_the_statements_over_rate_alternatives():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    rated, bits = r.rate_alternatives(texts, contexts, k=3, streams=4)
    max_prob = quantile_of(rated, 0.3)
    for precision in ("bf16", "split"):
        found, bits2 = r.suspect_words(texts, contexts, k=3, streams=4, max_prob=max_prob, min_rank=1, precision=precision)
        assert np.array_equal(bits2, bits)
        want, words = statements_over(r, texts, rated, " \n", max_prob, 1, 1, 0.0, 1)
        selected = same_words(found, want)
        assert 0 < selected < words, (selected, words)
    assert len(found[0]) == len(found[1]) == 0          # texts without a prediction yield nothing
    # the words as strings: no delimiter inside, delimiters (or the text's ends) around
    for text, one in zip(texts, found):
        for (a, b), word in zip(one.spans(), one.strings(text)):
            assert word == text[a:b] and not set(word) & set(" \n") and len(word) == b - a > 0
            assert (a == 0 or text[a - 1] in " \n") and (b == len(text) or text[b] in " \n")
    # every rule bites: other delimiters, longer words only, more suspects, more bits per character
    everything, _ = r.suspect_words(texts, contexts, k=3, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    assert same_words(everything, statements_over(r, texts, rated, " \n", 1.0, 0, 0, 0.0, 1)[0]) > 0
    for rule in (dict(delimiters="a\n"), dict(min_chars=3), dict(min_suspects=2), dict(min_bits_per_char=3.0)):
        found, _ = r.suspect_words(texts, contexts, k=3, streams=4, max_prob=max_prob, min_rank=1, **rule)
        want, words = statements_over(r, texts, rated, rule.get("delimiters", " \n"), max_prob, 1, rule.get("min_suspects", 1),
                                      rule.get("min_bits_per_char", 0.0), rule.get("min_chars", 1))
        assert 0 < same_words(found, want) < words, rule
    # nothing but texts without a prediction
    found, bits = r.suspect_words(["", "a"])
    assert [len(f) for f in found] == [0, 0] and found[1].bits.shape == (0,) and bits.tolist() == [0.0, 0.0]


def test_words_per_text_cuts_a_corpus_ordered_selection():
    """the split of the device path: records in corpus positions -> one Words per text, positions within the text"""
    from ocrd_keraslm_amd.lib import Rater
    offsets = np.array([0, 5, 5, 6, 20, 20, 31], dtype=np.int64)      # empty texts, a single character, a text without a word
    start = np.array([0, 3, 7, 12, 20, 28], dtype=np.int64)
    end = start + np.array([2, 2, 4, 8, 3, 3])
    n = np.array([1, 2, 4, 8, 2, 3], dtype=np.int32)
    bits = np.arange(6, dtype=np.float64) + 0.5
    psum = np.arange(6, dtype=np.float64) / 4
    least = (np.arange(6) / 8).astype(np.float32)
    worst = np.array([1, 4, 9, 19, 21, -1], dtype=np.int64)
    bad = np.arange(6, dtype=np.int32)
    found = Rater._words_per_text([start, end, n, bits, psum, least, worst, bad], offsets)
    assert [len(f) for f in found] == [2, 0, 0, 2, 0, 2] and all(type(f) is ratebatch.Words for f in found)
    assert found[0].spans() == [(0, 2), (3, 5)] and found[3].spans() == [(1, 5), (6, 14)] and found[5].spans() == [(0, 3), (8, 11)]
    assert found[3].worst.tolist() == [3, 13] and found[5].worst.tolist() == [1, -1] and found[5].suspects.tolist() == [4, 5]
    assert found[3].mean_prob.tolist() == [0.5 / 4, 0.75 / 8] and found[3].bits.tolist() == [2.5, 3.5]
    assert found[3].min_prob.dtype == np.float32 and found[3].length.dtype == np.int32 and found[3].start.dtype == np.int64
    none = Rater._words_per_text([a[:0] for a in (start, end, n, bits, psum, least, worst, bad)], offsets)
    assert [len(f) for f in none] == [0] * 6 and none[0].bits.dtype == np.float64


def test_rate_segments_is_segments_host_over_rate_batch():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    probs, _ = r.rate_batch(texts, contexts, streams=4)
    sizes = [len(t) for t in texts]
    rng = np.random.default_rng(5)
    segments = [(5, 0, sizes[5]), (5, 3, 9), (8, 10, 30), (5, 4, 6), (2, 0, 1), (2, 0, 2), (3, 7, 7), (5, sizes[5] - 1, sizes[5])]
    for _ in range(20):
        i = int(rng.integers(2, len(texts)))
        a = int(rng.integers(0, sizes[i] + 1))
        segments.append((i, a, int(rng.integers(a, sizes[i] + 1))))
    for precision in ("bf16", "split"):
        found = r.rate_segments(texts, segments, contexts, streams=4, precision=precision)
        assert len(found) == len(texts) and all(type(f) is ratebatch.Segments for f in found)
        assert sum(len(f) for f in found) == len(segments) and len(found[0]) == len(found[1]) == 0
        for i, one in enumerate(found):
            mine = [(a, b) for t, a, b in segments if t == i]      # (the order given)
            assert one.spans() == mine
            start, end = np.array([a for a, _ in mine], dtype=np.int64), np.array([b for _, b in mine], dtype=np.int64)
            n, bits, psum, least, worst, bad = ratebulk.segments_host(probs[i], None, [0, sizes[i]], start, end)
            assert np.array_equal(one.n, n) and np.array_equal(one.bits, bits) and np.array_equal(one.worst, worst)
            assert np.array_equal(one.min_prob.view(np.uint32), least.view(np.uint32)) and not one.suspects.any()
            with np.errstate(invalid="ignore"):
                assert np.array_equal(one.mean_prob, np.where(n > 0, psum / np.maximum(n, 1), np.nan), equal_nan=True)
    two = found[2]      # (0, 1): the first character alone; (0, 2): one prediction
    assert two.spans()[:2] == [(0, 1), (0, 2)] and two.n[:2].tolist() == [0, 1] and two.worst[:2].tolist() == [-1, 1]
    assert two.min_prob[0] == np.inf and np.isnan(two.mean_prob[0])
    assert two.bits[0] == 0.0 and two.bits[1] == -np.log2(np.float64(probs[2][1]))
    # the whole text is rate_batch's bits
    assert found[5].bits[0] == pytest.approx(ratebatch.bits_of(probs[5]), rel=1e-12)
    assert [len(f) for f in r.rate_segments(texts, [], contexts)] == [0] * len(texts)
    assert r.rate_segments(["", "a"], [(1, 0, 1), (0, 0, 0)])[1].n.tolist() == [0]


def test_word_edits_feed_rescore():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    found, _ = r.suspect_words(texts, contexts, k=3, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    lexicon = lambda word: [] if len(word) < 2 else [word[::-1], word[:-1]]
    edits = ratebatch.word_edits(found, texts, lexicon)
    assert edits and edits == sorted(edits, key=lambda e: e[:2])
    kept = set((i, a, b) for i, a, b, _ in edits)
    for i, (one, text) in enumerate(zip(found, texts)):
        for (a, b), word in zip(one.spans(), one.strings(text)):
            assert ((i, a, b) in kept) == (a > 0 and len(word) >= 2)      # none at a text's first character, none without candidates
    for i, a, b, cands in edits:
        assert cands == lexicon(texts[i][a:b])
    table = dict((texts[i][a:b], ["ab"]) for i, a, b, _ in edits[:3])
    some = ratebatch.word_edits(found, texts, table)
    assert 3 <= len(some) <= len(edits) and all(c == ["ab"] for _, _, _, c in some)
    rescored = r.rescore(texts, edits, contexts, streams=4, precision="split")
    for i, one in enumerate(rescored):
        assert list(zip(one.starts.tolist(), one.ends.tolist())) == [(a, b) for t, a, b, _ in edits if t == i]
    with pytest.raises(ValueError):
        ratebatch.word_edits(found[:-1], texts, lexicon)


def test_argument_errors():
    r = small_rater(OracleLM, length=LENGTH)
    for wrong in (dict(min_rank=-1), dict(max_prob=float("nan")), dict(precision="f32"), dict(min_suspects=-1), dict(min_chars=0),
                  dict(min_bits_per_char=-1.0), dict(min_bits_per_char=float("nan"))):
        with pytest.raises(ValueError):
            r.suspect_words(["ab cd"], **wrong)
    for k in (0, 9):
        with pytest.raises(AssertionError):
            r.suspect_words(["ab cd"], k=k)
    for wrong in ([(1, 0, 1)], [(-1, 0, 1)], [(0, -1, 2)], [(0, 3, 2)], [(0, 2, 6)]):
        with pytest.raises(ValueError):
            r.rate_segments(["ab cd"], wrong)
    with pytest.raises(ValueError):
        r.rate_segments(["ab cd"], [(0, 0, 2)], precision="f32")
    r.stateful = False
    for precision in ("bf16", "split"):
        with pytest.raises(ValueError):
            r.suspect_words(["ab cd"], precision=precision)
        with pytest.raises(ValueError):
            r.rate_segments(["ab cd"], [(0, 0, 2)], precision=precision)


def test_default_delimiters_are_the_mapped_whitespace():
    r = small_rater(OracleLM, length=LENGTH)
    table = r._delimiter_table(None)
    assert table.dtype == np.uint8 and table.shape == (r.voc_size,)
    assert sorted(r.mapping[1][int(i)] for i in np.nonzero(table)[0]) == sorted(c for c in ALPHABET if c.isspace()) == ["\n", " "]
    # a whitespace character outside the mapping has id 0 and is part of a word; so is an unmapped delimiter
    assert table[0] == 0 and not r._delimiter_table("\t?").any()
    assert np.nonzero(r._delimiter_table("b "))[0].tolist() == sorted([r.mapping[0]["b"], r.mapping[0][" "]])


# ---------------------------------------------------------------------------------------------- command line
def test_cli_words(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("words") == run.COMMAND_ORDER.index("contexts") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(3)
    files, texts = [], []
    for i, size in enumerate((45, 1, 70)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
    contexts = [[170], [174], [178]]
    ref = small_rater(OracleLM, length=LENGTH)
    rated, _ = ref.rate_alternatives(texts, contexts, k=2, streams=2)
    max_prob = quantile_of(rated, 0.3)
    rule = dict(max_prob=max_prob, min_rank=1, min_suspects=1, min_bits_per_char=0.5, min_chars=2)
    res = CliRunner().invoke(run.cli, ["words", "-m", str(model), "-s", "2", "--precision", "split", "-k", "2", "--max-prob",
                                       repr(max_prob), "--min-rank", "1", "--min-suspects", "1", "--min-bits-per-char", "0.5",
                                       "--min-chars", "2", "--delimiters", " \n"] + files)
    assert res.exit_code == 0, res.output
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    found, bits = ref.suspect_words(texts, contexts, delimiters=" \n", k=2, streams=2, precision="split", **rule)
    assert sum(len(f) for f in found) > 0
    for line, text, one, total in zip(lines, texts, found, bits):
        assert line["chars"] == len(text) and line["bits_per_char"] == float(total) / max(len(text) - 1, 1)
        assert len(line["words"]) == len(one)
        for row, a, word, n, b, mean, least, worst, bad in zip(line["words"], one.start, one.strings(text), one.n, one.bits,
                                                                one.mean_prob, one.min_prob, one.worst, one.suspects):
            assert row == [int(a), word, int(n), float(b), float(mean), float(least), int(worst), int(bad)]
            assert n >= 2 and bad >= 1 and b >= 0.5 * n
    assert len(lines[1]["words"]) == 0
    for wrong in (["-k", "0"], ["--min-rank", "-1"], ["--precision", "f32"], ["--min-suspects", "-1"], ["--min-chars", "0"],
                  ["--min-bits-per-char", "-1"]):
        assert CliRunner().invoke(run.cli, ["words", "-m", str(model)] + wrong + files).exit_code != 0
