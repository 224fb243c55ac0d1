"""Look-up across word boundaries on the CPU: `ratebulk.lexicon_splits_host`, `ratebatch.Splits`, `ratebatch.join_edits`,
`Rater.lexicon_splits`, `Rater.correct_words(boundaries=True)` and `keraslm-rate lexicon --boundaries`.

The numpy statement of kl_lexicon_splits is held to a brute force over all (split point, entry, entry) triples with the two-row
Levenshtein distance of test_lexicon.py; the device kernel is held to the statement in test_lexicon_splits_gpu.py.  The
oracle-backed engine double has neither `lexicon_splits` nor `lexicon_neighbours`, so the Rater runs the statements -- the
chain around them is the product's, and is held to the same chain written out by hand."""
import json
import re

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.oracle_engine import OracleLM
from tests.test_lexicon import composed, lev, pooled, same_rescored
from tests.test_rate_bulk_gpu import small_rater
from tests.test_rate_suspects import contract_texts

LENGTH = 16


# ---------------------------------------------------------------------------------------------- the numpy statement
def brute_splits(queries, entries, V, max_dist, min_part, K):
    """all (s, left entry, right entry) triples; the distances of a half to every entry are computed once"""
    d = max_dist - 1
    found = np.zeros(len(queries), dtype=np.int32)
    out = np.full((4, len(queries), K), -1, dtype=np.int32)
    usable = [e for e, entry in enumerate(entries) if 1 <= len(entry) <= 64]
    for q, word in enumerate(queries):
        if not 1 <= len(word) <= 64:
            continue
        valid = []
        for s in range(min_part, len(word) - min_part + 1):
            lefts = [(lev(word[:s], entries[e], V), e) for e in usable]
            rights = [(lev(word[s:], entries[e], V), e) for e in usable]
            triples = [(a, b) for a in lefts for b in rights if a[0] <= d and b[0] <= d]
            if triples:
                (da, a), (db, b) = min(triples)      # (a product set: the least pair holds the least of either side)
                if 1 + da + db <= max_dist:
                    valid.append((1 + da + db, max(a, b), s, a, b))
        found[q] = len(valid)
        for place, (total, _, s, a, b) in enumerate(sorted(valid)[:K]):
            out[:, q, place] = s, a, b, total
    return found, out[0], out[1], out[2], out[3]


def test_lexicon_splits_host_against_all_triples():
    """a few hundred small lexicons over 2 .. 6 ids, so that ties are everywhere; ids outside [0, V), duplicates, and entries
    of no ids among them"""
    rng = np.random.default_rng(20)
    seen_dist, seen_found, n_ties = set(), set(), 0
    for trial in range(240):
        V = int(rng.integers(2, 7))
        entries = [rng.integers(-1 if trial % 5 == 0 else 0, V + (trial % 5 == 0), int(rng.integers(0, 5))).tolist()
                   for _ in range(int(rng.integers(1, 9)))]
        entries += [list(e) for e in entries[:2]]
        entries = [entries[i] for i in rng.permutation(len(entries))]
        queries = [rng.integers(0, V, int(rng.integers(0, 8))).tolist() for _ in range(3)]
        queries.append([i for e in (entries[0], entries[-1]) for i in e])      # two entries run together
        max_dist, min_part, K = int(rng.integers(1, 4)), int(rng.integers(1, 3)), int(rng.choice([1, 3, 16]))
        layout = ratebulk.lexicon_layout_host(*pooled(entries))
        if not len(layout[1]):
            continue
        got = ratebulk.lexicon_splits_host(*pooled(queries), *layout, V=V, max_dist=max_dist, min_part=min_part, K=K)
        want = brute_splits(queries, entries, V, max_dist, min_part, K)
        assert [a.dtype for a in got] == [np.int32] * 5 and got[1].shape == (len(queries), K)
        for g, w, name in zip(got, want, ("found", "split", "left", "right", "dist")):
            assert np.array_equal(g, w), (trial, name, max_dist, min_part, K)
        seen_dist.update(got[4].reshape(-1).tolist())
        seen_found.update(got[0].tolist())
        n_ties += int(((got[4][:, 1:] == got[4][:, :-1]) & (got[4][:, 1:] > 0)).sum())
    assert seen_dist == {-1, 1, 2, 3} and {0, 1, 2, 3} <= seen_found and n_ties > 20


def ids(word):
    return [ord(c) - ord("a") for c in word]


def splits_of(words, entries, max_dist=1, min_part=2, K=4, V=26):
    layout = ratebulk.lexicon_layout_host(*pooled([e if isinstance(e, list) else ids(e) for e in entries]))
    return ratebulk.lexicon_splits_host(*pooled([w if isinstance(w, list) else ids(w) for w in words]), *layout, V=V,
                                        max_dist=max_dist, min_part=min_part, K=K)


def test_hand_made_splits():
    # `ofthe`: the one place, the two entries, one edit -- `other` is what the neighbours answer
    found, split, left, right, dist = splits_of(["ofthe"], ["the", "of", "other", "off"])
    assert found.tolist() == [1] and split[0].tolist() == [2, -1, -1, -1] and left[0, 0] == 1 and right[0, 0] == 0
    assert dist[0].tolist() == [1, -1, -1, -1]
    # a half at distance exactly d and one at d + 1; both halves at d, which is beyond the budget of the whole
    words = ["ofthx", "ofxhx", "xfthx"]
    found, split, left, right, dist = splits_of(words, ["the", "of"], max_dist=2)
    assert found.tolist() == [1, 0, 0] and (split[0, 0], left[0, 0], right[0, 0], dist[0, 0]) == (2, 1, 0, 2)
    assert (split[1:] == -1).all() and (dist[1:] == -1).all()
    found, split, left, right, dist = splits_of(words, ["the", "of"], max_dist=3)
    assert found.tolist() == [1, 1, 1] and dist[:, 0].tolist() == [2, 3, 3]
    assert not splits_of(words, ["the", "of"], max_dist=1)[0].any()
    # ties: the smallest index of a side (duplicates are separate entries), then the larger index of the pair, then s
    entries = ["aa", "a", "aaa", "aa", "a"]
    found, split, left, right, dist = splits_of(["aaaa"], entries, min_part=1)
    assert found.tolist() == [3] and split[0].tolist() == [2, 1, 3, -1]
    assert left[0].tolist() == [0, 1, 2, -1] and right[0].tolist() == [0, 2, 1, -1] and dist[0].tolist() == [1, 1, 1, -1]
    found, split, left, right, dist = splits_of(["aaaa"], entries, min_part=1, K=2)
    assert found.tolist() == [3] and split[0].tolist() == [2, 1]
    # the nearer pair comes first whatever its indices are
    found, split, left, right, dist = splits_of(["aaaab"], ["aa", "a", "aaa", "zz", "zz", "zz", "ab"], max_dist=2, min_part=1)
    assert dist[0].tolist() == [1, 2, 2, -1] and (split[0, 0], left[0, 0], right[0, 0]) == (3, 2, 6) and found[0] == 3
    # min_part keeps single letters out; a word shorter than two parts has no place
    found, split, left, right, dist = splits_of(["aaaa", "aaa", "a", []], entries, min_part=2)
    assert found.tolist() == [1, 0, 0, 0] and split[0].tolist() == [2, -1, -1, -1] and (split[1:] == -1).all()
    assert splits_of(["ab" * 32], ["ab" * 16], min_part=32)[0].tolist() == [1]
    assert splits_of(["ab" * 32 + "a"], ["ab" * 16], min_part=1)[0].tolist() == [0]      # 65 ids
    # ids outside [0, V) equal nothing, themselves included
    V = 26
    found, split, left, right, dist = splits_of([[V, 1] + ids("the"), [-1, 1] + ids("the")], [[V, 1], ids("the"), [0, 1]], V=V)
    assert found.tolist() == [0, 0]
    found, split, left, right, dist = splits_of([[V, 1] + ids("the")], [[V, 1], ids("the"), [0, 1]], max_dist=2, V=V)
    assert found.tolist() == [1] and (left[0, 0], right[0, 0], dist[0, 0]) == (0, 1, 2)
    for wrong in (dict(max_dist=0), dict(max_dist=9), dict(min_part=0), dict(min_part=33), dict(K=0), dict(K=17), dict(V=0)):
        with pytest.raises(ValueError):
            splits_of(["ofthe"], ["of", "the"], **wrong)


# ---------------------------------------------------------------------------------------------- join_edits
def words_at(spans):
    n = len(spans)
    zeros = np.zeros(n)
    return ratebatch.Words(np.asarray([a for a, _ in spans], dtype=np.int64), np.asarray([b - a for a, b in spans], dtype=np.int32),
                           zeros.astype(np.int32), zeros, zeros, zeros.astype(np.float32), zeros.astype(np.int64), zeros.astype(np.int32))


def test_join_edits_on_hand_made_texts():
    delimiter_of = lambda c: c in " \n"
    join = lambda spans, text, **more: ratebatch.join_edits([words_at(spans)], [text], delimiter_of, **more)
    assert join([(3, 7)], "to gether we") == []                                  # a pair at the text's start
    assert join([(6, 12)], "so to gether we") == [(0, 3, 12, "together"), (0, 6, 15, "getherwe")]
    assert join([(3, 5)], "so to gether we") == [(0, 3, 12, "together")]         # "so to" begins at the first character
    assert join([(3, 5), (6, 12)], "so to gether we") == [(0, 3, 12, "together"), (0, 6, 15, "getherwe")]      # one edit per pair
    assert join([(4, 6)], "ab  cd  ef") == []                                    # two delimiters between the words
    assert join([(3, 5)], "ab\ncd\nef") == []                                    # a delimiter that is not the joiner
    assert join([(3, 5)], "ab\ncd\nef", joiner="\n") == [(0, 3, 8, "cdef")]
    assert join([(3, 5)], "ab cd") == [] and join([(0, 2)], "ab cd") == [] and join([(1, 3)], " ab") == []
    assert join([(3, 5), (6, 8)], "ab cd ef", only=lambda word: word == "ef") == [(0, 3, 8, "cdef")]
    assert join([(3, 5), (6, 8)], "ab cd ef", only=lambda word: False) == []
    # the longest span `rescore` takes is 64 characters
    assert join([(2, 33)], "x " + "a" * 31 + " " + "b" * 32) == [(0, 2, 66, "a" * 31 + "b" * 32)]
    assert join([(2, 33)], "x " + "a" * 31 + " " + "b" * 33) == []
    # several texts, ordered by text and start
    found = [words_at([(6, 8)]), words_at([]), words_at([(2, 3), (4, 5)])]
    assert ratebatch.join_edits(found, ["ab cd ef gh", "", "x a b c"], delimiter_of) == \
        [(0, 3, 8, "cdef"), (0, 6, 11, "efgh"), (2, 2, 5, "ab"), (2, 4, 7, "bc")]
    with pytest.raises(ValueError):
        ratebatch.join_edits(found, ["ab"], delimiter_of)


# ---------------------------------------------------------------------------------------------- the Rater on the double
ENTRIES = ["bad", "cab", "head", "face", "deaf", "bead", "he", "ad", "a", "fee", "feed", "ahead", "decade", "gag", "cafe"]
TEXTS = ["a badcab ahe ad face", "he ad\nbe ad gagcafe a", "", "fee d hea d", "facedeaf\nbadc ab beadfeed dec ade a"]


def test_rater_lexicon_splits_on_the_double():
    r = small_rater(OracleLM, length=LENGTH)
    lex = r.lexicon(ENTRIES)
    words = ["badcab", "bad", "gagcafe", "", "hxadfee", "badcab", "a?cab", "ab" * 40, "aa"]
    splits = r.lexicon_splits(iter(words), lex, max_dist=2, min_part=1, per_word=3)
    assert type(splits) is ratebatch.Splits and len(splits) == len(words)
    pool, off = pooled([[r.mapping[0].get(c, 0) for c in w] for w in words])
    want = ratebulk.lexicon_splits_host(pool, off, lex.chars, lex.order, lex.class_first, r.voc_size, 2, 1, 3)
    for got, ref in zip((splits.found, splits.at, splits.left, splits.right, splits.dist), want):
        assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert splits.strings(0)[0] == "bad cab" == splits.strings(5)[0] and splits.dist[0, 0] == 1 and splits.at[0, 0] == 3
    assert splits.strings(0, joiner="\n")[0] == "bad\ncab" and splits.strings(3) == [] and splits.found[7] == 0
    assert splits.strings(4)[0] == "head fee" and splits.dist[4, 0] == 2 and splits.strings(1) == ["a ad"]
    assert splits.strings(8) == ["a a"] and r.lexicon_splits(["aa"], lex).found.tolist() == [0]      # (min_part 2 by default)
    none = r.lexicon_splits([], lex, per_word=2)
    assert len(none) == 0 and none.at.shape == (0, 2) and none.found.dtype == np.int32
    none = r.lexicon_splits(["badcab"], r.lexicon([""]), per_word=2)
    assert none.found.tolist() == [0] and (none.at == -1).all() and (none.dist == -1).all()
    for wrong in (dict(max_dist=0), dict(max_dist=9), dict(min_part=0), dict(min_part=33), dict(per_word=0), dict(per_word=17)):
        with pytest.raises(ValueError):
            r.lexicon_splits(["badcab"], lex, **wrong)
    with pytest.raises(ValueError):
        r.lexicon_splits(["badcab"], ENTRIES)


def chain_by_hand(r, texts, contexts, lex, max_dist, per_word, known, min_part, rule, rescoring, joiner=" "):
    """correct_words(boundaries=True) written out: suspect_words, the three look-ups through the host statements, the
    candidates and the pairs found here from the texts themselves, rescore"""
    found, bits = r.suspect_words(texts, contexts, **rule)
    encoded = lambda strings: pooled([[r.mapping[0].get(c, 0) for c in w] for w in strings])
    layout = (lex.chars, lex.order, lex.class_first, r.voc_size)
    words = sorted(set(w for one, t in zip(found, texts) for w in one.strings(t)))
    exact, _, cand, _ = ratebulk.lexicon_neighbours_host(*encoded(words), *layout, max_dist, per_word)
    looked = dict((w, bool(known or exact[q] < 0)) for q, w in enumerate(words))
    table = dict((w, [lex.words[i] for i in cand[q] if i >= 0] if looked[w] else []) for q, w in enumerate(words))
    apart = [w for w in words if looked[w] and len(w) < 64]
    if apart:
        _, _, left, right, _ = ratebulk.lexicon_splits_host(*encoded(apart), *layout, max_dist, min_part, per_word)
        for q, w in enumerate(apart):
            for a, b in zip(left[q], right[q]):
                string = lex.words[a] + joiner + lex.words[b] if a >= 0 else None
                if string is not None and string not in table[w] and len(string) <= 64:
                    table[w].append(string)
    edits = ratebatch.word_edits(found, texts, table)
    pairs = []
    for i, (one, text) in enumerate(zip(found, texts)):
        chosen = set(one.spans())
        tokens = [(t.start(), t.end()) for t in re.finditer(r"[^ \n]+", text)]
        for (a, b), (c, e) in zip(tokens, tokens[1:]):
            mine = ((a, b) in chosen and looked[text[a:b]]) or ((c, e) in chosen and looked[text[c:e]])
            if c == b + 1 and text[b] == joiner and mine and a >= 1 and e - a <= 64:
                pairs.append((i, a, e, text[a:b] + text[c:e]))
    if pairs:
        exact, _, cand, _ = ratebulk.lexicon_neighbours_host(*encoded([p[3] for p in pairs]), *layout, max_dist - 1, per_word)
        for q, (i, a, e, _) in enumerate(pairs):
            strings = [lex.words[j] for j in [exact[q]] + cand[q].tolist() if j >= 0]
            if strings:
                edits.append((i, a, e, strings))
    edits.sort(key=lambda e: e[:3])
    return found, edits, r.rescore(texts, edits, contexts, **rescoring), bits


RULE = dict(k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)      # (every word is selected)
RESCORING = dict(streams=4, left=12, ahead=3, min_gain=0.5)


def test_correct_words_with_boundaries_is_the_chain_by_hand():
    r = small_rater(OracleLM, length=LENGTH)
    lex = r.lexicon(ENTRIES)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    sizes = {}
    for known, max_dist, min_part in ((False, 1, 2), (True, 2, 1), (False, 2, 3)):
        found, rescored, bits = r.correct_words(TEXTS, lex, contexts, max_dist=max_dist, per_word=4, known=known, boundaries=True,
                                                min_part=min_part, **dict(RULE, **RESCORING))
        ref_found, edits, ref_rescored, ref_bits = chain_by_hand(r, TEXTS, contexts, lex, max_dist, 4, known, min_part, RULE, RESCORING)
        assert np.array_equal(bits, ref_bits) and [one.spans() for one in found] == [one.spans() for one in ref_found]
        same_rescored(rescored, ref_rescored)
        assert sum(len(one) for one in rescored) == len(edits) > 0
        by_span = dict(((i, a, b), c) for i, a, b, c in edits)
        sizes[known, max_dist, min_part] = len(edits)
        # `badcab` gets its split, `he ad` is one word to the pair's edit, and both of a pair's words are one edit
        assert "bad cab" in by_span[0, 2, 8] and by_span[1, 6, 11][:1] == ["bead"] and (1, 0, 5) not in by_span      # (starts at 0)
        assert by_span[0, 9, 15][0] == "ahead" and (by_span[3, 6, 11][0] == "head") and len([e for e in edits if e[:3] == (0, 9, 15)]) == 1
        assert by_span[4, 26, 33][0] == "decade"
        if min_part == 3:
            assert "gag cafe" in by_span[1, 12, 19] and "a head" not in by_span.get((0, 9, 12), [])
        assert edits == sorted(edits, key=lambda e: e[:3])
        # an entry is left alone by default: no split of `ahead` into `a head`, no pair that holds only entries
        assert known or (0, 16, 20) not in by_span
    assert sizes[True, 2, 1] > sizes[False, 2, 3]
    # overlapping spans are `apply`'s business: the result is a text again
    assert isinstance(rescored[0].apply(TEXTS[0]), str)
    # max_dist 0 leaves no edit for a delimiter: the flag changes nothing
    plain = r.correct_words(TEXTS, lex, contexts, max_dist=0, per_word=4, known=True, **dict(RULE, **RESCORING))
    flagged = r.correct_words(TEXTS, lex, contexts, max_dist=0, per_word=4, known=True, boundaries=True, **dict(RULE, **RESCORING))
    same_rescored(flagged[1], plain[1])
    for wrong in (dict(joiner="a"), dict(joiner="  "), dict(joiner=""), dict(joiner="\t"), dict(min_part=0), dict(min_part=33)):
        with pytest.raises(ValueError):
            r.correct_words(TEXTS, lex, contexts, boundaries=True, **wrong)
    with pytest.raises(ValueError):
        r.correct_words(TEXTS, lex, contexts, boundaries=True, delimiters="\n")      # the joiner is no delimiter here
    r.correct_words(TEXTS[:1], lex, contexts[:1], boundaries=False, joiner="a", min_part=0, **dict(RULE, **RESCORING))      # (not read)


def test_correct_words_with_boundaries_and_a_channel():
    """the candidates are the chain's, the priors are what the issue prices: a split unit_bits * dist, a merge its bits plus
    unit_bits for the joiner, both times channel_weight"""
    r = small_rater(OracleLM, length=LENGTH)
    lex = r.lexicon(ENTRIES)
    channel = r.channel([("c", "e", 30, 100), ("h", "b", 25, 100)], unit_bits=4.0)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    seen = {}
    real = r.rescore
    r.rescore = lambda texts, edits, contexts=None, **more: seen.update(edits=list(edits), prior=more.get("prior")) or real(texts, edits, contexts, **more)
    found, rescored, bits = r.correct_words(TEXTS, lex, contexts, max_dist=2, per_word=4, boundaries=True, channel=channel, max_bits=9.0,
                                            channel_weight=0.5, **dict(RULE, **RESCORING))
    edits, prior = seen["edits"], seen["prior"]
    assert len(prior) == len(edits) > 0 and all(len(p) == len(e[3]) for p, e in zip(prior, edits))
    assert edits == sorted(edits, key=lambda e: e[:3])
    by_span = dict((e[:3], (e[3], p)) for e, p in zip(edits, prior))
    strings, weights = by_span[0, 2, 8]                                          # badcab: the split costs one unit
    assert weights[strings.index("bad cab")] == 0.5 * 4.0 * 1
    strings, weights = by_span[1, 6, 11]                                         # be ad -> bead: identical, the joiner's unit alone
    assert strings[0] == "bead" and weights[0] == 0.5 * 4.0
    merged = r.lexicon_neighbours(["head"], lex, channel=channel, max_bits=5.0)
    strings, weights = by_span[3, 6, 11]                                         # hea d -> head, and bead through h -> b
    at = merged.strings(0).index("bead")
    assert strings[0] == "head" and weights[strings.index("bead")] == 0.5 * (float(merged.bits[0][at]) + 4.0)
    # a budget below one unit leaves no merge
    r.correct_words(TEXTS, lex, contexts, max_dist=2, per_word=4, boundaries=True, channel=channel, max_bits=3.0, **dict(RULE, **RESCORING))
    assert not [e for e in seen["edits"] if " " in TEXTS[e[0]][e[1]:e[2]]]


def test_boundaries_off_is_what_it_was():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    everything, _ = r.suspect_words(texts, contexts, **RULE)
    in_text = sorted(set(w for one, t in zip(everything, texts) for w in one.strings(t) if len(w) > 1))
    lex = r.lexicon(in_text[::3] + ENTRIES)
    for known in (False, True):
        ref_found, edits, ref_rescored, ref_bits = composed(r, texts, contexts, lex, 1, 3, known, RULE, RESCORING)
        for more in ({}, dict(boundaries=False), dict(boundaries=False, min_part=5, joiner="\n")):
            found, rescored, bits = r.correct_words(texts, lex, contexts, max_dist=1, per_word=3, known=known, **dict(RULE, **RESCORING),
                                                    **more)
            assert bits.tobytes() == ref_bits.tobytes()
            same_rescored(rescored, ref_rescored)
            for one, ref in zip(rescored, ref_rescored):
                assert all(getattr(one, name).tobytes() == getattr(ref, name).tobytes()
                           for name in ("starts", "ends", "first", "cost0", "cost", "best", "gain"))


# ---------------------------------------------------------------------------------------------- command line
def test_cli_lexicon_boundaries(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    files, texts = [], [t for t in TEXTS if t]
    for i, text in enumerate(texts):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        name.write_text(text)
        files.append(str(name))
    contexts = [[170], [174], [178], [182]]
    listing = tmp_path / "words.tsv"
    listing.write_text("".join("%s\t%d\n" % (w, 1000 - i) for i, w in enumerate(ENTRIES)))
    options = ["-s", "4", "-k", "2", "--max-prob", "1", "--min-rank", "0", "--min-suspects", "0", "--max-dist", "2", "--per-word", "4",
               "--left", "12", "--ahead", "3", "--min-gain", "0.5"]
    base = ["lexicon", "-m", str(model), "--lexicon", str(listing), "--apply"]
    res = CliRunner().invoke(run.cli, base + ["--boundaries", "--min-part", "3"] + options + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    ref = small_rater(OracleLM, length=LENGTH)
    _, found, _ = ref.correct_words(texts, ref.lexicon(ENTRIES), contexts, max_dist=2, per_word=4, boundaries=True, min_part=3,
                                    **dict(RULE, **RESCORING))
    kinds = set()
    for line, text, one in zip(lines, texts, found):
        assert line["corrected"] == one.apply(text) and len(line["rescored"]) == len(one)
        for row, a, b, new, g in zip(line["rescored"], one.starts, one.ends, one.proposals(), one.gain):
            assert row[:5] == [int(a), int(b), text[int(a):int(b)], new, float(g)]
            assert row[5] == ("merge" if " " in row[2] else "split" if new is not None and " " in new else "word")
            kinds.add(row[5])
    assert "merge" in kinds and len(kinds) >= 2
    # without the flag: today's records, and no pair among them
    plain = CliRunner().invoke(run.cli, base + options + files)
    assert plain.exit_code == 0
    rows = [row for l in plain.output.strip().split("\n") for row in json.loads(l)["rescored"]]
    assert rows and all(len(row) == 5 and " " not in row[2] for row in rows)
    assert len(rows) < sum(len(l["rescored"]) for l in lines)
    for wrong in (["--min-part", "0"], ["--min-part", "33"]):
        assert CliRunner().invoke(run.cli, base + ["--boundaries"] + wrong + files).exit_code != 0, wrong
