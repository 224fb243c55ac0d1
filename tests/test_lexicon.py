"""`ratebulk.lexicon_layout_host`, `lexicon_neighbours_host`, `ratebatch.Lexicon`, `Rater.lexicon`, `Rater.lexicon_neighbours`,
`Rater.correct_words` and `keraslm-rate lexicon` on the CPU.

The oracle-backed engine double has no `lexicon_neighbours`, so the Rater runs the numpy statement -- normalising, the unique
words, the spread over duplicates, the table of candidates and the command are the product's.  The statement itself is held to
a two-row Levenshtein distance written here; the device kernel is held to the statement in test_lexicon_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import ALPHABET, random_text, small_rater
from tests.test_rate_suspects import contract_texts

LENGTH = 16


# ---------------------------------------------------------------------------------------------- the numpy statements
def lev(a, b, V):
    """Levenshtein distance, unit costs, two rows; two ids are equal iff they are the same number within [0, V)"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            same = x == y and 0 <= x < V
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1)))
        prev = cur
    return prev[-1]


def brute_neighbours(queries, entries, V, max_dist, K):
    exact = np.full(len(queries), -1, dtype=np.int32)
    found = np.zeros(len(queries), dtype=np.int32)
    cand = np.full((len(queries), K), -1, dtype=np.int32)
    dist = np.full((len(queries), K), -1, dtype=np.int32)
    for q, word in enumerate(queries):
        if not 1 <= len(word) <= 64:
            continue
        near = []
        for e, entry in enumerate(entries):
            if 1 <= len(entry) <= 64 and abs(len(entry) - len(word)) <= max_dist:
                d = lev(word, entry, V)
                if d <= max_dist:
                    near.append((d, e))
        same = [e for d, e in near if d == 0]
        if same:
            exact[q] = min(same)
        near = sorted(p for p in near if p[0] > 0)
        found[q] = len(near)
        for place, (d, e) in enumerate(near[:K]):
            cand[q, place], dist[q, place] = e, d
    return exact, found, cand, dist


def pooled(words):
    pool = np.asarray([i for w in words for i in w], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64)
    return pool, off


def mutate(rng, word, V, edits):
    word = list(word)
    for _ in range(edits):
        op = int(rng.integers(0, 3))
        at = int(rng.integers(0, len(word) + 1))
        if op == 0 and word:
            word[min(at, len(word) - 1)] = int(rng.integers(-1, V + 1))
        elif op == 1 and len(word) > 1:
            del word[min(at, len(word) - 1)]
        else:
            word.insert(at, int(rng.integers(-1, V + 1)))
    return word


def random_lexicon(rng, V, n, lengths):
    """n entries over [-1, V] -- ids outside [0, V) on purpose --, with duplicates, the lengths 0, 1, 64 and 65 among them"""
    entries = [rng.integers(-1, V + 1, int(rng.choice(lengths))).tolist() for _ in range(n)]
    entries += [list(e) for e in entries[:n // 8]]                        # duplicates are separate entries
    entries += [[], [1], [V], [2] * 64, [2] * 65, [1] * 63 + [0]]
    order = rng.permutation(len(entries))
    return [entries[i] for i in order]


def test_lexicon_neighbours_host_against_a_two_row_levenshtein():
    rng = np.random.default_rng(0)
    V = 3
    entries = random_lexicon(rng, V, 120, [1, 2, 3, 4, 5, 6, 7])
    queries = [mutate(rng, entries[int(rng.integers(0, len(entries)))] or [1], V, int(rng.integers(0, 4))) for _ in range(40)]
    queries += [list(entries[5]), [], [1], [V], [-1], [2] * 64, [2] * 65, [2] * 63, [2] * 62 + [1, 1], [0] + [2] * 63]
    layout = ratebulk.lexicon_layout_host(*pooled(entries))
    q_pool, q_off = pooled(queries)
    seen = set()
    for max_dist in (0, 1, 2, 3):
        for K in (1, 16):
            want = brute_neighbours(queries, entries, V, max_dist, K)
            got = ratebulk.lexicon_neighbours_host(q_pool, q_off, *layout, V=V, max_dist=max_dist, K=K)
            assert [a.dtype for a in got] == [np.int32] * 4 and got[2].shape == got[3].shape == (len(queries), K)
            for g, w, name in zip(got, want, ("exact", "found", "cand", "dist")):
                assert np.array_equal(g, w), (max_dist, K, name)
            seen.update(got[3].reshape(-1).tolist())
            if max_dist == 0:
                assert not got[1].any() and (got[2] == -1).all()
    assert seen == {-1, 1, 2, 3}
    want = brute_neighbours(queries, entries, V, 2, 16)
    assert (want[0] >= 0).sum() >= 4 and want[1].max() > 16 and (want[1] == 0).any()
    # an id outside [0, V) equals nothing, itself included: [V] and [-1] are no entries of their own lexicon
    at = dict((tuple(w), i) for i, w in enumerate(queries))
    assert want[0][at[(V,)]] == -1 and want[0][at[(-1,)]] == -1 and want[0][at[(1,)]] >= 0
    assert want[0][at[()]] == -1 and want[1][at[()]] == 0 and want[0][at[(2,) * 65]] == -1 and want[1][at[(2,) * 65]] == 0
    assert want[0][at[(2,) * 64]] >= 0
    for wrong in (dict(V=0), dict(V=4097), dict(max_dist=-1), dict(max_dist=9), dict(K=0), dict(K=17)):
        with pytest.raises(ValueError):
            ratebulk.lexicon_neighbours_host(q_pool, q_off, *layout, **dict(dict(V=V, max_dist=1, K=2), **wrong))
    with pytest.raises(ValueError):
        ratebulk.lexicon_neighbours_host(q_pool, q_off, layout[0][:-1], layout[1], layout[2], V, 1, 2)


def test_lexicon_layout_host_reads_back():
    rng = np.random.default_rng(1)
    entries = random_lexicon(rng, 50, 300, [1, 2, 3, 5, 8, 13, 40, 64, 65, 70, 0])
    pool, off = pooled(entries)
    chars, order, class_first = ratebulk.lexicon_layout_host(pool, off)
    assert chars.dtype == order.dtype == np.int32 and class_first.dtype == np.int64 and class_first.shape == (66,)
    kept = [i for i, e in enumerate(entries) if 1 <= len(e) <= 64]
    assert len(kept) < len(entries) and sorted(order.tolist()) == kept and class_first[0] == class_first[1] == 0
    assert class_first[65] == len(order) and (np.diff(class_first) >= 0).all()
    base = 0
    for L in range(1, 65):
        a, b = int(class_first[L]), int(class_first[L + 1])
        n = b - a
        assert order[a:b].tolist() == sorted(i for i in kept if len(entries[i]) == L)      # ascending within a class
        for p in range(a, b):
            assert [int(chars[base + j * n + (p - a)]) for j in range(L)] == entries[order[p]]
        base += L * n
    assert base == len(chars)
    none = ratebulk.lexicon_layout_host(np.zeros(0, dtype=np.int32), [0, 0, 0])
    assert none[0].shape == none[1].shape == (0,) and not none[2].any()


# ---------------------------------------------------------------------------------------------- the Rater on the double
def test_rater_lexicon_drops_and_counts():
    r = small_rater(OracleLM, length=LENGTH)
    words = ["abc", "", "abd", "abc", "a" * 64, "a" * 65, "axc", "bad cab", "be", "abd", "é"]
    lex = r.lexicon(iter(words))
    assert type(lex) is ratebatch.Lexicon and lex.words == ["abc", "abd", "a" * 64, "bad cab", "be"] and len(lex) == 5
    assert lex.dropped == dict(empty=1, long=1, unmapped=2, duplicate=2)
    assert lex.pool.dtype == np.int32 and lex.off.tolist() == [0, 3, 6, 70, 77, 79]
    assert lex.pool[:3].tolist() == [r.mapping[0][c] for c in "abc"] and lex.voc_size == r.voc_size
    for mine, ref in zip((lex.chars, lex.order, lex.class_first), ratebulk.lexicon_layout_host(lex.pool, lex.off)):
        assert np.array_equal(mine, ref)
    assert lex.order.tolist() == [4, 0, 1, 3, 2]
    # a rater whose mapping has changed since: another object, or a character more
    near = r.lexicon_neighbours(["abe"], lex)
    assert near.strings(0) == ["abc", "abd", "be"] and near.dist[0].tolist() == [1, 1, 1] + [-1] * 5
    r.mapping[0]["z"] = 99
    with pytest.raises(ValueError):
        r.lexicon_neighbours(["abe"], lex)
    del r.mapping[0]["z"]
    assert r.lexicon_neighbours(["abe"], lex).strings(0) == ["abc", "abd", "be"]
    r.mapping = (dict(r.mapping[0]), r.mapping[1])
    with pytest.raises(ValueError):
        r.lexicon_neighbours(["abe"], lex)
    with pytest.raises(ValueError):
        r.correct_words(["ab cd"], lex)
    r.voc_size = 4097
    with pytest.raises(ValueError):
        r.lexicon(["abc"])


def lexicon_words(rng, n):
    """n words over the letters of the alphabet, 1 .. 7 characters, most of them short"""
    letters = [c for c in ALPHABET if not c.isspace()]
    return ["".join(letters[int(k)] for k in rng.integers(0, len(letters), int(rng.integers(1, 8)))) for _ in range(n)]


def test_lexicon_neighbours_on_the_double():
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(2)
    lex = r.lexicon(lexicon_words(rng, 300))
    words = lexicon_words(rng, 30) + [lex.words[3], "a?c", "", "ab" * 40, lex.words[3]]
    words += words[:7]                                                    # duplicates in the input
    near = r.lexicon_neighbours(iter(words), lex, max_dist=2, per_word=5)
    assert type(near) is ratebatch.Neighbours and len(near) == len(words) and near.index.shape == near.dist.shape == (len(words), 5)
    pool, off = pooled([[r.mapping[0].get(c, 0) for c in w] for w in words])
    want = ratebulk.lexicon_neighbours_host(pool, off, lex.chars, lex.order, lex.class_first, r.voc_size, 2, 5)
    for got, ref in zip((near.exact, near.found, near.index, near.dist), want):
        assert got.dtype == np.int32 and np.array_equal(got, ref)
    at = len(words) - 12
    assert near.exact[at] == 3 == near.exact[at + 4] and near.found[at + 2] == 0 == near.found[at + 3]
    assert near.found.max() > 5 and near.strings(0) == [lex.words[i] for i in near.index[0] if i >= 0]
    # an unmapped character keeps id 0: an ordinary id that no entry holds -- one substitution away from "abc" and its like
    one = r.lexicon_neighbours(["a?c"], r.lexicon(["abc", "a?c", "ac"]), max_dist=1)
    assert one.exact[0] == -1 and one.strings(0) == ["abc", "ac"]
    # no words; a lexicon without a kept entry
    none = r.lexicon_neighbours([], lex, per_word=3)
    assert len(none) == 0 and none.index.shape == (0, 3) and none.exact.dtype == np.int32
    empty = r.lexicon(["", "?"])
    assert len(empty) == 0 and empty.dropped == dict(empty=1, long=0, unmapped=1, duplicate=0)
    none = r.lexicon_neighbours(["ab", "ab"], empty, per_word=3)
    assert none.exact.tolist() == [-1, -1] and none.found.tolist() == [0, 0] and (none.index == -1).all() and (none.dist == -1).all()
    for wrong in (dict(max_dist=-1), dict(max_dist=9), dict(per_word=0), dict(per_word=17)):
        with pytest.raises(ValueError):
            r.lexicon_neighbours(["ab"], lex, **wrong)
    with pytest.raises(ValueError):
        r.lexicon_neighbours(["ab"], ["ab"])


def composed(r, texts, contexts, lex, max_dist, per_word, known, rule, rescoring):
    """suspect_words + word_edits with a table from the host statement + rescore"""
    found, bits = r.suspect_words(texts, contexts, **rule)
    words = sorted(set(w for one, t in zip(found, texts) for w in one.strings(t)))
    pool, off = pooled([[r.mapping[0].get(c, 0) for c in w] for w in words])
    exact, _, cand, _ = ratebulk.lexicon_neighbours_host(pool, off, lex.chars, lex.order, lex.class_first, r.voc_size, max_dist,
                                                         per_word)
    table = dict((w, [lex.words[i] for i in cand[q] if i >= 0] if known or exact[q] < 0 else []) for q, w in enumerate(words))
    edits = ratebatch.word_edits(found, texts, table)
    return found, edits, r.rescore(texts, edits, contexts, **rescoring), bits


def same_rescored(got, want):
    assert len(got) == len(want)
    for one, ref in zip(got, want):
        assert type(one) is ratebatch.Rescored and one.candidates == ref.candidates
        for name in ("starts", "ends", "first", "cost0", "cost", "best", "gain"):
            assert np.array_equal(getattr(one, name), getattr(ref, name)), name


def test_correct_words_is_the_composed_call():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(3)
    everything, _ = r.suspect_words(texts, contexts, k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    in_text = sorted(set(w for one, t in zip(everything, texts) for w in one.strings(t) if len(w) > 1))
    lex = r.lexicon(in_text[::3] + lexicon_words(rng, 300))               # every third word of the texts is an entry
    rule = dict(k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.5)
    n_edits = {}
    for known in (False, True):
        for precision in ("bf16", "split"):
            found, rescored, bits = r.correct_words(texts, lex, contexts, max_dist=1, per_word=3, known=known, precision=precision,
                                                    **dict(rule, **rescoring))
            ref_found, edits, ref_rescored, ref_bits = composed(r, texts, contexts, lex, 1, 3, known, dict(rule, precision=precision),
                                                                dict(rescoring, precision=precision))
            assert np.array_equal(bits, ref_bits)
            for one, ref in zip(found, ref_found):
                assert one.spans() == ref.spans() and np.array_equal(one.bits, ref.bits)
            same_rescored(rescored, ref_rescored)
            assert sum(len(one) for one in rescored) == len(edits) > 0
            n_edits[known] = len(edits)
            entries = [(i, a, b) for i, a, b, _ in edits if texts[i][a:b] in lex.words]
            assert bool(entries) == known                                # a word of the lexicon is left alone by default
    assert n_edits[True] > n_edits[False]
    found, rescored, bits = r.correct_words(["", "a"], lex)
    assert [len(f) for f in found] == [0, 0] == [len(f) for f in rescored] and bits.tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------- command line
def test_cli_lexicon(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("lexicon") == run.COMMAND_ORDER.index("words") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(4)
    files, texts = [], []
    for i, size in enumerate((60, 1, 80)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
    contexts = [[170], [174], [178]]
    entries = lexicon_words(rng, 200)
    listing = tmp_path / "words.tsv"
    listing.write_text("".join("%s\t%d\n" % (w, 1000 - i) for i, w in enumerate(entries)) + "\n")
    options = ["-s", "2", "--precision", "split", "-k", "2", "--max-prob", "1", "--min-rank", "0", "--min-suspects", "0",
               "--max-dist", "1", "--per-word", "4", "--left", "10", "--ahead", "2", "--min-gain", "0.25", "--delimiters", " \n"]
    res = CliRunner().invoke(run.cli, ["lexicon", "-m", str(model), "--lexicon", str(listing), "--apply"] + options + files)
    assert res.exit_code == 0, res.output
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    ref = small_rater(OracleLM, length=LENGTH)
    lex = ref.lexicon(entries)
    assert lex.dropped["duplicate"] + len(lex) == len(entries)            # (the empty last line and the counts are not entries)
    _, found, _ = ref.correct_words(texts, lex, contexts, max_dist=1, per_word=4, delimiters=" \n", k=2, max_prob=1.0, min_rank=0,
                                    min_suspects=0, left=10, ahead=2, min_gain=0.25, streams=2, precision="split")
    assert sum(len(f) for f in found) > 0 and sum(int((f.best >= 0).sum()) for f in found) > 0
    for line, text, one in zip(lines, texts, found):
        assert line["chars"] == len(text) and line["corrected"] == one.apply(text)
        assert line["rescored"] == [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                                    for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
    assert lines[1]["rescored"] == [] and lines[1]["corrected"] == texts[1]
    plain = CliRunner().invoke(run.cli, ["lexicon", "-m", str(model), "--lexicon", str(listing)] + options + files)
    assert plain.exit_code == 0 and "corrected" not in json.loads(plain.output.strip().split("\n")[0])
    # usage errors
    base = ["lexicon", "-m", str(model)]
    assert CliRunner().invoke(run.cli, base + files).exit_code != 0                                        # no --lexicon
    assert CliRunner().invoke(run.cli, base + ["--lexicon", str(tmp_path / "none.txt")] + files).exit_code != 0
    for wrong in (["--max-dist", "-1"], ["--max-dist", "9"], ["--per-word", "0"], ["--per-word", "17"], ["-k", "0"],
                  ["--precision", "f32"], ["--min-rank", "-1"], ["--min-chars", "0"], ["--left", "0"], ["--ahead", "-1"]):
        assert CliRunner().invoke(run.cli, base + ["--lexicon", str(listing)] + wrong + files).exit_code != 0, wrong
