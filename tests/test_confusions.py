"""`ratebulk.confusion_counts_host`, `ratebatch.Confusions`, `Rater.confusions` and `keraslm-rate confusions` on the CPU.

The oracle-backed engine double has no `confusion_counts`, so the Rater runs the numpy statements -- normalising, the code points,
the result class and the command are the product's.  The statement itself is held to a brute force written out here (a Counter
over `Alignment.strings` with the anchoring rules, occurrences by `str.find`) and to hand-made cases with their tables written
out; the device kernels are held to the statement in test_confusions_gpu.py."""
import collections
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_lexicon import pooled
from tests.test_rate_bulk_gpu import random_text, small_rater
from tests.test_witnesses import noisy

LENGTH = 16


def codes(strings):
    return pooled([[ord(c) for c in s] for s in strings])


def aligned(A, B, max_dist, join=0):
    """the pools of the strings A (OCR) and B (truth) and what align_pairs_host makes of them: confusion_counts_host's inputs"""
    longest = max(len(t) for t in A + B)
    args = codes(A) + codes(B)
    return args + ratebulk.align_pairs_host(*args, longest, max_dist, join)


def anchored(A, B, max_dist, join=0):
    """the issue's rules, spelled out over `Alignment.strings`: [(pair, start, end, source, target)] for every span of an
    accepted pair that has a source, plus the number of spans of empty texts"""
    _, _, _, _, dist, n_spans, spans = aligned(A, B, max_dist, join)
    found, empty = [], 0
    for p, (a, b) in enumerate(zip(A, B)):
        if dist[p] < 0:
            continue
        one = ratebatch.Alignment(dist[p], spans[p, :n_spans[p]])
        for (written, reading), (a0, a1, b0, b1) in zip(one.strings(a, b), one.spans.tolist()):
            if written:
                found.append((p, a0, a1, written, reading))
            elif a0 > 0:                                     # lost characters: anchored on the character in front
                assert a[a0 - 1] == b[b0 - 1]
                found.append((p, a0 - 1, a0, a[a0 - 1], b[b0 - 1:b1]))
            elif a:                                          # ... at the beginning: on the one behind
                assert a[0] == b[b1]
                found.append((p, 0, 1, a[0], b[:b1 + 1]))
            else:
                empty += 1
    return found, empty, dist


def brute(A, B, max_dist, join, max_chars):
    """[(source, target, count, occ)] in order of first occurrence and (R, counted, long, empty)"""
    found, empty, dist = anchored(A, B, max_dist, join)
    seen = collections.Counter()
    too_long = 0
    for _, _, _, source, target in found:
        if len(source) > max_chars or len(target) > max_chars:
            too_long += 1
        else:
            seen[source, target] += 1
    stands = {}
    for source, _ in seen:
        stands[source] = 0
        for p, a in enumerate(A):
            if dist[p] >= 0:
                start = a.find(source)
                while start >= 0:
                    stands[source] += 1
                    start = a.find(source, start + 1)
    table = [(source, target, times, stands[source]) for (source, target), times in seen.items()]
    return table, (len(table), sum(seen.values()), too_long, empty)


def table_of(rules, count, occ):
    rows = []
    for r, c, o in zip(rules.tolist(), count.tolist(), occ.tolist()):
        if r[0] < 0:
            assert r == [-1] * 10 and c == 0 and o == 0
            continue
        assert 1 <= r[0] <= 4 and 0 <= r[1] <= 4 and r[2 + r[0]:6] == [0] * (4 - r[0]) and r[6 + r[1]:] == [0] * (4 - r[1])
        rows.append(("".join(map(chr, r[2:2 + r[0]])), "".join(map(chr, r[6:6 + r[1]])), c, o))
    return rows


def statement(A, B, max_dist, join=0, max_chars=4, room=64):
    rules, count, occ, stats = ratebulk.confusion_counts_host(*aligned(A, B, max_dist, join), max_chars, room)
    assert rules.dtype == np.int32 and rules.shape == (room, 10) and stats.dtype == np.int64 and stats.shape == (4,)
    assert count.dtype == np.int64 and occ.dtype == np.int64 and count.shape == (room,) and occ.shape == (room,)
    return table_of(rules, count, occ), tuple(stats.tolist())


def confused_pairs(rng, count, V, longest=24, most=6):
    A = ["".join(chr(65 + int(x)) for x in rng.integers(0, V, int(rng.integers(0, longest + 1)))) for _ in range(count)]
    B = []
    for a in A:
        b = list(a)
        for _ in range(int(rng.integers(0, most + 1))):
            op, at = int(rng.integers(0, 3)), int(rng.integers(0, len(b) + 1))
            if op == 0 and b:
                b[min(at, len(b) - 1)] = chr(65 + int(rng.integers(0, V)))
            elif op == 1 and b:
                del b[min(at, len(b) - 1)]
            else:
                b.insert(at, chr(65 + int(rng.integers(0, V))))
        B.append("".join(b))
    return A, B


# ---------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("V", [2, 50])
@pytest.mark.parametrize("max_chars", [1, 2, 4])
def test_confusion_counts_host_against_a_brute_force(V, max_chars):
    rng = np.random.default_rng(V + max_chars)
    seen = np.zeros(4, dtype=np.int64)
    for join in (0, 1):
        A, B = confused_pairs(rng, 120, V)
        A[7], A[8] = "", ""                                  # empty OCR texts: against an empty truth and against some
        B[7] = ""
        want, stats = brute(A, B, 4, join, max_chars)
        got, got_stats = statement(A, B, 4, join, max_chars, room=len(want) + 3)
        assert got == want and got_stats == stats
        assert all(count <= occ for _, _, count, occ in got) and all(source for source, _, _, _ in got)
        seen += stats
    assert (seen > 0).all()                                  # records, long spans and empty texts all occurred


CASES = [
    # A (OCR), B (truth), max_dist, [(source, target, count, occ)], (R, counted, long, empty)
    (["modern"], ["modem"], 4, [("rn", "m", 1, 1)], (1, 1, 0, 0)),
    (["abxc"], ["abc"], 4, [("x", "", 1, 1)], (1, 1, 0, 0)),                          # a deletion
    (["abcb"], ["abxcb"], 4, [("b", "bx", 1, 2)], (1, 1, 0, 0)),                      # an insertion, anchored in front
    (["abca"], ["xabca"], 4, [("a", "xa", 1, 2)], (1, 1, 0, 0)),                      # ... at the start, anchored behind
    ([""], ["q"], 4, [], (0, 0, 0, 1)),                                               # ... into an empty text
    (["a12345b"], ["aYb"], 6, [], (0, 0, 1, 0)),                                      # five characters against one
    (["xaaaa"], ["xaa"], 4, [("aa", "", 1, 3)], (1, 1, 0, 0)),                        # overlapping occurrences count
    (["xya", "bcab"], ["xya", "bcm"], 4, [("ab", "m", 1, 1)], (1, 1, 0, 0)),          # "a" | "b": not across the border
    (["rnx", "rnrnrnrn", "arn"], ["mx", "zzzzzzzzzzzzzzzzzz", "arn"], 4, [("rn", "m", 1, 2)], (1, 1, 0, 0)),      # a rejected pair
    (["abab", "xbab"], ["cbcb", "xbcb"], 4, [("a", "c", 3, 3)], (1, 3, 0, 0)),        # one record, three spans
    (["ab", "ab"], ["xb", "yb"], 4, [("a", "x", 1, 2), ("a", "y", 1, 2)], (2, 2, 0, 0)),      # one source, two records, one occ
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_confusion_counts_host_by_hand(case):
    A, B, max_dist, table, stats = CASES[case]
    assert statement(A, B, max_dist) == (table, stats)
    assert brute(A, B, max_dist, 0, 4) == (table, stats)


def test_confusion_counts_host_limits_and_room():
    A, B = ["a12345b", "abc", "abcd"], ["aYb", "xabc", "abyyyyd"]
    # max_chars counts AFTER anchoring: the insertion "x" in front of "a" is ("a", "xa"), two characters
    assert statement(A, B, 6, max_chars=4) == ([("a", "xa", 1, 3), ("c", "yyyy", 1, 2)], (2, 2, 1, 0))
    assert statement(A, B, 6, max_chars=2) == ([("a", "xa", 1, 3)], (1, 1, 2, 0))
    assert statement(A, B, 6, max_chars=1) == ([], (0, 0, 3, 0))
    # room smaller than R: the first `room` records, stats[0] == R, -1 and 0 behind
    A = ["abcdefgh"]
    B = ["AbCdEfGh"]
    full = [("a", "A", 1, 1), ("c", "C", 1, 1), ("e", "E", 1, 1), ("g", "G", 1, 1)]
    for room in (1, 3, 4, 9):
        rules, count, occ, stats = ratebulk.confusion_counts_host(*aligned(A, B, 4), 4, room)
        assert table_of(rules, count, occ) == full[:room] and stats.tolist() == [4, 4, 0, 0]
        assert (rules[4:] == -1).all() and not count[4:].any() and not occ[4:].any()
    # spans beyond n_spans are not read, fields outside the texts are `long`, offsets outside the pools reject the pair
    args = list(aligned(["abc", "abc"], ["abd", "xbc"], 3))
    spans = args[6].copy()
    spans[0, 1] = [0, 1, 0, 1]                               # (behind n_spans[0] == 1)
    spans[1, 0] = [0, 4, 0, 1]                               # a1 beyond the text
    rules, count, occ, stats = ratebulk.confusion_counts_host(*args[:6], spans, 4, 4)
    assert table_of(rules, count, occ) == [("c", "d", 1, 2)] and stats.tolist() == [1, 1, 1, 0]
    off = args[1].copy()
    off[2] = 7                                               # pair 1 reaches beyond a_pool: neither its spans nor its text count
    rules, count, occ, stats = ratebulk.confusion_counts_host(args[0], off, *args[2:], 4, 4)
    assert table_of(rules, count, occ) == [("c", "d", 1, 1)] and stats.tolist() == [1, 1, 0, 0]
    for wrong in (dict(max_chars=0), dict(max_chars=5), dict(room=0)):
        with pytest.raises(ValueError):
            ratebulk.confusion_counts_host(*args, **dict(dict(max_chars=4, room=4), **wrong))
    with pytest.raises(ValueError):
        ratebulk.confusion_counts_host(*args[:4], args[4][:1], *args[5:], 4, 4)


def test_planted_substitutions_are_counted_exactly():
    """substitutions of symbols that occur nowhere else, at least three places apart, planted k times each: the table holds
    exactly these counts; a source that also stands where it was read correctly has occ above count"""
    rng = np.random.default_rng(3)
    planted = [("ā", "ȁ", 7), ("Ă", "Ȃ", 1), ("ă", "ȃ", 12), ("Ą", "", 5)]
    todo = [pair for pair in planted for _ in range(pair[2])]
    order = rng.permutation(len(todo))
    A, B = [], []
    for line in range(5):
        a, b = [], []
        for k in order[line::5]:
            filler = random_text(rng, int(rng.integers(3, 7)))
            a += [filler, todo[k][0]]
            b += [filler, todo[k][1]]
        A.append("".join(a) + "xxā")                      # (read correctly here: an occurrence, not a confusion)
        B.append("".join(b) + "xxā")
    table, stats = statement(A, B, 32)
    assert sorted(table) == sorted((s, t, k, k + (5 if s == "ā" else 0)) for s, t, k in planted)
    assert stats == (4, 25, 0, 0) and all(count <= occ for _, _, count, occ in table)


# ---------------------------------------------------------------------------------------------- the result class
def hand_made():
    """six records over three sources, counts and occurrences chosen for the thresholds"""
    rows = [("a", "x", 5, 100), ("b", "y", 9, 10), ("a", "", 7, 100), ("c", "z", 1, 2), ("a", "w", 2, 100), ("a", "v", 7, 100), ("b", "q", 1, 10)]
    rules = np.zeros((len(rows), 10), dtype=np.int32)
    for row, (source, target, _, _) in zip(rules, rows):
        row[:2] = len(source), len(target)
        row[2:2 + len(source)] = [ord(c) for c in source]
        row[6:6 + len(target)] = [ord(c) for c in target]
    return ratebatch.Confusions(rules, [r[2] for r in rows], [r[3] for r in rows], np.array([len(rows), 32, 3, 1]), np.array([3, -1, 0, 5]),
                                np.array([40, 10, 0, 60]))


def test_confusions_fields_rules_and_write(tmp_path):
    from ocrd_keraslm_amd.scripts import run
    found = hand_made()
    assert len(found) == 7 and found.sources[:3] == ["a", "b", "a"] and found.targets[:3] == ["x", "y", ""]
    assert found.count.dtype == np.int64 and found.occ.dtype == np.int64 and found.dist.tolist() == [3, -1, 0, 5]
    assert found.chars == 100 and found.edits == 8 and found.cer == 0.08 and found.spans == 32
    assert found.skipped == dict(different=1, long=3, empty=1)
    assert found.rate(1) == 0.9 and found.rate(0) == 0.05
    # sources by their best record's (-count, first occurrence), replacements likewise, cut to per_source
    assert found.rules() == [("b", ["y"]), ("a", ["", "v", "x"])]
    assert found.rules(per_source=99) == [("b", ["y"]), ("a", ["", "v", "x", "w"])]
    assert found.rules(min_count=1, per_source=1) == [("b", ["y"]), ("a", [""]), ("c", ["z"])]
    assert found.rules(min_count=1, per_source=2)[0] == ("b", ["y", "q"])
    assert found.rules(min_count=6) == [("b", ["y"]), ("a", ["", "v"])]
    assert found.rules(min_count=1, min_rate=0.06) == [("b", ["y", "q"]), ("a", ["", "v"]), ("c", ["z"])]
    assert found.rules(min_count=1, min_rate=0.5) == [("b", ["y"]), ("c", ["z"])]
    assert found.rules(min_count=10) == []
    # the TSV is what `rescore --confusions` reads
    for same in (dict(), dict(min_count=1, per_source=99), dict(min_count=10)):
        path = tmp_path / "table.tsv"
        assert found.write(str(path), **same) == len(found.rules(**same))
        assert run._read_confusions(str(path)) == found.rules(**same)
    assert (tmp_path / "table.tsv").read_text() == ""
    with open(str(tmp_path / "open.tsv"), "w") as file:
        found.write(file, min_count=6)
    assert (tmp_path / "open.tsv").read_text() == "b\ty\na\t\tv\n"
    # no pairs, no records
    none = ratebatch.Confusions(np.zeros((0, 10)), [], [], np.zeros(4), [], [])
    assert len(none) == 0 and none.rules() == [] and none.cer == 0.0 and none.chars == 0 and none.skipped == dict(different=0, long=0, empty=0)


# ---------------------------------------------------------------------------------------------- the Rater on the double
def confusion_corpus(seed):
    rng = np.random.default_rng(seed)
    truths = [random_text(rng, size) for size in (40, 33, 0, 25, 60, 18, 30, 50, 0)]
    texts = [noisy(rng, t, int(rng.integers(0, 6))) if t else "" for t in truths]
    texts[5] = random_text(rng, 20)                          # another text altogether
    texts[6] = truths[6]                                     # read without an error
    texts[8] = ""                                            # nothing read where something stands
    truths[8] = "ab"
    return texts, truths


def same_confusions(got, rules, count, occ, stats, dist, truths):
    R = int(stats[0])
    want = ratebatch.Confusions(rules[:R], count[:R], occ[:R], stats, dist, [len(t) for t in truths])
    assert type(got) is ratebatch.Confusions
    for name in ("sources", "targets", "chars", "edits", "cer", "skipped", "spans"):
        assert getattr(got, name) == getattr(want, name), name
    for name in ("count", "occ", "dist"):
        assert getattr(got, name).dtype == getattr(want, name).dtype and np.array_equal(getattr(got, name), getattr(want, name)), name
    assert len(got) == R and got.spans == got.count.sum()
    return want


def test_rater_confusions_on_the_double():
    r = small_rater(OracleLM, length=LENGTH)
    texts, truths = confusion_corpus(4)
    texts += ["été", "modern times"]              # decomposed accents are composed first
    truths += ["ete", "modem times"]
    for max_dist, join, max_chars in ((8, 0, 4), (8, 1, 2), (3, 0, 1)):
        got = r.confusions(iter(texts), iter(truths), max_dist=max_dist, join=join, max_chars=max_chars)
        a, b = [windows.normalize(t) for t in texts], [windows.normalize(t) for t in truths]
        args = aligned(a, b, max_dist, join)
        want = same_confusions(got, *ratebulk.confusion_counts_host(*args, max_chars, 1000), args[4], b)
        assert got.skipped["different"] >= 1 and got.skipped["empty"] == 1 and len(got) > 5
        assert got.rules(min_count=1) == want.rules(min_count=1)
    assert ("é", "e") in zip(got.sources, got.targets)
    # more records than the first call has room for: once more with room for all -- the same result
    small = small_rater(OracleLM, length=LENGTH)
    small._CONFUSION_ROOM = 3
    again = small.confusions(texts, truths, max_dist=3, join=0, max_chars=1)
    assert len(again) > 3 and again.sources == got.sources and again.targets == got.targets and np.array_equal(again.occ, got.occ)
    # the character error rate by hand: 2 + 1 edits over 5 + 4 characters, the rejected pair left out
    by_hand = r.confusions(["modern", "abc", "qqqqqqqq"], ["modem", "abcd", "a"], max_dist=4)
    assert by_hand.dist.tolist() == [2, 1, -1] and by_hand.chars == 9 and by_hand.edits == 3 and by_hand.cer == 3 / 9
    assert list(zip(by_hand.sources, by_hand.targets, by_hand.count.tolist(), by_hand.occ.tolist())) == [("rn", "m", 1, 1), ("c", "cd", 1, 1)]
    assert by_hand.skipped == dict(different=1, long=0, empty=0) and by_hand.rules(min_count=1) == [("rn", ["m"]), ("c", ["cd"])]
    none = r.confusions([], [])
    assert type(none) is ratebatch.Confusions and len(none) == 0 and none.rules() == [] and none.cer == 0.0 and len(none.dist) == 0
    for wrong in (dict(texts=["a" * 4097]), dict(truths=["a" * 4097]), dict(truths=["a", "b"]), dict(max_dist=0), dict(max_dist=256),
                  dict(join=-1), dict(max_chars=0), dict(max_chars=5)):
        with pytest.raises(ValueError):
            r.confusions(**dict(dict(texts=["abc"], truths=["abd"]), **wrong))


def test_rules_lead_confusion_edits_to_every_counted_span():
    """`confusion_edits` under rules(min_count=1, per_source=99) finds every span that was counted, at its anchored place, with
    the truth's reading among the replacements"""
    r = small_rater(OracleLM, length=LENGTH)
    texts, truths = confusion_corpus(9)
    found = r.confusions(texts, truths, max_dist=8)
    rules = found.rules(min_count=1, per_source=99)
    assert sum(len(replacements) for _, replacements in rules) == len(found)
    edits = {}
    for i, start, end, replacements in ratebatch.confusion_edits(texts, rules):
        edits.setdefault((i, start, end), []).extend(replacements)
    spans, _, _ = anchored(texts, truths, 8)
    counted = [s for s in spans if len(s[3]) <= 4 and len(s[4]) <= 4]
    assert len(counted) == found.spans > 10
    for p, start, end, source, target in counted:
        assert texts[p][start:end] == source and target in edits[p, start, end]


# ---------------------------------------------------------------------------------------------- command line
def test_cli_confusions(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("confusions") == run.COMMAND_ORDER.index("witnesses") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(10)
    truth = tmp_path / "gt"
    truth.mkdir()
    files, texts, truths = [], [], []
    for i, size in enumerate((60, 80, 50, 70)):
        name = tmp_path / ("line%d.txt" % i)
        clean = random_text(rng, size)
        read = noisy(rng, clean.replace("a", "e"), 2)        # a planted confusion and some noise
        name.write_text(read)
        files.append(str(name))
        if i != 2:                                           # file 2 has no truth: left out
            (truth / name.name).write_text(clean)
            texts.append(read)
            truths.append(clean)
    base = ["confusions", "-m", str(model), "--truth", str(truth)]
    ref = small_rater(OracleLM, length=LENGTH).confusions(texts, truths, max_dist=16, join=0, max_chars=3)
    assert ("e", "a") in zip(ref.sources, ref.targets)
    res = CliRunner().invoke(run.cli, base + ["--max-dist", "16", "--max-chars", "3", "--per-source", "2"] + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    table = tmp_path / "table.tsv"
    table.write_text(res.stdout)
    assert run._read_confusions(str(table)) == ref.rules(min_count=2, per_source=2) and len(ref.rules(min_count=2, per_source=2)) >= 1
    last = json.loads(res.stderr.strip().split("\n")[-1])
    assert last == dict(pairs=3, different=0, long=ref.skipped["long"], empty=0, chars=ref.chars, edits=ref.edits, cer=ref.cer)
    assert ref.edits > 10 and 0 < ref.cer < 1
    counts = CliRunner().invoke(run.cli, base + ["--max-dist", "16", "--max-chars", "3", "--counts", "--min-count", "1", "--min-rate", "0.02",
                                                 "--per-source", "5"] + files)
    assert counts.exit_code == 0, counts.output + repr(counts.exception)
    lines = [json.loads(l) for l in counts.stdout.strip().split("\n")]
    kept = [i for rows in ref.kept(min_count=1, min_rate=0.02, per_source=5) for i in rows]
    assert lines == [dict(source=ref.sources[i], target=ref.targets[i], count=int(ref.count[i]), occ=int(ref.occ[i]), rate=ref.rate(i))
                     for i in kept] and len(lines) > 3
    assert lines[0]["source"] == "e" and lines[0]["target"] == "a" and lines[0]["count"] >= lines[1]["count"]
    # usage errors
    assert CliRunner().invoke(run.cli, ["confusions", "-m", str(model)] + files).exit_code != 0                       # no --truth
    assert CliRunner().invoke(run.cli, ["confusions", "-m", str(model), "--truth", str(tmp_path / "none")] + files).exit_code != 0
    for wrong in (["--max-dist", "0"], ["--max-dist", "256"], ["--join", "-1"], ["--max-chars", "0"], ["--max-chars", "5"], ["--per-source", "0"]):
        assert CliRunner().invoke(run.cli, base + wrong + files).exit_code != 0, wrong
    long = tmp_path / "long.txt"
    long.write_text("a" * 4097)
    (truth / long.name).write_text("a" * 4090)
    too_long = CliRunner().invoke(run.cli, base + [str(long)])
    assert too_long.exit_code == 2 and "4096" in too_long.output                                                      # a click.UsageError
