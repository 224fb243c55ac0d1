"""`ratebulk.align_pairs_host`, `ratebatch.Alignment`, `ratebatch.witness_edits`, `Rater.align`, `Rater.merge_witnesses` and
`keraslm-rate witnesses` on the CPU.

The oracle-backed engine double has no `align_pairs`, so the Rater runs the numpy statement -- normalising, the code points, the
compaction, the edits and the command are the product's.  The statement itself (a banded DP) is held to a full distance matrix
and a walk back written out here; the device kernel is held to the statement in test_witnesses_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_lexicon import lev, pooled, same_rescored
from tests.test_rate_bulk_gpu import random_text, small_rater

LENGTH = 16
BIG = 1 << 30      # (ids are equal iff they are the same number: lev's range check never bites)


# ---------------------------------------------------------------------------------------------- the statement, in full
def full_alignment(a, b, max_dist, join):
    """(dist, spans) of one pair by the full matrix: the issue's statement, word for word"""
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    d = D[n][m]
    if d > max_dist:
        return -1, []
    ops = []      # backwards: "=", "s", "d", "i"
    i, j = n, m
    while i > 0 or j > 0:
        if i > 0 and j > 0 and a[i - 1] == b[j - 1] and D[i - 1][j - 1] == D[i][j]:
            ops.append("=")
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and D[i - 1][j - 1] + 1 == D[i][j]:
            ops.append("s")
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
            ops.append("d")
            i -= 1
        else:
            ops.append("i")
            j -= 1
    ops.reverse()
    runs = []      # maximal runs of non-matches: [a_start, a_end, b_start, b_end]
    i = j = 0
    previous = "="
    for op in ops:
        i2, j2 = i + (op != "i"), j + (op != "d")
        if op != "=":
            if previous != "=":
                runs[-1][1], runs[-1][3] = i2, j2
            else:
                runs.append([i, i2, j, j2])
        previous = op
        i, j = i2, j2
    spans = []
    for run in runs:      # (a match advances both sides: the matches between two runs are run[0] - spans[-1][1])
        if spans and run[0] - spans[-1][1] <= join:
            spans[-1][1], spans[-1][3] = run[1], run[3]
        else:
            spans.append(list(run))
    return d, spans


def full_pairs(A, B, max_len, max_dist, join):
    P = len(A)
    dist = np.zeros(P, dtype=np.int32)
    n_spans = np.zeros(P, dtype=np.int32)
    spans = np.full((P, max_dist, 4), -1, dtype=np.int32)
    for p, (a, b) in enumerate(zip(A, B)):
        if len(a) > max_len or len(b) > max_len:
            dist[p] = -2
            continue
        dist[p], found = full_alignment(a, b, max_dist, join)
        n_spans[p] = len(found)
        if found:
            spans[p, :len(found)] = found
    return dist, n_spans, spans


def host(A, B, max_len, max_dist, join):
    return ratebulk.align_pairs_host(*pooled(A), *pooled(B), max_len, max_dist, join)


def edited(rng, word, V, edits):
    word = list(word)
    for _ in range(edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(0, len(word) + 1))
        if op == 0 and word:
            word[min(at, len(word) - 1)] = int(rng.integers(0, V))
        elif op == 1 and word:
            del word[min(at, len(word) - 1)]
        else:
            word.insert(at, int(rng.integers(0, V)))
    return word


def applied(a, b, spans):
    out = list(a)
    for a0, a1, b0, b1 in reversed([s for s in spans.tolist() if s[0] >= 0]):
        out[a0:a1] = b[b0:b1]
    return out


def letters(word):
    return "".join(chr(65 + x) for x in word)


def random_pairs(rng, count, V=3, longest=14, most=5):
    A = [rng.integers(0, V, int(rng.integers(0, longest + 1))).tolist() for _ in range(count)]
    return A, [edited(rng, a, V, int(rng.integers(0, most + 1))) for a in A]


def test_align_pairs_host_against_the_full_matrix():
    rng = np.random.default_rng(0)
    statuses = set()
    for max_dist in range(1, 7):
        for join in range(3):
            A, B = random_pairs(rng, 170)
            got = host(A, B, 19, max_dist, join)
            want = full_pairs(A, B, 19, max_dist, join)
            assert [g.dtype for g in got] == [np.int32] * 3 and got[2].shape == (len(A), max_dist, 4)
            for g, w, name in zip(got, want, ("dist", "n_spans", "spans")):
                assert np.array_equal(g, w), (max_dist, join, name)
            dist, n_spans, spans = got
            for p, (a, b) in enumerate(zip(A, B)):
                true = lev(a, b, BIG)
                assert dist[p] == (true if true <= max_dist else -1)
                assert (spans[p, n_spans[p]:] == -1).all() and (spans[p, :n_spans[p]] >= 0).all() and n_spans[p] <= max(dist[p], 0)
                if dist[p] >= 0:
                    assert applied(a, b, spans[p]) == b
                    assert ratebatch.Alignment(dist[p], spans[p, :n_spans[p]]).apply(letters(a), letters(b)) == letters(b)
                    if join == 0:
                        width = np.maximum(spans[p, :, 1] - spans[p, :, 0], spans[p, :, 3] - spans[p, :, 2])
                        assert width[:n_spans[p]].sum() == dist[p]
            statuses.update(dist.tolist())
    assert statuses == set(range(-1, 6))


def test_align_pairs_host_edges():
    K = 4
    base = list(range(10, 40))                      # 30 distinct symbols
    spaced = lambda count: [(-x if at % 6 == 2 and at // 6 < count else x) for at, x in enumerate(base)]
    A = [[], [], [1, 2, 3], base[:10], base[:10], base, base, base[:9], base, [5, 5], [7, 8, 9], [-3, 2 ** 20, 2 ** 31 - 1, -2 ** 31]]
    B = [[], [1, 2, 3], [], base[:10 + K], base[:10 + K + 1], spaced(K), spaced(K + 1), base[:8], base, [5, 5], [7, 8, 9, 9],
         [-3, 2 ** 20 + 1, 2 ** 31 - 1, -2 ** 31]]
    dist, n_spans, spans = got = host(A, B, 30, K, 0)
    for g, w in zip(got, full_pairs(A, B, 30, K, 0)):
        assert np.array_equal(g, w)
    assert dist.tolist() == [0, 3, 3, K, -1, K, -1, 1, 0, 0, 1, 1]
    assert n_spans.tolist() == [0, 1, 1, 1, 0, K, 0, 1, 0, 0, 1, 1]
    assert spans[1, 0].tolist() == [0, 0, 0, 3] and spans[2, 0].tolist() == [0, 3, 0, 0]      # one empty text: one span
    assert spans[3, 0].tolist() == [10, 10, 10, 14] and spans[7, 0].tolist() == [8, 9, 8, 8]
    assert spans[5, :, 0].tolist() == [2, 8, 14, 20] and spans[11, 0].tolist() == [1, 2, 1, 2]
    assert (spans[4] == -1).all() and (spans[8] == -1).all()
    # canonical: the walk from the end takes the diagonal first, so of a run of equal symbols the surplus one is the first
    assert spans[10, 0].tolist() == [2, 2, 2, 3]
    # a text longer than max_len: -2 for that pair, the neighbours as before
    short = host(A, B, 29, K, 0)
    assert short[0].tolist() == [0, 3, 3, K, -1, -2, -2, 1, -2, 0, 1, 1] and (short[2][5] == -1).all() and short[1][5] == 0
    keep = [p for p in range(len(A)) if p not in (5, 6, 8)]
    assert all(np.array_equal(s[keep], g[keep]) for s, g in zip(short, got))
    # offsets that descend or reach outside their pool
    a_pool, a_off = pooled(A)
    b_pool, b_off = pooled(B)
    bad = a_off.copy()
    bad[3] = bad[4] + 1
    wrong = ratebulk.align_pairs_host(a_pool, bad, b_pool, b_off, 30, K, 0)
    assert wrong[0][3] == -2 and wrong[0][:2].tolist() == [0, 3] and wrong[0][4:].tolist() == dist[4:].tolist()
    assert ratebulk.align_pairs_host(a_pool[:-1], a_off, b_pool, b_off, 30, K, 0)[0].tolist() == dist.tolist()[:-1] + [-2]
    # join: differences 1, 2 and 4 symbols apart
    a = list(range(100, 130))
    b = list(a)
    for at in (3, 5, 10, 13, 20, 25):
        b[at] = -b[at]
    counts = [host([a], [b], 30, 8, join)[1][0] for join in (0, 1, 2, 3, 4)]
    assert counts == [6, 5, 4, 4, 2]
    assert host([a], [b], 30, 8, 1)[2][0, 0].tolist() == [3, 6, 3, 6]
    for wrong in (dict(max_len=-1), dict(max_len=4097), dict(max_dist=0), dict(max_dist=256), dict(join=-1)):
        with pytest.raises(ValueError):
            ratebulk.align_pairs_host(a_pool, a_off, b_pool, b_off, **dict(dict(max_len=30, max_dist=K, join=0), **wrong))
    with pytest.raises(ValueError):
        ratebulk.align_pairs_host(a_pool, a_off, b_pool, b_off[:-1], 30, K, 0)


def test_alignment_strings_and_apply():
    one = ratebatch.Alignment(np.int32(3), np.array([[1, 2, 1, 1], [4, 4, 3, 5]], dtype=np.int32))
    assert one.dist == 3 and len(one) == 2
    assert one.strings("abcdef", "acdXYef") == [("b", ""), ("", "XY")] and one.apply("abcdef", "acdXYef") == "acdXYef"


# ---------------------------------------------------------------------------------------------- witness_edits
def spans_of(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def test_witness_edits_pools_orders_and_counts():
    texts = ["the quick brown fox", "second line", "third"]
    witnesses = [["the quiek brown f0x", "the quack brown fox", "the quick brown fox"], [], ["something else", "Third", "th" + "x" * 65 + "ird"]]
    pairs = [(2, 0), (0, 0), (0, 1), (0, 2), (2, 1), (2, 2)]
    alignments = [ratebatch.Alignment(-1, spans_of([])),
                  ratebatch.Alignment(2, spans_of([[7, 8, 7, 8], [17, 18, 17, 18]])),
                  ratebatch.Alignment(1, spans_of([[6, 7, 6, 7]])),
                  ratebatch.Alignment(0, spans_of([])),                       # a witness equal to the text: no edit
                  ratebatch.Alignment(1, spans_of([[0, 1, 0, 1]])),
                  ratebatch.Alignment(65, spans_of([[2, 2, 2, 67]]))]
    edits, skipped = ratebatch.witness_edits(alignments, pairs, texts, witnesses)
    assert edits == [(0, 6, 7, ["a"]), (0, 7, 8, ["e"]), (0, 17, 18, ["0"])]
    assert skipped == dict(different=1, first=1, long=1)
    assert ratebatch.witness_edits(alignments, pairs, texts, witnesses, max_len=65)[0][-1] == (2, 2, 2, ["x" * 65])
    # the same span from two witnesses: readings pooled, first seen first, duplicates dropped; overlapping spans stay apart
    witnesses = [["abXdef", "abYdef", "abXdef", "aQQdef"]]
    alignments = [ratebatch.Alignment(1, spans_of([[2, 3, 2, 3]]))] * 3 + [ratebatch.Alignment(2, spans_of([[1, 3, 1, 3]]))]
    edits, skipped = ratebatch.witness_edits(alignments, [(0, 0), (0, 1), (0, 2), (0, 3)], ["abcdef"], witnesses)
    assert edits == [(0, 1, 3, ["QQ"]), (0, 2, 3, ["X", "Y"])] and skipped == dict(different=0, first=0, long=0)
    assert ratebatch.witness_edits([], [], ["a"], [[]]) == ([], dict(different=0, first=0, long=0))
    with pytest.raises(ValueError):
        ratebatch.witness_edits(alignments, [(0, 0)], ["abcdef"], witnesses)
    with pytest.raises(ValueError):
        ratebatch.witness_edits([], [], ["a", "b"], [[]])


# ---------------------------------------------------------------------------------------------- the Rater on the double
def noisy(rng, text, edits):
    out = list(text)
    for _ in range(edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(1, len(out)))
        if op == 0:
            out[at] = random_text(rng, 1)
        elif op == 1 and len(out) > 2:
            del out[at]
        else:
            out.insert(at, random_text(rng, 1))
    return "".join(out)


def witness_corpus(seed):
    """eight texts with 0 .. 3 witnesses each: equal ones, near ones, one too far, an empty text"""
    rng = np.random.default_rng(seed)
    texts = [random_text(rng, size) for size in (40, 33, 0, 25, 60, 18, 30, 50)]
    witnesses = [[noisy(rng, t, int(rng.integers(0, 4))) for _ in range(i % 4)] if t else [""] for i, t in enumerate(texts)]
    witnesses[5][0] = random_text(rng, 20)                  # another text altogether
    witnesses[6][0] = texts[6]                              # the same reading
    return texts, witnesses, [[170 + i] for i in range(len(texts))]


def test_rater_align_on_the_double():
    r = small_rater(OracleLM, length=LENGTH)
    texts, witnesses, _ = witness_corpus(5)
    pairs = [(i, w) for i, ws in enumerate(witnesses) for w in range(len(ws))]
    a, b = [texts[i] for i, _ in pairs], [witnesses[i][w] for i, w in pairs]
    a += ["été", "\U0001F600x", ""]            # decomposed accents are composed first; astral code points
    b += ["été", "\U0001F601x", "ab"]
    for join in (0, 2):
        got = r.align(iter(a), iter(b), max_dist=6, join=join)
        codes = lambda strings: pooled([[ord(c) for c in windows.normalize(s)] for s in strings])
        dist, n_spans, spans = ratebulk.align_pairs_host(*codes(a), *codes(b), 60, 6, join)
        assert len(got) == len(a) and all(type(one) is ratebatch.Alignment for one in got)
        for p, one in enumerate(got):
            assert one.dist == dist[p] and one.spans.dtype == np.int32 and np.array_equal(one.spans, spans[p, :n_spans[p]])
            if one.dist >= 0:
                assert one.apply(windows.normalize(a[p]), windows.normalize(b[p])) == windows.normalize(b[p])
        assert got[-3].dist == 0 and got[-2].dist == 1 and got[-2].spans.tolist() == [[0, 1, 0, 1]] and got[-1].strings("", "ab") == [("", "ab")]
        assert sorted(set(one.dist for one in got))[0] == -1 and any(one.dist == 0 for one in got[:-3])
    assert r.align([], []) == []
    assert r.align(["a" * 4096], ["a" * 4095 + "b"], max_dist=1)[0].spans.tolist() == [[4095, 4096, 4095, 4096]]
    for wrong in (dict(texts=["a" * 4097]), dict(others=["a" * 4097]), dict(others=["a", "b"]), dict(max_dist=0), dict(max_dist=256),
                  dict(join=-1)):
        with pytest.raises(ValueError):
            r.align(**dict(dict(texts=["abc"], others=["abd"]), **wrong))


def test_merge_witnesses_is_the_composed_call():
    r = small_rater(OracleLM, length=LENGTH)
    texts, witnesses, contexts = witness_corpus(6)
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.25)
    pairs = [(i, w) for i, ws in enumerate(witnesses) for w in range(len(ws))]
    for precision in ("bf16", "split"):
        alignments, rescored, skipped = r.merge_witnesses(texts, witnesses, contexts, max_dist=5, join=1, precision=precision, **rescoring)
        flat = r.align([texts[i] for i, _ in pairs], [witnesses[i][w] for i, w in pairs], max_dist=5, join=1)
        edits, ref_skipped = ratebatch.witness_edits(flat, pairs, texts, witnesses)
        same_rescored(rescored, r.rescore(texts, edits, contexts, precision=precision, **rescoring))
        assert skipped == ref_skipped and skipped["different"] == 1 and len(edits) > 5
        assert [len(one) for one in alignments] == [len(ws) for ws in witnesses]
        assert [one.dist for per in alignments for one in per] == [one.dist for one in flat]
        assert sum(len(one) for one in rescored) == len(edits)
    assert r.merge_witnesses(texts, witnesses, contexts, **rescoring)[0][1][0].dist == flat[0].dist      # join defaults to 1
    none = r.merge_witnesses(["ab", ""], [[], []])
    assert none[0] == [[], []] and [len(one) for one in none[1]] == [0, 0] and none[2] == dict(different=0, first=0, long=0)
    for wrong in (dict(witnesses=[["abd"], []]), dict(max_dist=0), dict(max_dist=256), dict(join=-1), dict(left=0), dict(ahead=-1),
                  dict(precision="f32"), dict(witnesses=[["a" * 4097]])):
        with pytest.raises(ValueError):
            r.merge_witnesses(**dict(dict(texts=["abc"], witnesses=[["abd"]]), **wrong))
    r.stateful = False
    with pytest.raises(ValueError):
        r.merge_witnesses(["abc"], [["abd"]])
    assert r.align(["abc"], ["abd"])[0].dist == 1                # `align` needs a loaded engine only


def test_merge_witnesses_proposes_the_reading_the_model_prefers():
    """a planted error whose repair the double's model prefers -- found by rating the repair directly --: the witness that holds
    the clean reading makes `merge_witnesses` propose exactly that repair, and `apply` gives the clean text"""
    r = small_rater(OracleLM, length=LENGTH)
    rng = np.random.default_rng(7)
    clean = random_text(rng, 48)
    rescoring = dict(streams=4, left=16, ahead=4, min_gain=0.25)      # (the double's weights are random: gains are small)
    planted = None
    for at in range(8, 40):
        wrong = [c for c in "abcdefgh" if c != clean[at]][at % 7]
        text = clean[:at] + wrong + clean[at + 1:]
        direct = r.rescore([text], [(0, at, at + 1, [clean[at]])], **rescoring)[0]
        if direct.best[0] == 0:
            planted = (at, text, direct)
            break
    assert planted is not None
    at, text, direct = planted
    alignments, rescored, skipped = r.merge_witnesses([text], [[clean, text]], **rescoring)
    assert [one.dist for one in alignments[0]] == [1, 0] and alignments[0][0].spans.tolist() == [[at, at + 1, at, at + 1]]
    one = rescored[0]
    assert one.starts.tolist() == [at] and one.ends.tolist() == [at + 1] and one.proposals() == [clean[at]]
    assert one.gain[0] == direct.gain[0] >= 0.25 and one.apply(text) == clean


# ---------------------------------------------------------------------------------------------- command line
def test_cli_witnesses(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    assert run.COMMAND_ORDER.index("witnesses") == run.COMMAND_ORDER.index("lexicon") + 1
    r = small_rater(OracleLM, length=LENGTH)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    rng = np.random.default_rng(8)
    first, second = tmp_path / "engine2", tmp_path / "engine3"
    first.mkdir()
    second.mkdir()
    files, texts, readings = [], [], []
    for i, size in enumerate((60, 1, 80)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
        readings.append([])
        for directory in ((first, second) if i != 1 else (second,)):          # file 1 has no witness in the first directory
            readings[-1].append(noisy(rng, texts[-1], 3) if size > 1 else texts[-1])
            (directory / name.name).write_text(readings[-1][-1])
    contexts = [[170], [174], [178]]
    options = ["-s", "2", "--precision", "split", "--max-dist", "8", "--join", "1", "--left", "10", "--ahead", "2", "--min-gain", "0.25"]
    base = ["witnesses", "-m", str(model)]
    res = CliRunner().invoke(run.cli, base + ["--witness", str(first), "--witness", str(second), "--apply"] + options + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    assert all(sorted(l) == ["chars", "corrected", "file", "rescored", "skipped", "witnesses"] for l in lines)
    ref = small_rater(OracleLM, length=LENGTH)
    alignments, found, skipped = ref.merge_witnesses(texts, readings, contexts, max_dist=8, join=1, left=10, ahead=2, min_gain=0.25,
                                                     streams=2, precision="split")
    assert sum(len(f) for f in found) > 0
    total = dict(different=0, first=0, long=0)
    for i, (line, text, one) in enumerate(zip(lines, texts, found)):
        assert line["chars"] == len(text) and line["corrected"] == one.apply(text)
        assert line["rescored"] == [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                                    for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
        assert [w["dist"] for w in line["witnesses"]] == [al.dist for al in alignments[i]]
        for reason in total:
            total[reason] += line["skipped"][reason]
    assert total == skipped
    assert [w["file"] for w in lines[0]["witnesses"]] == [str(first / "auth_title0_1700.txt"), str(second / "auth_title0_1700.txt")]
    assert [w["file"] for w in lines[1]["witnesses"]] == [str(second / "auth_title1_1740.txt")]      # the missing one is simply absent
    assert lines[1]["witnesses"][0]["dist"] == 0 and lines[1]["rescored"] == [] and lines[1]["corrected"] == texts[1]
    plain = CliRunner().invoke(run.cli, base + ["--witness", str(first)] + options + files)
    assert plain.exit_code == 0 and "corrected" not in json.loads(plain.output.strip().split("\n")[0])
    # usage errors
    assert CliRunner().invoke(run.cli, base + files).exit_code != 0                                         # no --witness
    assert CliRunner().invoke(run.cli, base + ["--witness", str(tmp_path / "none")] + files).exit_code != 0
    for wrong in (["--max-dist", "0"], ["--max-dist", "256"], ["--join", "-1"], ["--precision", "f32"], ["--left", "0"], ["--ahead", "-1"]):
        assert CliRunner().invoke(run.cli, base + ["--witness", str(first)] + wrong + files).exit_code != 0, wrong
    long = tmp_path / "long_1800.txt"
    long.write_text("a" * 4097)
    (first / long.name).write_text("a" * 4090)
    too_long = CliRunner().invoke(run.cli, base + ["--witness", str(first)] + options + [str(long)])
    assert too_long.exit_code == 2 and "4096" in too_long.output                                            # a click.UsageError
