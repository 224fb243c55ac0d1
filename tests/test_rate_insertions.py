"""Insertion hypotheses of `Rater.corrections` on the CPU: `ratebulk.variant_windows_host(insertions=1)`, the `best_op`, `edits`
and `apply` of `ratebatch.Corrections`, `Rater.corrections(insertions=True)` on the oracle-backed engine double and
`keraslm-rate correct --insertions`.

An insertion variant puts an alternative IN FRONT of the written character: for a character the text has lost.  The numpy
statement is held to rows built from Python lists, every cost to a fresh one-row window over the hypothesis; kl_edit_windows
and the device path are held to the same statements in test_rate_insertions_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import small_rater
from tests.test_rate_corrections import LENGTH, brute_row, fresh_cost, same_suspects, variant_corpus, variant_suspects
from tests.test_rate_suspects import contract_texts

Cor = ratebatch.Corrections


def kind_of(v, K, deletions):
    """("written" | "substitute" | "delete" | "insert", index of the alternative or None)"""
    if v == 0:
        return "written", None
    if v <= K:
        return "substitute", v - 1
    if deletions and v == K + 1:
        return "delete", None
    return "insert", v - (K + 1 + deletions)


def brute_edit_row(corpus, offsets, text_ctx, g, alts, v, left, ahead, deletions, T):
    """one row of the definition from Python lists: (idx [T], ctx [T][n_ctx], tgt [T], valid, L, A); the rows that are not
    insertions are test_rate_corrections' brute_row"""
    K = len(alts)
    kind, j = kind_of(v, K, deletions)
    if kind != "insert":
        return brute_row(corpus, offsets, text_ctx, g, alts, v, left, ahead, T)
    n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
    written = brute_row(corpus, offsets, text_ctx, g, alts, 0, left, ahead, T)
    L, A = written[4], written[5]
    a = int(alts[j])
    if not written[3] or a < 0:
        return [0] * T, [[0] * n_ctx for _ in range(T)], [-1] * T, 0, L, A
    x = [int(c) for c in corpus]
    q = x[g - L:g] + [a, x[g]] + x[g + 1:g + 1 + A]
    assert len(q) == L + 2 + A
    fed = len(q) - 1
    idx = q[:fed] + [0] * (T - fed)
    tgt = [-1] * T
    for t in range(L - 1, fed):
        tgt[t] = q[t + 1]
    i = [i for i in range(len(offsets) - 1) if offsets[i] <= g < offsets[i + 1]][0]
    ctx = [[int(c) for c in text_ctx[i]] if n_ctx else [] for _ in range(fed)] + [[0] * n_ctx for _ in range(T - fed)]
    return idx, ctx, tgt, 1, L, A


# ---------------------------------------------------------------------------------------------- the numpy statement
@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("deletions", [0, 1])
def test_variant_windows_host_insertions_against_brute_force(deletions, n_ctx):
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = variant_suspects(corpus, offsets)
    S, K = alts.shape
    R0 = K + 1 + deletions
    R = R0 + K
    for left, ahead, T in ((5, 4, 10), (5, 4, 13), (1, 0, 3), (7, 0, 8)):
        seen = set()
        idx, ctx, tgt, valid = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T,
                                                             insertions=1)
        assert idx.shape == tgt.shape == (S * R, T) and ctx.shape == (S * R, T, n_ctx) and valid.shape == (S * R,)
        assert idx.dtype == ctx.dtype == tgt.dtype == valid.dtype == np.int32
        # the rows v <= K + deletions are those without insertions, word for word
        old = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T)
        for new, ref in zip((idx, ctx, tgt, valid), old):
            new, ref = new.reshape((S, R) + new.shape[1:]), ref.reshape((S, R0) + ref.shape[1:])
            assert np.array_equal(new[:, :R0], ref)
        for s, g in enumerate(pos):
            g = int(g)
            for v in range(R):
                b = s * R + v
                want = brute_edit_row(corpus, offsets, text_ctx, g, alts[s], v, left, ahead, deletions, T)
                assert idx[b].tolist() == want[0], (left, ahead, T, s, v)
                assert ctx[b].tolist() == want[1], (left, ahead, T, s, v)
                assert tgt[b].tolist() == want[2], (left, ahead, T, s, v)
                assert int(valid[b]) == want[3]
                kind, j = kind_of(v, K, deletions)
                if kind != "insert":
                    continue
                L, A = want[4], want[5]
                a = int(alts[s, j])
                if L is None:
                    seen.add("outside")
                    assert not want[3]
                elif L == 0:
                    seen.add("L==0")
                    assert not want[3]
                elif a < 0:
                    seen.add("a<0")
                    assert not want[3]
                else:
                    assert want[3]
                    seen.add("a==w" if a == corpus[g] else "a!=w")
                    # the targets: the inserted character, the written one and the A characters after it
                    assert (tgt[b] >= 0).sum() == A + 2
                    assert tgt[b, L - 1] == a and tgt[b, L] == corpus[g] and idx[b, L] == a
                    if A == 0:
                        seen.add("A==0")
                        assert (tgt[b] >= 0).sum() == 2
                    if L + 1 + A == T:
                        seen.add("full row")
        assert {"outside", "L==0", "a<0", "a==w", "a!=w", "A==0"} <= seen, seen
        if T == left + ahead + 1:
            assert "full row" in seen
    for bad in (dict(T=9), dict(T=1025), dict(insertions=2), dict(insertions=-1), dict(deletions=2), dict(left=0)):
        a = dict(dict(left=5, ahead=4, deletions=0, T=10, insertions=1), **bad)
        with pytest.raises(ValueError):
            ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, a["left"], a["ahead"], a["deletions"], a["T"],
                                          insertions=a["insertions"])
    # (T = left + ahead is enough without insertions, T = 1024 is allowed with them)
    ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, 5, 4, 0, 9, insertions=0)
    ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos[:2], alts[:2], 1000, 23, 0, 1024, insertions=1)


def test_variant_pick_orders_substitution_deletion_insertion():
    """equal costs: the smallest v -- a substitution before the deletion before an insertion, within a kind by rank"""
    # k = 2 with deletions -- v: 0 written, 1 2 substituted, 3 dropped, 4 5 inserted
    cost = np.array([[9.0, 4.0, 4.0, 4.0, 4.0, 4.0], [9.0, 5.0, 5.0, 4.0, 4.0, 4.0], [9.0, 5.0, 5.0, 5.0, 4.0, 4.0],
                     [9.0, 5.0, 5.0, 5.0, 5.0, 4.0]])
    _, best, gain = ratebulk.variant_pick_host(cost, np.ones(cost.shape, dtype=np.int32))
    assert best.tolist() == [1, 3, 4, 5] and gain.tolist() == [5.0, 5.0, 5.0, 5.0]


# ---------------------------------------------------------------------------------------------- the record
def test_corrections_best_op_edits_and_apply():
    mapping = ({"a": 1, "b": 2, "c": 3}, {1: "a", 2: "b", 3: "c"})
    k = 2
    # best_op is derived from best_id where it is not given: every construction from before it keeps working
    old = Cor(np.array([1, 3, 4, 6], dtype=np.int64), np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.int32),
              np.zeros((4, k), dtype=np.int32), np.zeros((4, k), dtype=np.float32), np.zeros((4, k + 2)),
              np.array([3, -2, -1, 0], dtype=np.int32), np.array([2.0, 1.5, 0.0, 3.0]))
    assert (Cor.OP_NONE, Cor.OP_SUBSTITUTE, Cor.OP_DELETE, Cor.OP_INSERT) == (0, 1, 2, 3)
    assert old.best_op.dtype == np.int32 and old.best_op.tolist() == [Cor.OP_SUBSTITUTE, Cor.OP_DELETE, Cor.OP_NONE, Cor.OP_SUBSTITUTE]
    #       0123456
    text = "abacaba"
    assert old.edits(text, mapping) == ["c", "", None, None] == old.proposals(mapping)
    assert old.apply(text, mapping) == "acaaba"
    # all four ops, an insertion of the unmapped id 0, edits at the neighbouring positions 1, 2 and 3, a position outside
    m = 7
    one = Cor(np.array([1, 2, 3, 4, 5, 6, 9], dtype=np.int64), np.zeros(m, dtype=np.float32), np.ones(m, dtype=np.int32),
              np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.float32), np.zeros((m, 2 * k + 2)),
              np.array([3, 2, -2, -1, 0, 1, 2], dtype=np.int32), np.array([2.0, 1.0, 1.5, 0.0, 3.0, 1.0, 1.0]),
              np.array([Cor.OP_INSERT, Cor.OP_SUBSTITUTE, Cor.OP_DELETE, Cor.OP_NONE, Cor.OP_INSERT, Cor.OP_INSERT, Cor.OP_INSERT],
                       dtype=np.int32))
    assert isinstance(one, ratebatch.Suspects) and len(one) == m
    # proposals keeps its contract: the character substituted or inserted, "" for a deletion, None without one (or id 0)
    assert one.proposals(mapping) == ["c", "b", "", None, None, "a", "b"] == one.proposals(mapping[1])
    assert one.edits(text, mapping) == ["cb", "b", "", None, None, "aa", None] == one.edits(text, mapping[1])
    # 'b' -> 'cb', 'a' -> 'b', 'c' dropped, 'a' and 'b' kept, the last 'a' doubled: from right to left, positions stay true
    assert one.apply(text, mapping) == "a" + "cb" + "b" + "" + "a" + "b" + "aa" == "acbbabaa"
    none = Cor(*([a[:0] for a in (one.positions, one.probs, one.rank, one.alt_ids, one.alt_probs, one.cost, one.best_id, one.gain,
                                  one.best_op)]))
    assert none.edits(text, mapping) == [] and none.apply(text, mapping) == text and none.apply("", mapping) == ""
    derived = Cor(*([a[:0] for a in (one.positions, one.probs, one.rank, one.alt_ids, one.alt_probs, one.cost, one.best_id,
                                     one.gain)]))
    assert derived.best_op.shape == (0,) and derived.best_op.dtype == np.int32


# ---------------------------------------------------------------------------------------------- the Rater on the double
def fresh_edit_cost(r, ids, ctx, j, alts, v, left, ahead, deletions):
    """the cost of variant v of the suspect at position j of one text, by definition: a one-row window from a zero state over
    the hypothesis, nothing padded; None where there is no such variant.  Rows that are no insertions: fresh_cost."""
    K = len(alts)
    kind, a = kind_of(v, K, deletions)
    if kind != "insert":
        return fresh_cost(r, ids, ctx, j, alts, v, left, ahead)
    L, A = min(left, j), min(ahead, len(ids) - 1 - j)
    if L == 0 or alts[a] < 0:
        return None
    q = list(ids[j - L:j]) + [int(alts[a]), int(ids[j])] + list(ids[j + 1:j + 1 + A])
    x = np.array([q[:-1]], dtype=np.int32)
    z = np.tile(np.asarray(windows.clamp_context(ctx), dtype=np.int32)[None, None, :], (1, x.shape[1], 1))
    r.model.reset_states(1)
    full = np.asarray(r.model.forward_window(x, z, want_probs=True), dtype=np.float64)[0]
    return float(-sum(np.log2(max(full[t, q[t + 1]], 1e-99)) for t in range(L - 1, len(q) - 1)))


def check_edits_against_definition(ref, texts, contexts, found, k, left, ahead, deletions, min_gain):
    R = 2 * k + 1 + deletions
    seen = dict((name, 0) for name in ("substitute", "delete", "insert", "none", "insert valid", "doubled"))
    for text, ctx, one in zip(texts, contexts, found):
        ids = windows.encode(windows.normalize(text), ref.mapping[0])
        assert one.cost.shape == (len(one), R) and one.cost.dtype == np.float64
        assert one.best_id.shape == one.gain.shape == one.best_op.shape == (len(one),)
        assert one.best_id.dtype == one.best_op.dtype == np.int32 and one.gain.dtype == np.float64
        for m, j in enumerate(one.positions):
            for v in range(R):
                want = fresh_edit_cost(ref, ids, ctx, int(j), one.alt_ids[m], v, left, ahead, deletions)
                if want is None:
                    assert one.cost[m, v] == np.inf
                else:
                    assert abs(one.cost[m, v] - want) <= 1e-9 * abs(want), (m, v)
                    kind, a = kind_of(v, k, deletions)
                    if kind == "insert":
                        seen["insert valid"] += 1
                        seen["doubled"] += int(one.alt_ids[m, a] == ids[int(j)])
            # best_id, best_op and gain follow from the costs the call returned
            _, best, gain = ratebulk.variant_pick_host(one.cost[m:m + 1], np.isfinite(one.cost[m:m + 1]))
            best, gain = int(best[0]), float(gain[0])
            if best == 0 or not gain >= min_gain:
                assert one.best_id[m] == Cor.NO_PROPOSAL and one.best_op[m] == Cor.OP_NONE and one.gain[m] == 0.0
                seen["none"] += 1
                continue
            kind, a = kind_of(best, k, deletions)
            assert one.gain[m] == gain
            assert one.best_op[m] == {"substitute": Cor.OP_SUBSTITUTE, "delete": Cor.OP_DELETE, "insert": Cor.OP_INSERT}[kind]
            assert one.best_id[m] == (Cor.DELETE if kind == "delete" else one.alt_ids[m, a])
            seen[kind] += 1
    return seen


def test_corrections_with_insertions_on_the_double_follow_the_definition():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    ref = small_rater(OracleLM, length=LENGTH)
    rated, _ = ref.rate_alternatives(texts, contexts, k=3, streams=4)
    median = float(np.median(np.concatenate([x.probs[1:] for x in rated])))
    k, left, ahead = 3, 5, 3
    total = {}
    # the suspects below the median probability; then every predicted character (the model's first choices among them: the
    # written character doubled is an insertion, though it is no substitution)
    for deletions, streams, precision, min_gain, max_prob, min_rank in ((True, 16, "bf16", 0.25, median, 1),
                                                                        (False, 7, "split", -np.inf, 1.0, 0)):
        args = dict(k=k, streams=streams, max_prob=max_prob, min_rank=min_rank, precision=precision)
        want, want_bits = ref.suspects(texts, contexts, **args)
        found, bits = r.corrections(texts, contexts, left=left, ahead=ahead, deletions=deletions, min_gain=min_gain, insertions=True,
                                    **args)
        assert np.array_equal(bits, want_bits)
        same_suspects(found, want)
        seen = check_edits_against_definition(ref, texts, contexts, found, k, left, ahead, int(deletions), min_gain)
        assert seen["insert valid"], seen
        for name, count in seen.items():
            total[name] = total.get(name, 0) + count
        # afterwards: a freshly reset single row
        assert r.model.states[0].shape[0] == 1 and not any(np.asarray(st).any() for st in r.model.states)
        # insertions=False is the call without the keyword, array for array; its variants are the first of the call with it
        off, off_bits = r.corrections(texts, contexts, left=left, ahead=ahead, deletions=deletions, min_gain=min_gain,
                                      insertions=False, **args)
        plain, plain_bits = r.corrections(texts, contexts, left=left, ahead=ahead, deletions=deletions, min_gain=min_gain, **args)
        assert np.array_equal(off_bits, plain_bits)
        R0 = k + 1 + int(deletions)
        for a, b, c in zip(off, plain, found):
            for name in ("positions", "probs", "rank", "alt_ids", "alt_probs", "cost", "best_id", "gain", "best_op"):
                x, y = getattr(a, name), getattr(b, name)
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
            assert a.cost.shape == (len(a), R0)
            derived = Cor(a.positions, a.probs, a.rank, a.alt_ids, a.alt_probs, a.cost, a.best_id, a.gain)
            assert np.array_equal(a.best_op, derived.best_op) and not (a.best_op == Cor.OP_INSERT).any()
            assert np.array_equal(np.isinf(a.cost), np.isinf(c.cost[:, :R0]))
            fin = np.isfinite(a.cost)
            assert (np.abs(a.cost[fin] - c.cost[:, :R0][fin]) <= 1e-9 * np.abs(a.cost[fin])).all()
    assert total["doubled"] and total["none"] and total["delete"] and total["insert"] + total["substitute"], total


def successor_rater():
    """a model that knows one thing: a b c d e f g h ' ' follow each other in a ring.  `small_rater` with hand-set weights --
    one-hot embeddings, no recurrence, input and output gates open, forget gates shut; layer 0 maps a character to its
    successor, layer 1 passes it on, the tied output layer reads it: about 0.995 for the successor."""
    from oracle import lstm_oracle as O
    r = small_rater(OracleLM, length=LENGTH)
    cfg = O.ModelConfig(2, 64, r.voc_size, 1)
    w = O.init_weights(cfg, seed=1, dtype=np.float32)
    W = cfg.width
    ring = "abcdefgh "
    follows = dict((r.mapping[0][a], r.mapping[0][b]) for a, b in zip(ring, ring[1:] + ring[0]))
    w["E"][:] = 0.0
    w["Ctx0"][:] = 0.0
    for i in range(r.voc_size):
        w["E"][i, i] = 10.0
    for l in range(2):
        w["K%d" % l][:] = 0.0
        w["U%d" % l][:] = 0.0
        b = w["b%d" % l]
        b[0:W], b[W:2 * W], b[2 * W:3 * W], b[3 * W:4 * W] = 10.0, -10.0, 0.0, 10.0
    for a, b in follows.items():
        w["K0"][a, 2 * W + b] = 1.0        # (the candidate g: tanh(10) at the successor's unit)
    for i in range(r.voc_size):
        w["K1"][i, 2 * W + i] = 10.0
    r.model.set_weights(w, 3)
    return r


def test_a_lost_character_is_put_back():
    """'abcdefgh abcdfgh': the second run has lost its 'e'.  The 'f' after 'd' is the one suspect; 'e' in its place makes the
    'g' after it unlikely, dropping it the 'g' after 'd', and only 'e' in front of it explains everything that follows.
    By the double: one suspect at position 13, 11.008 bits as written, 0.028 with the 'e' inserted, 11.001 with the 'f'
    dropped (a gain of 0.007: no proposal), 21.99 for every other variant."""
    r = successor_rater()
    text = "abcdefgh abcdfgh"
    k, left, ahead = 3, 6, 3
    args = dict(k=k, streams=16, max_prob=0.01, min_rank=1, left=left, ahead=ahead, deletions=True, min_gain=1.0, precision="split")
    (one,), _ = r.corrections([text], [[171]], insertions=True, **args)
    assert one.positions.tolist() == [13] and text[13] == "f"
    e = r.mapping[0]["e"]
    assert one.alt_ids[0, 0] == e and one.cost.shape == (1, 2 * k + 2)
    print("cost as written %.3f, variants %s" % (one.cost[0, 0], np.round(one.cost[0, 1:], 3).tolist()))
    assert int(np.argmin(one.cost[0, 1:])) + 1 == k + 2      # (v = k + 1 + deletions + 0: the first alternative inserted)
    assert one.best_op.tolist() == [Cor.OP_INSERT] and one.best_id.tolist() == [e] and one.gain[0] > 8.0
    assert one.gain[0] == one.cost[0, 0] - one.cost[0, k + 2]
    assert one.proposals(r.mapping) == ["e"] and one.edits(text, r.mapping) == ["ef"]
    assert one.apply(text, r.mapping) == "abcdefgh abcdefgh"
    # without insertions substitution and deletion read no better than the text as written: no proposal
    (old,), _ = r.corrections([text], [[171]], **args)
    assert old.positions.tolist() == [13] and old.best_id.tolist() == [Cor.NO_PROPOSAL] and old.best_op.tolist() == [Cor.OP_NONE]
    assert old.apply(text, r.mapping) == text


def test_corrections_insertions_edge_inputs_and_errors():
    r = small_rater(OracleLM, length=LENGTH)
    # texts without a prediction, and no suspects at all: empty arrays of the right shapes and dtypes
    for deletions, R in ((True, 6), (False, 5)):
        for texts, kw in ((["", "a"], {}), (["abcabc", "", "b"], dict(max_prob=0.0)), ([], {})):
            found, bits = r.corrections(texts, k=2, deletions=deletions, insertions=True, **kw)
            want, want_bits = r.suspects(texts, k=2, **kw)
            assert np.array_equal(bits, want_bits) and len(found) == len(texts)
            same_suspects(found, want)
            for one in found:
                assert len(one) == 0 and one.cost.shape == (0, R) and one.cost.dtype == np.float64
                assert one.best_id.shape == (0,) and one.best_id.dtype == np.int32
                assert one.best_op.shape == (0,) and one.best_op.dtype == np.int32
                assert one.gain.shape == (0,) and one.gain.dtype == np.float64
                assert one.edits("abc", r.mapping) == [] and one.apply("abc", r.mapping) == "abc"
    with pytest.raises(ValueError):
        r.corrections(["abcabcabc"], left=1000, ahead=24, max_prob=1.0, min_rank=0, insertions=True)      # (1025)
    for bad in (dict(left=0), dict(ahead=-1), dict(precision="f32")):
        with pytest.raises(ValueError):
            r.corrections(["abc"], insertions=True, **bad)
    found, _ = r.corrections(["abcabcabc"], left=1000, ahead=23, max_prob=1.0, min_rank=0, insertions=True)      # (1024 is allowed)
    assert found[0].cost.shape == (8, 7) and found[0].best_op.dtype == np.int32
    r.corrections(["abcabcabc"], left=1000, ahead=24, max_prob=1.0, min_rank=0)                              # (and without)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_correct_insertions(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    r = successor_rater()
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    texts = ["abcdefgh abcdfgh", "a", "fgh abcdefh abcd"]
    files = []
    for i, text in enumerate(texts):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        name.write_text(text)
        files.append(str(name))
    contexts = [[170], [174], [178]]
    ref = successor_rater()
    args = ["correct", "-m", str(model), "-s", "12", "--precision", "split", "-k", "2", "--max-prob", "0.01", "--min-rank", "1",
            "--left", "6", "--ahead", "3", "--deletions", "--min-gain", "0.5"]
    kw = dict(k=2, streams=12, max_prob=0.01, min_rank=1, left=6, ahead=3, deletions=True, min_gain=0.5, precision="split")
    outputs = {}
    for flag in ([], ["--insertions"]):
        found, bits = ref.corrections(texts, contexts, insertions=bool(flag), **kw)
        for extra in ([], ["--apply"]):
            res = CliRunner().invoke(run.cli, args + flag + extra + files)
            assert res.exit_code == 0, res.output
            outputs[bool(flag), bool(extra)] = res.output
            lines = [json.loads(l) for l in res.output.strip().split("\n")]
            assert [l["file"] for l in lines] == files
            for line, text, one, total in zip(lines, texts, found, bits):
                assert line["chars"] == len(text) and line["bits_per_char"] == float(total) / max(len(text) - 1, 1)
                assert [row[0] for row in line["suspects"]] == one.positions.tolist()
                assert [row[2] for row in line["corrections"]] == one.edits(text, ref.mapping)
                for (pos, written, new, gain), j, g in zip(line["corrections"], one.positions, one.gain):
                    assert pos == int(j) and written == text[pos] and gain == float(g)
                assert ("corrected" in line) == bool(extra)
                if extra:
                    assert line["corrected"] == one.apply(text, ref.mapping)
        if flag:
            # the lost 'e' and the lost 'g' come back: a two-character edit each
            assert [row[2] for row in lines[0]["corrections"]] == ["ef"] and lines[0]["corrected"] == "abcdefgh abcdefgh"
            assert "gh" in [row[2] for row in lines[2]["corrections"]] and lines[2]["corrected"] == "fgh abcdefgh abcd"
        else:
            # without the flag: the third field is the proposal, as it was -- null, "" or one character
            for line, one in zip(lines, found):
                assert [row[2] for row in line["corrections"]] == one.proposals(ref.mapping)
                assert all(row[2] is None or len(row[2]) <= 1 for row in line["corrections"])
    assert outputs[False, True] != outputs[True, True]
    res = CliRunner().invoke(run.cli, ["correct", "-m", str(model), "--left", "1000", "--ahead", "24", "--insertions"] + files[:1])
    assert res.exit_code == 2 and "must not exceed 1024" in res.output      # (a usage error)
    assert CliRunner().invoke(run.cli, ["correct", "-m", str(model), "--left", "1000", "--ahead", "24"] + files[:1]).exit_code == 0
