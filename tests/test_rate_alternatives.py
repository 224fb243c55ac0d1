"""`ratebatch.alternatives_of`, `Rater.rate_alternatives` and `keraslm-rate apply --alternatives` on the CPU.

The oracle-backed engine double has no `rate_window_alts`, so the Rater runs through `forward_window` and the numpy
statement of the selection (`alternatives_of`) -- the scheduler, the per-text slicing and the bookkeeping are the
product's.  The device selection itself is held to the same statement in test_rate_alternatives_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, windows
from tests import test_rate_batch as tb
from tests.oracle_engine import OracleLM


def test_alternatives_of_ties_resolve_to_the_lower_id():
    full = np.array([[[0.1, 0.3, 0.3, 0.2, 0.1],      # 1 and 2 tied at the top, 0 and 4 tied at the bottom
                      [0.2, 0.2, 0.2, 0.2, 0.2],      # all equal: the id order
                      [0.0, 0.0, 0.0, 1.0, 0.0]]])    # everything but the winner at 0: still in id order
    y = np.array([[2, 3, 4]])
    tprob, ids, probs, rank = ratebatch.alternatives_of(full, y, 4)
    assert ids.dtype == np.int32 and rank.dtype == np.int32 and probs.dtype == full.dtype
    assert ids.tolist() == [[[1, 2, 3, 0], [0, 1, 2, 3], [3, 0, 1, 2]]]
    assert probs.tolist() == [[[0.3, 0.3, 0.2, 0.1], [0.2, 0.2, 0.2, 0.2], [1.0, 0.0, 0.0, 0.0]]]
    # a tied target's rank is counted by id: 2 stands behind 1; 3 behind 0, 1, 2; 4 behind 3 and the ids 0, 1, 2
    assert rank.tolist() == [[1, 3, 4]]
    assert tprob.tolist() == [[0.3, 0.2, 0.0]]
    for t in range(3):      # rank < k: the target is among the alternatives, with its own probability
        if rank[0, t] < 4:
            assert ids[0, t, rank[0, t]] == y[0, t] and probs[0, t, rank[0, t]] == tprob[0, t]


def test_alternatives_of_pads_beyond_the_vocabulary():
    full = np.array([[[0.5, 0.1, 0.4]]], dtype=np.float32)
    tprob, ids, probs, rank = ratebatch.alternatives_of(full, np.array([[1]]), 5)
    assert ids.tolist() == [[[0, 2, 1, -1, -1]]]
    assert probs.tolist() == [[[np.float32(0.5), np.float32(0.4), np.float32(0.1), 0.0, 0.0]]]
    assert rank.tolist() == [[2]] and tprob[0, 0] == np.float32(0.1) and probs.dtype == np.float32


def test_alternatives_of_without_a_target_delivers_nothing():
    full = np.array([[[0.5, 0.1, 0.4], [0.2, 0.7, 0.1], [0.3, 0.3, 0.4]]])
    tprob, ids, probs, rank = ratebatch.alternatives_of(full, np.array([[-1, -2, 3]]), 2)
    assert ids[0, :2].tolist() == [[-1, -1], [-1, -1]] and not probs[0, :2].any()
    assert rank.tolist() == [[-1, -1, -1]] and tprob.tolist() == [[0.0, 0.0, 0.0]]
    # an id beyond the vocabulary is no target either (probability 0, no rank), but the position is a real one
    assert ids[0, 2].tolist() == [2, 0] and probs[0, 2].tolist() == [0.4, 0.3]


def brute_force(rater, texts, contexts, k):
    """one text at a time: reset, the whole softmax of every window of `stateful_windows`, `alternatives_of`"""
    out = []
    lm = rater.model
    for text, context in zip(texts, contexts):
        text = windows.normalize(text)
        n = len(text)
        lm.reset_states(1)
        parts = []
        for x, z, y in windows.stateful_windows(text, context, rater.length, rater.mapping[0]):
            parts.append(ratebatch.alternatives_of(np.asarray(lm.forward_window(x[None], z[None])), y[None], k))
        probs = np.ones(n, dtype=np.float32)
        rank = np.full(n, -1, dtype=np.int32)
        ids = np.full((n, k), -1, dtype=np.int32)
        alt = np.zeros((n, k), dtype=np.float32)
        if parts:
            probs[1:] = np.concatenate([p[0][0] for p in parts]).astype(np.float32)[:n - 1]
            ids[1:] = np.concatenate([p[1][0] for p in parts])[:n - 1]
            alt[1:] = np.concatenate([p[2][0] for p in parts]).astype(np.float32)[:n - 1]
            rank[1:] = np.concatenate([p[3][0] for p in parts])[:n - 1]
        out.append((probs, rank, ids, alt))
    return out


@pytest.fixture(scope="module")
def reference():
    """rate_batch's results and the brute-force loop at the largest k (its first columns are the smaller k's), computed once"""
    r = tb.make_rater(OracleLM, True, False)
    texts, contexts = tb.contract_texts(r.length)
    batch = dict((streams, r.rate_batch(texts, contexts, streams=streams)) for streams in (1, 3, 64))
    return texts, contexts, batch, brute_force(tb.make_rater(OracleLM, True, False), texts, contexts, 8)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("streams", [1, 3, 64])
def test_rate_alternatives_contract(reference, streams, k):
    texts, contexts, batch, brute = reference
    r = tb.make_rater(OracleLM, True, False)
    r.rate(texts[6], contexts[6])            # (a carried state the call must not continue)
    rated, bits = r.rate_alternatives(texts, contexts, k=k, streams=streams)
    ref_probs, ref_bits = batch[streams]
    assert len(rated) == len(texts) and bits.dtype == np.float64 and bits.tolist() == ref_bits.tolist()
    voc = r.voc_size
    for i, t in enumerate(texts):
        one, n = rated[i], len(windows.normalize(t))
        probs, rank, ids, alt = brute[i]
        assert len(one) == n
        assert one.probs.dtype == np.float32 and one.probs.shape == (n,)
        assert one.rank.dtype == np.int32 and one.rank.shape == (n,)
        assert one.alt_ids.dtype == np.int32 and one.alt_ids.shape == (n, k)
        assert one.alt_probs.dtype == np.float32 and one.alt_probs.shape == (n, k)
        assert np.array_equal(one.probs, ref_probs[i]), i
        assert np.array_equal(one.probs, probs), i
        assert np.array_equal(one.rank, rank), i
        assert np.array_equal(one.alt_ids, ids[:, :k]), i
        assert np.array_equal(one.alt_probs, alt[:, :k]), i
        if n:       # the first character has no prediction
            assert one.probs[0] == 1.0 and one.rank[0] == -1 and (one.alt_ids[0] == -1).all() and not one.alt_probs[0].any()
        assert ((one.rank[1:] >= 0) & (one.rank[1:] < voc)).all()
        assert (np.diff(one.alt_probs[1:], axis=1) <= 0).all()
        hit = one.rank[1:] < k
        at = np.nonzero(hit)[0] + 1
        assert np.array_equal(one.alt_probs[at, one.rank[at]], one.probs[at])
        chars = one.chars(r.mapping)
        assert len(chars) == n and all(len(c) == k for c in chars)
        assert chars == one.chars(r.mapping[1])
        for row, names in zip(one.alt_ids, chars):
            assert names == [None if v < 0 else ("" if v == 0 else r.mapping[1][int(v)]) for v in row]
    assert len(rated[0]) == 0 and bits[0] == 0.0                      # the empty text
    assert rated[1].probs.tolist() == [1.0] and bits[1] == 0.0        # one character
    # afterwards: one reset row
    assert all(s.shape[0] == 1 and not s.any() for s in r.model.states)


def test_rate_alternatives_without_a_single_window():
    r = tb.make_rater(OracleLM, True, False)
    rated, bits = r.rate_alternatives(["", "a"], k=2)
    assert [len(x) for x in rated] == [0, 1] and not bits.any()
    assert rated[1].alt_ids.tolist() == [[-1, -1]] and rated[1].rank.tolist() == [-1]
    assert all(s.shape[0] == 1 and not s.any() for s in r.model.states)


def test_rate_alternatives_one_context_for_all_and_none():
    r = tb.make_rater(OracleLM, True, False)
    texts, _ = tb.contract_texts(r.length)
    for contexts in ([23], None):
        probs, bits = r.rate_batch(texts[5:8], contexts, streams=2)
        rated, bits2 = r.rate_alternatives(texts[5:8], contexts, k=2, streams=2)
        assert bits2.tolist() == bits.tolist()
        assert all(np.array_equal(a.probs, b) for a, b in zip(rated, probs))


def test_rate_alternatives_asserts():
    with pytest.raises(AssertionError):
        tb.make_rater(OracleLM, False, False).rate_alternatives(["abc"])      # stateless
    with pytest.raises(AssertionError):
        tb.make_rater(OracleLM, False, True).rate_alternatives(["abc"])       # incremental
    r = tb.make_rater(OracleLM, True, False)
    for k in (0, 9):
        with pytest.raises(AssertionError):
            r.rate_alternatives(["abc"], k=k)


def test_cli_apply_alternatives(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    option = [p for p in run.apply.params if p.name == "alternatives"]
    assert len(option) == 1 and option[0].default is None and "--alternatives" in option[0].opts      # off by default
    r = tb.make_rater(OracleLM, True, False)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    text = tb.random_text(np.random.default_rng(3), r.length + 4)
    res = CliRunner().invoke(run.cli, ["apply", "-m", str(model), "-c", "1784", "--alternatives", "2", text])
    assert res.exit_code == 0, res.output
    lines = res.output.strip().split("\n")
    assert len(lines) == 2
    listed = json.loads(lines[1])
    rated, bits = tb.make_rater(OracleLM, True, False).rate_alternatives([text], [[179]], k=2)
    assert float(lines[0]) == 2.0 ** (bits[0] / len(text))
    assert len(listed) == len(text)
    for i, (char, prob, rank, alts) in enumerate(listed):
        assert char == text[i] and prob == float(rated[0].probs[i]) and rank == int(rated[0].rank[i])
        assert len(alts) == 2
        for j, (c, p) in enumerate(alts):
            v = int(rated[0].alt_ids[i, j])
            assert c == (None if v < 0 else r.mapping[1].get(v, "")) and p == float(rated[0].alt_probs[i, j])
    for k in ("0", "9"):
        assert CliRunner().invoke(run.cli, ["apply", "-m", str(model), "--alternatives", k, text]).exit_code != 0
