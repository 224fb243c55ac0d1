"""`Rater.rate_batch` and its scheduler (lib/ratebatch.py) on the CPU: the oracle-backed engine double has no
`rate_window`, so the batch runs through `forward_window` and a host-side pick -- the scheduler, the window
contents, the resets and the per-text bookkeeping are the product's.

Contract: `probs[i]` is what `model.reset_states(1); rate(texts[i], contexts[i])` returns, as a float32 array, and
`bits[i]` is -sum(log2(max(p, 1e-99))) over `probs[i][1:]`.  The loop's values are doubles here (the oracle computes
in f64), so they are compared AT the contract's dtype -- rounded to float32, the bits taken from the rounded values --
within the 1e-9 that test_rater_golden.py holds this engine double to."""
import json
import os
from math import ceil

import numpy as np
import pytest

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import Rater
from ocrd_keraslm_amd.lib import ratebatch, windows
from tests.oracle_engine import OracleLM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEAM = json.load(open(os.path.join(GOLD, "rater_seam.json")))


def make_rater(factory, stateful, incremental):
    """as tests/test_rater_golden.py builds it"""
    m = SEAM["model"]
    chars = m["chars"]
    r = Rater(engine_factory=factory)
    r.width, r.depth, r.length = m["width"], m["depth"], m["length"]
    r.stateful, r.incremental = stateful, incremental
    r.mapping = (dict((c, i) for i, c in enumerate(chars, 1)), dict((i, c) for i, c in enumerate(chars, 1)))
    r.voc_size = len(chars) + 1
    r.configure()
    cfg = O.ModelConfig(m["depth"], m["width"], r.voc_size, 1)
    w = O.init_weights(cfg, seed=m["seed"], emb_std=m["emb_std"], dtype=np.float64)
    r.model.set_weights(w, 3)
    r.status = 2
    if incremental:
        r.batch_size = 128
    return r


def random_text(rng, size, chars=None):
    chars = chars or SEAM["model"]["chars"]
    return "".join(chars[int(k)] for k in rng.integers(0, len(chars), size))


def contract_texts(length, chars=None):
    """the sizes around the window length, an unmapped character and a string that NFC changes; contexts that differ"""
    rng = np.random.default_rng(11)
    texts = [random_text(rng, s, chars) for s in (0, 1, 2, length - 1, length, length + 1, 2 * length + 1, 5 * length + 3)]
    unmapped = random_text(rng, length + 5, chars)
    texts.append(unmapped[:7] + "\u2603" + unmapped[7:])
    nfc = random_text(rng, length // 2 + 3, chars)
    texts.append(nfc[:3] + "a\u0308" + nfc[3:] + "e\u0301")      # (combining marks: NFC composes them)
    assert windows.normalize(texts[-1]) != texts[-1]
    contexts = [[(7 * i) % 200] for i in range(len(texts))]
    return texts, contexts


def loop(rater, texts, contexts):
    """the reset-and-rate loop, at the contract's dtype"""
    probs, bits = [], []
    for t, c in zip(texts, contexts):
        rater.model.reset_states(1)
        p = np.asarray(rater.rate(t, c), dtype=np.float64).astype(np.float32)
        probs.append(p)
        bits.append(-sum(np.log2(max(float(q), 1e-99)) for q in p[1:]))
    return probs, np.array(bits, dtype=np.float64)


@pytest.mark.parametrize("streams", [1, 3, 8, 64])
def test_rate_batch_contract(streams):
    r = make_rater(OracleLM, True, False)
    texts, contexts = contract_texts(r.length)
    ref_probs, ref_bits = loop(make_rater(OracleLM, True, False), texts, contexts)
    probs, bits = r.rate_batch(texts, contexts, streams=streams)
    assert len(probs) == len(texts) and bits.shape == (len(texts),) and bits.dtype == np.float64
    for i, t in enumerate(texts):
        assert isinstance(probs[i], np.ndarray) and probs[i].dtype == np.float32 and probs[i].ndim == 1
        assert len(probs[i]) == len(windows.normalize(t)) == len(ref_probs[i])
        if len(probs[i]):
            assert probs[i][0] == 1.0
            assert np.abs(probs[i].astype(np.float64) - ref_probs[i]).max() < 1e-9, i
        assert abs(bits[i] - ref_bits[i]) <= 1e-9 * abs(ref_bits[i]), i
    assert probs[0].size == 0 and bits[0] == 0.0
    assert probs[1].tolist() == [1.0] and bits[1] == 0.0
    # one context for all texts, and none
    one, one_bits = r.rate_batch(texts[5:8], [23], streams=streams)
    ref_one, ref_one_bits = loop(make_rater(OracleLM, True, False), texts[5:8], [[23]] * 3)
    none, _ = r.rate_batch(texts[5:8], streams=streams)
    ref_none, _ = loop(make_rater(OracleLM, True, False), texts[5:8], [None] * 3)
    for a, b, c, d in zip(one, ref_one, none, ref_none):
        assert np.abs(a.astype(np.float64) - b).max() < 1e-9
        assert np.abs(c.astype(np.float64) - d).max() < 1e-9
    assert np.all(np.abs(one_bits - ref_one_bits) <= 1e-9 * np.abs(ref_one_bits))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 4, 16])
def test_scheduler_alone(seed, B):
    """every text's windows, collected per row in call order, are `stateful_windows` of that text; the rows that are
    reset are exactly those that start a text; calls <= ceil(sum N_i / B) + max N_i (list scheduling)"""
    length = 12
    chars = SEAM["model"]["chars"]
    c_i = dict((c, i) for i, c in enumerate(chars, 1))
    rng = np.random.default_rng(100 + seed)
    sizes = [int(s) for s in rng.integers(0, 7 * length, 37)] + [0, 1, 2, length, length + 1, 9 * length + 5]
    texts = [random_text(rng, s) for s in sizes]
    contexts = [[int(rng.integers(0, 200))] for _ in texts]
    ids = [windows.encode(t, c_i) for t in texts]
    plan = ratebatch.plan(ids, contexts, length, B)
    counts = [windows.count_windows(s, length) for s in sizes]
    assert plan.B == min(B, sum(1 for c in counts if c))
    assert plan.n_calls <= ceil(sum(counts) / plan.B) + max(counts)
    assert plan.n_calls >= ceil(sum(counts) / plan.B)
    current = [None] * plan.B
    got = dict((i, []) for i in range(len(texts)))
    started = []
    for s in range(plan.n_calls):
        x, z, y = plan.call(s)
        assert x.shape == y.shape == (plan.B, length) and z.shape == (plan.B, length, 1)
        assert x.dtype == y.dtype == z.dtype == np.int32
        for i in plan.starting(s):
            r = int(plan.row[i])
            assert current[r] is None or len(got[current[r]]) == counts[current[r]], "row taken before its text ended"
            current[r] = i
            started.append(i)
        assert sorted(plan.reset_rows(s)) == sorted(int(plan.row[i]) for i in plan.starting(s))
        assert len(set(plan.reset_rows(s))) == len(plan.reset_rows(s))
        for r in range(plan.B):
            i = current[r]
            if i is not None and len(got[i]) < counts[i]:
                got[i].append((x[r], z[r], y[r]))
            else:       # nothing left for this row: no input, no target
                assert not x[r].any() and not z[r].any() and (y[r] == -1).all()
    assert sorted(started) == [i for i, c in enumerate(counts) if c]
    for i, t in enumerate(texts):
        ref = list(windows.stateful_windows(t, contexts[i], length, c_i))
        assert len(got[i]) == len(ref) == counts[i]
        for (x, z, y), (rx, rz, ry) in zip(got[i], ref):
            assert x.tolist() == rx.tolist() and y.tolist() == ry.tolist() and z.tolist() == rz.tolist()
    assert ratebatch.plan([np.zeros(0, np.int32), np.zeros(1, np.int32)], [[0], [0]], length, B) is None


def test_want_probs_false_gives_the_same_bits():
    r = make_rater(OracleLM, True, False)
    texts, contexts = contract_texts(r.length)
    _, bits = r.rate_batch(texts, contexts, streams=4)
    none, bits_only = r.rate_batch(texts, contexts, streams=4, want_probs=False)
    assert none is None
    assert bits_only.tolist() == bits.tolist()


def test_stateless_rater_gives_the_loop():
    r = make_rater(OracleLM, False, False)
    texts, contexts = contract_texts(r.length)
    ref_probs, ref_bits = loop(make_rater(OracleLM, False, False), texts, contexts)
    probs, bits = r.rate_batch(texts, contexts, streams=8)
    for a, b in zip(probs, ref_probs):
        assert a.dtype == np.float32 and len(a) == len(b)
        assert np.abs(a.astype(np.float64) - b).max(initial=0) < 1e-9
    assert np.all(np.abs(bits - ref_bits) <= 1e-9 * np.abs(ref_bits))


def test_incremental_rater_asserts():
    r = make_rater(OracleLM, False, True)
    with pytest.raises(AssertionError):
        r.rate_batch(["abc"])
    with pytest.raises(AssertionError):
        Rater(engine_factory=OracleLM).rate_batch(["abc"])      # not configured / loaded


def test_rate_after_rate_batch_starts_from_a_reset_state():
    r = make_rater(OracleLM, True, False)
    texts, contexts = contract_texts(r.length)
    r.rate(texts[6], contexts[6])            # (a carried state the batch call must not continue either)
    r.rate_batch(texts, contexts, streams=3)
    fresh = make_rater(OracleLM, True, False)
    fresh.model.reset_states(1)
    for t, c in zip(texts[5:8], contexts[5:8]):      # consecutive calls carry their state, as ever
        assert np.abs(np.array(r.rate(t, c), dtype=np.float64) - np.array(fresh.rate(t, c), dtype=np.float64)).max() < 1e-9
