"""The scheduler of bulk rating (lib/ratebulk.py) and `Rater.rate_batch(precision="bf16")` on the CPU.

The plan describes every window call by the rows `kl_assemble_windows` reads; `windows_host` / `scatter_host` /
`text_bits_host` are the numpy statements of the three kernels around the window call (held to the kernels in
tests/test_rate_bulk_gpu.py).  Here: the windows a plan yields are `windows.stateful_windows` of every text, cut at the
call's T; every prediction is covered exactly once; rows are reset exactly where a text starts; and the way back restores
every text's slice.  The oracle-backed engine double has no `rate_window_bulk`: the switch must fall through to the
ordinary plan there and give identical results."""
import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests import test_rate_batch as tb
from tests.oracle_engine import OracleLM


def corpus_of(rng, sizes, voc=50):
    """ids 1 .. voc - 1 end to end (0 would hide a wrong read behind the padding value)"""
    return [rng.integers(1, voc, s).astype(np.int32) for s in sizes]


@pytest.mark.parametrize("streams", [1, 3, 64])
@pytest.mark.parametrize("length", [8, 32])
def test_plan_covers_every_text(length, streams):
    rng = np.random.default_rng(length * 100 + streams)
    sizes = [0, 1, 2, length, length + 1, 2 * length + 1] + [int(s) for s in rng.integers(0, 5 * length, 23)]
    ids = corpus_of(rng, sizes)
    contexts = [[int(rng.integers(0, 200)), int(rng.integers(0, 200))] for _ in sizes]
    corpus = np.concatenate(ids)
    plan = ratebulk.plan(sizes, contexts, length, streams)
    assert plan.offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist() and plan.total == len(corpus)
    assert plan.n_ctx == 2
    # the reference windows of every text: identity mapping over code points = ids
    c_i = dict((chr(k), k) for k in range(1, 50))
    ref = [list(windows.stateful_windows("".join(chr(int(k)) for k in a), c, length, c_i)) for a, c in zip(ids, contexts)]
    counts = [windows.count_windows(s, length) for s in sizes]
    assert plan.count.tolist() == counts
    got = dict((i, []) for i in range(len(sizes)))
    covered = np.zeros(len(corpus), dtype=np.int64)
    flat = np.full(len(corpus), -7.0, dtype=np.float32)
    marks = (np.arange(len(corpus)) + 0.5).astype(np.float32)      # "the probability of the character at g" = g + 0.5
    current = {}
    for s, call in enumerate(plan.calls):
        assert min(3, length) <= call.T <= length
        assert call.rows.dtype == np.int64 and call.rows.shape == (call.B, 4 + 2) and 1 <= call.B <= streams
        assert call.reset.dtype == np.bool_ and call.reset.shape == (call.B,)
        assert (call.rows[:, 2:4] == -1).all()
        x, z, y = ratebulk.windows_host(corpus, call.rows, call.T)
        assert x.dtype == y.dtype == z.dtype == np.int32 and z.shape == (call.B, call.T, 2)
        starting = [int(i) for i in range(len(sizes)) if counts[i] and plan.first[i] == s]
        assert sorted(np.nonzero(call.reset)[0].tolist()) == sorted(int(plan.row[i]) for i in starting)
        for i in starting:
            r = int(plan.row[i])
            prev = current.get(r)
            # (a row takes a new text only when its text has ended; a change of B between calls starts every row anew)
            assert prev is None or len(got[prev]) == counts[prev], "row taken before its text ended"
            current[r] = i
        if s and call.B != plan.calls[s - 1].B:
            assert call.reset.all()
        tprob = np.zeros((call.B, call.T), dtype=np.float32)
        for r in range(call.B):
            i = current.get(r)
            if i is not None and len(got[i]) < counts[i] and plan.first[i] + len(got[i]) == s:
                got[i].append((x[r], z[r], y[r], call.T))
                start, vlen = int(call.rows[r, 0]), int(call.rows[r, 1])
                done = sum(t for _x, _z, _y, t in got[i][:-1])
                assert start == plan.offsets[i] + done and vlen == min(call.T, sizes[i] - 1 - done) and vlen > 0
                covered[start + 1:start + 1 + vlen] += 1
                tprob[r, :vlen] = marks[start + 1:start + 1 + vlen]
                tprob[r, vlen:] = -1.0      # (must not be scattered)
            else:       # nothing for this row: no input, no target
                assert call.rows[r, 1] == 0 and not call.reset[r]
                assert not x[r].any() and not z[r].any() and (y[r] == -1).all()
                tprob[r] = -1.0
        ratebulk.scatter_host(tprob, call.rows, flat)
    for i, size in enumerate(sizes):
        assert len(got[i]) == len(ref[i]) == counts[i], i
        for (x, z, y, T), (rx, rz, ry) in zip(got[i], ref[i]):
            assert x.tolist() == rx[:T].tolist() and y.tolist() == ry[:T].tolist() and z.tolist() == rz[:T].tolist()
            assert not rx[T:].any() and (ry[T:] == -1).all()      # (the cut takes nothing away)
        a = int(plan.offsets[i])
        # every prediction once, the first character never; scatter restores the text's slice
        assert covered[a:a + size].tolist() == ([0] + [1] * (size - 1) if size else [])
        assert flat[a:a + size].tolist() == ([-7.0] + marks[a + 1:a + size].tolist() if size else [])
    # texts that fit one window share calls no longer than they need
    short_T = [c.T for c in plan.calls if c.reset.all() and (c.rows[:, 1] <= c.T).all()]
    assert all(t == length or t % 32 == 0 or t == 3 for t in short_T)


def test_short_lines_run_short_windows():
    """20 000-line corpora of 30 .. 90 characters must not run `length`-step windows: T = the group's longest, rounded to 32"""
    rng = np.random.default_rng(1)
    sizes = [int(s) for s in rng.integers(30, 91, 500)]
    plan = ratebulk.plan(sizes, [[0]] * len(sizes), 256, 128)
    assert plan.n_calls == 4 and [c.B for c in plan.calls] == [128, 128, 128, 116]
    assert [c.T for c in plan.calls] == [64, 64, 96, 96] or [c.T for c in plan.calls] == [64, 64, 64, 96]
    assert len(set((c.B, c.T) for c in plan.calls)) <= 4
    empty = ratebulk.plan([0, 1], [[0], [0]], 8, 4)
    assert empty.calls == [] and empty.total == 1


def test_text_bits_host_is_bits_of():
    rng = np.random.default_rng(2)
    sizes = [0, 1, 2, 65, 300]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    probs = rng.random(int(offsets[-1])).astype(np.float32)
    probs[offsets[3] + 5] = 0.0       # (the clamp)
    bits = ratebulk.text_bits_host(probs, offsets)
    assert bits.dtype == np.float64 and bits[0] == bits[1] == 0.0
    for i in range(len(sizes)):
        want = ratebatch.bits_of(probs[offsets[i]:offsets[i + 1]])
        assert abs(bits[i] - want) <= 1e-12 * max(1.0, abs(want))
    assert bits[3] > 300       # -log2(1e-99) = 328.9


@pytest.mark.parametrize("streams", [1, 3, 64])
def test_bf16_switch_on_an_engine_without_bulk_rating_is_the_ordinary_plan(streams):
    r = tb.make_rater(OracleLM, True, False)
    assert not hasattr(r.model, "rate_window_bulk")
    texts, contexts = tb.contract_texts(r.length)
    probs, bits = r.rate_batch(texts, contexts, streams=streams, precision="split")
    probs16, bits16 = r.rate_batch(texts, contexts, streams=streams, precision="bf16")
    assert bits16.tolist() == bits.tolist()
    for a, b in zip(probs, probs16):
        assert a.dtype == b.dtype == np.float32 and a.tolist() == b.tolist()
    none, bits_only = r.rate_batch(texts, contexts, streams=streams, want_probs=False, precision="bf16")
    assert none is None and bits_only.tolist() == bits.tolist()


def test_bf16_switch_needs_a_stateful_rater_and_a_known_precision():
    r = tb.make_rater(OracleLM, False, False)
    with pytest.raises(ValueError):
        r.rate_batch(["abc", "de"], precision="bf16")
    probs, _ = r.rate_batch(["abc", "de"])      # (the default is untouched)
    assert len(probs) == 2
    with pytest.raises(ValueError):
        tb.make_rater(OracleLM, True, False).rate_batch(["abc"], precision="fp8")
