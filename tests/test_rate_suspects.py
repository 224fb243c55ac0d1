"""`ratebulk.select_host`, `ratebulk.scatter_alts_host`, `Rater.suspects`, `Rater.rate_alternatives(precision=...)` and
`keraslm-rate suspects` on the CPU.

The oracle-backed engine double has neither `rate_window_alts_bulk` nor `rate_select`, so the Rater runs
`rate_alternatives`' ordinary path and the numpy statement of the selection -- argument checking, the per-text split and the
command are the product's.  The device kernels are held to the same statements in test_rate_suspects_gpu.py."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.oracle_engine import OracleLM
from tests.test_rate_bulk_gpu import random_text, small_rater

LENGTH = 16


def contract_texts():
    """the texts and contexts of test_rate_bulk_gpu.test_rate_batch_bf16_matches_the_oracle_rater"""
    rng = np.random.default_rng(12)
    texts = [random_text(rng, s) for s in (0, 1, 2, LENGTH, LENGTH + 1, 3 * LENGTH + 5, 2 * LENGTH + 1, 7, 40)]
    return texts, [[(171 if i % 2 else 185)] for i in range(len(texts))]


def settings_of(rated):
    """the three settings (max_prob, min_rank): everything, nothing, and the median predicted probability with min_rank 1 --
    which, by the arrays themselves, selects at least one predicted position and not all of them"""
    probs = np.concatenate([r.probs[1:] for r in rated])
    rank = np.concatenate([r.rank[1:] for r in rated])
    median = float(np.median(probs))
    hit = (rank >= 1) & (probs <= np.float32(median))
    assert 0 < hit.sum() < len(probs)
    return [(1.0, 0), (-1.0, 0), (median, 1)]


def same_as_filter(found, rated, max_prob, min_rank, exact=True):
    """found[i] holds exactly the rows of rated[i] with rank >= min_rank and probs <= f32(max_prob), ascending"""
    assert len(found) == len(rated)
    total = 0
    for one, ref in zip(found, rated):
        keep = np.nonzero((ref.rank >= min_rank) & (ref.probs <= np.float32(max_prob)))[0]
        assert isinstance(one, ratebatch.Suspects) and len(one) == len(keep)
        assert one.positions.dtype == np.int64 and np.array_equal(one.positions, keep)
        assert one.probs.dtype == np.float32 and one.rank.dtype == np.int32
        assert one.alt_ids.dtype == np.int32 and one.alt_probs.dtype == np.float32
        assert one.alt_ids.shape == one.alt_probs.shape == (len(keep), ref.alt_ids.shape[1])
        assert np.array_equal(one.probs.view(np.uint32), ref.probs[keep].view(np.uint32))
        assert np.array_equal(one.rank, ref.rank[keep]) and np.array_equal(one.alt_ids, ref.alt_ids[keep])
        assert np.array_equal(one.alt_probs.view(np.uint32), ref.alt_probs[keep].view(np.uint32))
        total += len(keep)
    return total


# ---------------------------------------------------------------------------------------------- the numpy statements
def test_select_host_rule():
    nan = np.float32("nan")
    probs = np.array([1.0, 0.25, 0.5, nan, 0.5000001, 0.1, 0.5, 0.0], dtype=np.float32)
    rank = np.array([-1, 3, 0, 2, 1, -1, 2, 7], dtype=np.int32)
    alt_id = np.arange(16, dtype=np.int32).reshape(8, 2)
    alt_p = np.arange(16, dtype=np.float32).reshape(8, 2) / 16
    # a tie at the threshold is selected; NaN is not; rank -1 is not, however small its probability
    pos, p, r, ai, ap = ratebulk.select_host(probs, rank, alt_id, alt_p, 0.5, 1)
    assert pos.dtype == np.int64 and pos.tolist() == [1, 6, 7]
    assert p.tolist() == [0.25, 0.5, 0.0] and r.tolist() == [3, 2, 7]
    assert ai.tolist() == [[2, 3], [12, 13], [14, 15]] and np.array_equal(ap, alt_p[[1, 6, 7]])
    assert p.dtype == np.float32 and r.dtype == np.int32 and ai.dtype == np.int32 and ap.dtype == np.float32
    # the comparison is made in f32: a threshold that rounds to 0.5 selects 0.5
    assert ratebulk.select_host(probs, rank, alt_id, alt_p, 0.5 - 1e-12, 1)[0].tolist() == [1, 6, 7]
    assert ratebulk.select_host(probs, rank, alt_id, alt_p, np.nextafter(np.float32(0.5), np.float32(0)), 1)[0].tolist() == [1, 7]
    # min_rank 0 with max_prob = inf: every predicted position but the NaN
    assert ratebulk.select_host(probs, rank, alt_id, alt_p, np.inf, 0)[0].tolist() == [1, 2, 4, 6, 7]
    assert ratebulk.select_host(probs, rank, alt_id, alt_p, -1.0, 0)[0].tolist() == []
    # empty input
    out = ratebulk.select_host(probs[:0], rank[:0], alt_id[:0], alt_p[:0], 1.0, 0)
    assert [a.shape for a in out] == [(0,), (0,), (0,), (0, 2), (0, 2)] and out[0].dtype == np.int64
    for bad in ((0.5, -1), (float("nan"), 0)):
        with pytest.raises(ValueError):
            ratebulk.select_host(probs, rank, alt_id, alt_p, *bad)


def test_scatter_alts_host_is_scatter_host_per_plane():
    rng = np.random.default_rng(1)
    B, T, K, n_ctx = 6, 5, 3, 1
    tprob = rng.random((B, T)).astype(np.float32)
    rank = rng.integers(0, 9, (B, T)).astype(np.int32)
    alt_id = rng.integers(0, 9, (B, T, K)).astype(np.int32)
    alt_p = rng.random((B, T, K)).astype(np.float32)
    rows = np.zeros((B, 4 + n_ctx), dtype=np.int64)
    rows[:, 0] = np.arange(B) * (T + 2) + 1
    rows[:, 1] = [0, 1, T, T + 3, -2, T]
    n = int(rows[-1, 0]) + 1 + T // 2               # the last row ends beyond the outputs
    out = (np.full(n, -5.0, dtype=np.float32), np.full(n, -5, dtype=np.int32), np.full((n, K), -5, dtype=np.int32),
           np.full((n, K), -5.0, dtype=np.float32))
    got = ratebulk.scatter_alts_host(tprob, rank, alt_id, alt_p, rows, *out)
    assert all(a is b for a, b in zip(got, out))
    want = ratebulk.scatter_host(tprob, rows, np.full(n, -5.0, dtype=np.float32))
    assert np.array_equal(out[0], want)
    written = want != -5.0
    assert written.any() and not written.all()
    for a in out[1:]:
        assert (a[~written] == -5).all() and (a[written] != -5).all()
    b, t = 2, 3
    g = int(rows[b, 0]) + 1 + t
    assert out[1][g] == rank[b, t] and np.array_equal(out[2][g], alt_id[b, t]) and np.array_equal(out[3][g], alt_p[b, t])


def test_documented_constants_agree():
    """the selection's block sizes: header and binding"""
    import os
    import re
    from ocrd_keraslm_amd.lib import hipabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "keraslm_hip.h")).read()
    for name in ("KL_RATE_SELECT_BLOCK", "KL_RATE_SELECT_SCAN_THREADS"):
        assert [int(v) for v in re.findall(r"^#define %s (\d+)$" % name, text, flags=re.M)] == [getattr(hipabi, name)]


# ---------------------------------------------------------------------------------------------- the Rater on the double
def test_suspects_is_the_filter_of_rate_alternatives():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    rated, bits = r.rate_alternatives(texts, contexts, k=3, streams=4)
    counts = []
    for precision in ("bf16", "split"):
        for max_prob, min_rank in settings_of(rated):
            found, bits2 = r.suspects(texts, contexts, k=3, streams=4, max_prob=max_prob, min_rank=min_rank, precision=precision)
            assert np.array_equal(bits2, bits)
            counts.append(same_as_filter(found, rated, max_prob, min_rank))
            assert len(found[0]) == len(found[1]) == 0          # texts without a prediction yield nothing
    predicted = sum(max(len(t) - 1, 0) for t in texts)
    assert counts[0] == predicted and counts[1] == 0 and 0 < counts[2] < predicted and counts[3:] == counts[:3]
    # ... as characters
    found, _ = r.suspects(texts, contexts, k=3, streams=4, max_prob=1.0, min_rank=0)
    assert found[5].chars(r.mapping) == rated[5].chars(r.mapping)[1:]
    # nothing but texts without a prediction
    found, bits = r.suspects(["", "a"])
    assert [len(f) for f in found] == [0, 0] and found[1].alt_ids.shape == (0, 3) and bits.tolist() == [0.0, 0.0]


def test_rate_alternatives_bf16_on_the_double_is_split():
    texts, contexts = contract_texts()
    r = small_rater(OracleLM, length=LENGTH)
    a, bits_a = r.rate_alternatives(texts, contexts, k=4, streams=4)
    b, bits_b = r.rate_alternatives(texts, contexts, k=4, streams=4, precision="bf16")
    c, bits_c = r.rate_alternatives(texts, contexts, k=4, streams=4, precision="split")
    assert np.array_equal(bits_a, bits_b) and np.array_equal(bits_a, bits_c)
    for x, y, z in zip(a, b, c):
        for name in ("probs", "rank", "alt_ids", "alt_probs"):
            assert np.array_equal(getattr(x, name), getattr(y, name)) and np.array_equal(getattr(x, name), getattr(z, name))


def test_argument_errors():
    r = small_rater(OracleLM, length=LENGTH)
    for bad in (dict(min_rank=-1), dict(max_prob=float("nan")), dict(precision="f32")):
        with pytest.raises(ValueError):
            r.suspects(["abc"], **bad)
    for k in (0, 9):
        with pytest.raises(AssertionError):
            r.suspects(["abc"], k=k)
    with pytest.raises(ValueError):
        r.rate_alternatives(["abc"], precision="f32")
    r.stateful = False
    for precision in ("bf16", "split"):
        with pytest.raises(ValueError):
            r.suspects(["abc"], precision=precision)
    with pytest.raises(ValueError):
        r.rate_alternatives(["abc"], precision="bf16")


# ---------------------------------------------------------------------------------------------- command line
def test_cli_suspects(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
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
    rated, _ = ref.rate_alternatives(texts, contexts, k=2, streams=2)
    median = float(np.median(np.concatenate([x.probs[1:] for x in rated])))
    res = CliRunner().invoke(run.cli, ["suspects", "-m", str(model), "-s", "2", "--precision", "split", "-k", "2", "--max-prob",
                                       repr(median), "--min-rank", "1"] + files)
    assert res.exit_code == 0, res.output
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    found, bits = ref.suspects(texts, contexts, k=2, streams=2, max_prob=median, min_rank=1, precision="split")
    assert sum(len(f) for f in found) > 0
    for line, text, one, total in zip(lines, texts, found, bits):
        assert line["chars"] == len(text) and line["bits_per_char"] == float(total) / max(len(text) - 1, 1)
        assert len(line["suspects"]) == len(one)
        for (pos, char, prob, rank, alts), j, p, q, ids, ps in zip(line["suspects"], one.positions, one.probs, one.rank,
                                                                   one.alt_ids, one.alt_probs):
            assert pos == int(j) and char == text[pos] and prob == float(p) and rank == int(q)
            assert alts == [[ref.mapping[1].get(int(v), ""), float(w)] for v, w in zip(ids, ps)]
    assert len(lines[1]["suspects"]) == 0
    for bad in (["-k", "0"], ["-k", "9"], ["--min-rank", "-1"], ["--precision", "f32"]):
        assert CliRunner().invoke(run.cli, ["suspects", "-m", str(model)] + bad + files).exit_code != 0
