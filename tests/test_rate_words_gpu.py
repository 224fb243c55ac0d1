"""Word-level ratings on the GPU (run with -m gpu on an MI355X): kl_word_bounds, kl_rate_segments, kl_segment_select, the engine
wrappers, `Rater.suspect_words` and `Rater.rate_segments`.

The three kernels are held to their numpy statements in lib/ratebulk.py: the compactions bit for bit, the f64 sums of
kl_rate_segments within 1e-12 * max(1, |value|) + len * 2^-50 (the project's bounds for such sums: test_rate_bulk_gpu.py,
kl_context_mix).  The shapes are the smallest at which each kernel can go wrong: a wave, a round of 256 threads and a block of
KL_RATE_SELECT_BLOCK items on either side of a word, one input beyond a round of the offsets workgroup."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.test_rate_bulk_gpu import device, lib_and_stream, small_rater
from tests.test_rate_suspects import contract_texts
from tests.test_rate_suspects_gpu import BLOCK, SCAN_THREADS
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words import LENGTH, quantile_of, same_words, special_case_inputs, statements_over

pytestmark = pytest.mark.gpu

KL_ERR_WORKSPACE, KL_ERR_ARG = 4, 5
FILL = 0xA5      # every byte of an output before the call
GUARD = 64       # elements behind each output


def marked(n, dtype):
    """n + GUARD elements of dtype on the device, every byte FILL"""
    torch, dev = device()
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full(((n + GUARD) * size,), FILL, dtype=torch.uint8, device=dev).view(dtype)


def raw(t, first=0):
    """the bytes of a device tensor from element `first` on"""
    return t.cpu().numpy().view(np.uint8).reshape(-1)[first * t.element_size():]


def same_bytes(t, ref, count):
    """the first `count` elements of the device tensor are ref[:count] bit for bit, everything behind keeps FILL"""
    ref = np.ascontiguousarray(ref[:count])
    got = raw(t)
    return np.array_equal(got[:ref.nbytes], ref.view(np.uint8).reshape(-1)) and (got[ref.nbytes:] == FILL).all()


def up(a):
    torch, dev = device()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def shifted(p, by):
    return C.c_void_p(p.value + by)


# ---------------------------------------------------------------------------------------------- kl_word_bounds
class Bounds(object):
    """kl_word_bounds on device copies of host arrays; outputs of `room` entries plus a guard band"""

    def __init__(self, corpus, offsets, delim):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.n, self.n_texts, self.V = len(corpus), len(offsets) - 1, len(delim)
        self.src = [up(np.asarray(corpus, dtype=np.int32)) if len(corpus) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev),
                    up(np.asarray(offsets, dtype=np.int64)), up(np.asarray(delim, dtype=np.uint8))]
        self.n_ws = self.lib.kl_word_bounds_workspace_bytes(self.n, self.n_texts)
        self.ws = self.torch.empty(max(self.n_ws, 8), dtype=self.torch.uint8, device=self.dev)

    def run(self, capacity, room=None, null_out=False, ws_bytes=None, shift=None, **override):
        torch = self.torch
        room = capacity if room is None else room
        self.count = torch.full((1,), -77, dtype=torch.int64, device=self.dev)
        self.out = [marked(room, torch.int64), marked(room, torch.int64)]
        a = dict(corpus=ptr(self.src[0]), offsets=ptr(self.src[1]), delim=ptr(self.src[2]), n=self.n, n_texts=self.n_texts,
                 V=self.V, seg_start=ptr(self.out[0]), seg_end=ptr(self.out[1]), count=ptr(self.count), ws=ptr(self.ws))
        if null_out:
            a.update(seg_start=None, seg_end=None)
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_word_bounds(a["corpus"], a["n"], a["offsets"], a["n_texts"], a["delim"], a["V"], capacity,
                                       a["seg_start"], a["seg_end"], a["count"], a["ws"],
                                       self.n_ws if ws_bytes is None else ws_bytes, self.stream)
        torch.cuda.synchronize()
        return code

    def holds(self, want, capacity):
        """count is the total; the first min(count, capacity) words are want's; everything behind keeps FILL"""
        m = min(len(want[0]), capacity)
        return (int(self.count.item()) == len(want[0]) and same_bytes(self.out[0], want[0], m)
                and same_bytes(self.out[1], want[1], m))

    def untouched(self):
        return int(self.count.item()) == -77 and all((raw(t) == FILL).all() for t in self.out)


DELIM = np.array([0, 1, 0, 0, 1, 0, 0, 0], dtype=np.uint8)      # ids 1 and 4 separate words


def bounds_corpus(n, seed):
    """n ids with a delimiter at about every fourth place, ids outside the table, and runs of characters across a wave, a round
    of 256 threads and a block; the last word ends at n - 1; texts with empty ones among them, a boundary inside a run"""
    rng = np.random.default_rng(seed)
    corpus = rng.integers(-1, len(DELIM) + 2, n).astype(np.int32)
    corpus[rng.random(n) < 0.15] = 1
    for at in (64, 256, BLOCK, 2 * BLOCK, 3 * BLOCK):
        if at + 6 < n:
            corpus[at - 5:at + 6] = 2
            corpus[at - 6] = corpus[at + 6] = 4
    if n > 3 * BLOCK:
        corpus[3 * BLOCK - 2] = 600       # (inside the last run: an id outside the table is a character)
    corpus[n - 4:] = 3
    corpus[n - 5] = 1
    cuts = np.sort(rng.integers(0, n, 40))
    offsets = np.concatenate([[0], cuts, cuts[5:8], [min(66, n), min(2 * BLOCK - 2, n), n, n]])      # (repeated values: empty texts)
    return corpus, np.sort(offsets).astype(np.int64)


def test_word_bounds_is_word_bounds_host():
    n = 3 * BLOCK + 17
    corpus, offsets = bounds_corpus(n, 1)
    want = ratebulk.word_bounds_host(corpus, offsets, DELIM)
    m = len(want[0])
    inside = lambda at: ((want[0] < at) & (at < want[1])).any()
    assert inside(64) and inside(256) and inside(BLOCK) and inside(3 * BLOCK) and not inside(66) and not inside(2 * BLOCK - 2)
    assert (want[0] == 66).any() and (want[1] == 66).any()          # the text boundary inside a run of characters: two words
    assert want[1][-1] == n and m > 100 and (np.diff(offsets) == 0).any()
    assert ((corpus < 0) | (corpus >= len(DELIM))).sum() > 100
    b = Bounds(corpus, offsets, DELIM)
    assert b.n_ws >= 8 * -(-n // BLOCK)
    assert b.run(0, null_out=True) == 0 and int(b.count.item()) == m      # the counting call: no outputs at all
    runs = []
    for capacity in (m, m, m // 2, 1):
        assert b.run(capacity, room=m) == 0
        assert b.holds(want, capacity), capacity      # the full count; entries from `capacity` on keep their marker
        runs.append([raw(t).copy() for t in b.out])
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], runs[1]))      # two runs are identical
    # texts that cover a part of the corpus only, and end beyond it: nothing outside [offsets[0], n) is a character
    part = np.sort(np.concatenate([[7, n + 10], offsets[5:30]])).astype(np.int64)
    want = ratebulk.word_bounds_host(corpus, part, DELIM)
    assert want[0][0] >= 7 and want[1][-1] == n
    b = Bounds(corpus, part, DELIM)
    assert b.run(len(want[0])) == 0 and b.holds(want, len(want[0]))


def test_word_bounds_none_one_and_a_second_scan_round():
    # nothing but delimiters: count 0, nothing written
    n = BLOCK + 3
    b = Bounds(np.full(n, 4, dtype=np.int32), [0, 10, n], DELIM)
    assert b.run(4) == 0 and int(b.count.item()) == 0 and all((raw(t) == FILL).all() for t in b.out)
    # one text without a delimiter: one word [offsets[0], n)
    b = Bounds(np.full(n, 2, dtype=np.int32), [3, n], DELIM)
    assert b.run(4) == 0 and b.holds((np.array([3], dtype=np.int64), np.array([n], dtype=np.int64)), 4)
    # more blocks than the offsets workgroup takes per round
    n = (SCAN_THREADS + 1) * BLOCK + 5
    corpus, offsets = bounds_corpus(n, 2)
    want = ratebulk.word_bounds_host(corpus, offsets, DELIM)
    m = len(want[0])
    assert (want[0] > SCAN_THREADS * BLOCK).sum() > 10
    b = Bounds(corpus, offsets, DELIM)
    assert b.run(m) == 0 and b.holds(want, m)
    assert b.run(m - 7, room=m) == 0 and b.holds(want, m - 7)
    # an empty corpus is valid: no words
    b = Bounds(np.zeros(0, dtype=np.int32), [0, 0], DELIM)
    assert b.run(4) == 0 and int(b.count.item()) == 0 and all((raw(t) == FILL).all() for t in b.out)


def test_word_bounds_errors_return_before_any_launch():
    n = 300
    corpus, offsets = bounds_corpus(n, 3)
    b = Bounds(corpus, offsets, DELIM)
    size = b.lib.kl_word_bounds_workspace_bytes
    assert size(2 ** 40 + 1, 3) == 0 and size(n, 0) == 0 and b.n_ws > 0
    cases = [dict(corpus=None), dict(offsets=None), dict(delim=None), dict(count=None), dict(ws=None), dict(seg_start=None),
             dict(seg_end=None), dict(n_texts=0), dict(V=0), dict(n=2 ** 40 + 1)]
    cases += [dict(shift={name: by}) for name, by in (("corpus", 2), ("offsets", 4), ("seg_start", 4), ("seg_end", 4), ("count", 4),
                                                      ("ws", 4))]
    for case in cases:
        assert b.run(n, **case) == KL_ERR_ARG, case
        assert b.untouched(), case
    assert b.run(n, ws_bytes=b.n_ws - 1) == KL_ERR_WORKSPACE and b.untouched()
    want = ratebulk.word_bounds_host(corpus, offsets, DELIM)
    assert b.run(n) == 0 and b.holds(want, n)


# ---------------------------------------------------------------------------------------------- kl_rate_segments
class Rate(object):
    """kl_rate_segments on device copies of host arrays; six outputs of S entries plus a guard band"""
    NAMES = ("probs", "rank", "offsets", "seg_start", "seg_end", "seg_n", "seg_bits", "seg_psum", "seg_min", "seg_worst", "seg_bad")

    def __init__(self, probs, rank, offsets, seg_start, seg_end):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.n, self.n_texts, self.S = len(probs), len(offsets) - 1, len(seg_start)
        self.src = [up(probs), up(rank) if rank is not None else None, up(offsets), up(seg_start), up(seg_end)]

    def run(self, max_prob, min_rank, shift=None, **override):
        torch = self.torch
        kinds = (torch.int32, torch.float64, torch.float64, torch.float32, torch.int64, torch.int32)
        self.out = [marked(self.S, k) for k in kinds]
        a = dict(zip(self.NAMES, [ptr(t) for t in self.src] + [ptr(t) for t in self.out]), n=self.n, n_texts=self.n_texts, S=self.S)
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_rate_segments(a["probs"], a["rank"], a["n"], a["offsets"], a["n_texts"], a["seg_start"], a["seg_end"],
                                         a["S"], C.c_float(max_prob), min_rank, a["seg_n"], a["seg_bits"], a["seg_psum"],
                                         a["seg_min"], a["seg_worst"], a["seg_bad"], self.stream)
        torch.cuda.synchronize()
        return code

    def results(self):
        return [t.cpu().numpy()[:self.S] for t in self.out]

    def guards_hold(self):
        return all((raw(t, self.S) == FILL).all() for t in self.out)

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out)


def segments_inputs():
    """the special cases of test_rate_words.special_case_inputs in front; then texts of 70, 1100, 1 and 5200 characters with
    segments of 0, 1, 63, 64, 65, 1000 and 5000 positions, overlapping ones, one at a text's first character, one across a
    text's end; ten positions behind the last text (a < n in no text); all in descending order of their starts"""
    probs, rank, offsets, seg_start, seg_end = special_case_inputs()
    rng = np.random.default_rng(7)
    sizes = [70, 1100, 1, 5200]
    more = int(np.sum(sizes)) + 10
    new_p = (rng.random(more) ** 4).astype(np.float32)
    new_p[rng.random(more) < 0.02] = np.float32("nan")
    new_p[rng.random(more) < 0.02] = 0.0
    new_r = rng.integers(-1, 6, more).astype(np.int32)
    base = len(probs)
    probs, rank = np.concatenate([probs, new_p]), np.concatenate([rank, new_r])
    offsets = np.concatenate([offsets, base + np.cumsum(sizes)]).astype(np.int64)
    t70, t1100, t1, t5200 = (int(offsets[-5 + i]) for i in range(4))
    segs = [(t70 + 3, t70 + 3), (t70 + 3, t70 + 4), (t70 + 1, t70 + 64), (t70 + 1, t70 + 65), (t70 + 1, t70 + 66),
            (t70, t70 + 64), (t70 + 40, t70 + 400),                       # at the first character; across the text's end
            (t1100 + 50, t1100 + 1050), (t1100 + 60, t1100 + 125), (t1, t1 + 1),
            (t5200 + 100, t5200 + 5100), (t5200 + 1, t5200 + 5200), (t5200 + 4000, t5200 + 4064),
            (int(offsets[-1]) + 2, int(offsets[-1]) + 6)]                 # behind the last text: a < n, in no text
    seg_start = np.concatenate([seg_start, [a for a, _ in segs]]).astype(np.int64)[::-1].copy()
    seg_end = np.concatenate([seg_end, [b for _, b in segs]]).astype(np.int64)[::-1].copy()
    tie = t5200 + 200      # tied minima in three lanes of a group, the first position in the highest of them: it wins
    probs[tie + 30] = probs[tie + 11] = probs[tie + 12] = np.float32(-1.0)
    return probs, rank, offsets, seg_start, seg_end


def test_rate_segments_is_segments_host():
    probs, rank, offsets, seg_start, seg_end = segments_inputs()
    max_prob, min_rank = 0.05, 1
    assert (np.diff(seg_start) <= 0).sum() > len(seg_start) // 2 and int(offsets[-1]) < len(probs)
    for with_rank in (rank, None):
        want = ratebulk.segments_host(probs, with_rank, offsets, seg_start, seg_end, max_prob, min_rank)
        assert set([0, 1, 63, 64, 65, 1000, 5000]) <= set(want[0].tolist())
        assert (want[5] > 0).any() == (with_rank is not None) and np.isnan(want[2]).any() and (want[1] > 328.0).any()
        assert (want[4] == int(offsets[-2]) + 211).sum() == 2      # the tied minima: the first position
        r = Rate(probs, with_rank, offsets, seg_start, seg_end)
        runs = []
        for _ in range(2):
            assert r.run(max_prob, min_rank) == 0
            assert r.guards_hold()
            runs.append(r.results())
        for x, y in zip(*runs):      # two calls agree bit for bit
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        n, bits, psum, least, worst, bad = runs[0]
        assert np.array_equal(n, want[0]) and np.array_equal(worst, want[4]) and np.array_equal(bad, want[5])
        assert np.array_equal(least.view(np.uint32), want[3].view(np.uint32))
        bound = lambda ref, lens: 1e-12 * np.maximum(1.0, np.abs(ref)) + lens * 2.0 ** -50
        worst_bits = np.abs(bits - want[1]) / bound(want[1], want[0])
        fine = ~np.isnan(want[2])
        worst_psum = np.abs(psum[fine] - want[2][fine]) / bound(want[2][fine], want[0][fine])
        print("largest error over its bound: bits %.3g, psum %.3g" % (worst_bits.max(), worst_psum.max()))
        assert (worst_bits <= 1.0).all() and (worst_psum <= 1.0).all() and np.isnan(psum[~fine]).all()


def test_rate_segments_errors_return_before_any_launch():
    probs, rank, offsets, seg_start, seg_end = special_case_inputs()
    r = Rate(probs, rank, offsets, seg_start, seg_end)
    cases = [{name: None} for name in Rate.NAMES if name != "rank"]
    cases += [dict(S=0), dict(S=2 ** 32 + 1), dict(n_texts=0), dict(n=2 ** 40 + 1)]
    cases += [dict(shift={name: 2}) for name in ("probs", "rank", "seg_n", "seg_min", "seg_bad")]
    cases += [dict(shift={name: 4}) for name in ("offsets", "seg_start", "seg_end", "seg_bits", "seg_psum", "seg_worst")]
    for case in cases:
        assert r.run(0.25, 1, **case) == KL_ERR_ARG, case
        assert r.untouched(), case
    assert r.run(0.25, -1) == KL_ERR_ARG and r.untouched()
    assert r.run(float("nan"), 0) == KL_ERR_ARG and r.untouched()
    assert r.run(0.25, 1) == 0 and np.array_equal(r.results()[0], ratebulk.segments_host(probs, rank, offsets, seg_start, seg_end)[0])


# ---------------------------------------------------------------------------------------------- kl_segment_select
class Pick(object):
    """kl_segment_select on device copies of host records; nine outputs of `room` entries plus a guard band"""
    SRC = ("seg_start", "seg_end", "seg_n", "seg_bits", "seg_psum", "seg_min", "seg_worst", "seg_bad")
    OUT = ("sel_index", "sel_start", "sel_end", "sel_n", "sel_bits", "sel_psum", "sel_min", "sel_worst", "sel_bad")

    def __init__(self, records):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.S = len(records[0])
        self.src = [up(a) for a in records]
        self.n_ws = self.lib.kl_segment_select_workspace_bytes(self.S)
        self.ws = self.torch.empty(max(self.n_ws, 8), dtype=self.torch.uint8, device=self.dev)

    def run(self, min_n, min_bad, min_bpc, capacity, room=None, null_out=False, ws_bytes=None, shift=None, **override):
        torch = self.torch
        room = capacity if room is None else room
        self.count = torch.full((1,), -77, dtype=torch.int64, device=self.dev)
        self.out = [marked(room, torch.int64)] + [marked(room, t.dtype) for t in self.src]
        a = dict(zip(self.SRC + self.OUT, [ptr(t) for t in self.src] + [ptr(t) for t in self.out]), S=self.S,
                 count=ptr(self.count), ws=ptr(self.ws))
        if null_out:
            a.update(dict((name, None) for name in self.OUT))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_segment_select(*([a[name] for name in self.SRC] + [a["S"], min_n, min_bad, C.c_double(min_bpc), capacity]
                                            + [a[name] for name in self.OUT]
                                            + [a["count"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes, self.stream]))
        torch.cuda.synchronize()
        return code

    def holds(self, want, capacity):
        m = min(len(want[0]), capacity)
        return int(self.count.item()) == len(want[0]) and all(same_bytes(t, ref, m) for t, ref in zip(self.out, want))

    def untouched(self):
        return int(self.count.item()) == -77 and all((raw(t) == FILL).all() for t in self.out)


def random_records(S, seed, min_n, min_bad, min_bpc):
    """S records, about a third of them selected; equality planted on each of the three comparisons, NaN bits among them"""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, 2 ** 40, S).astype(np.int64)
    end = start + rng.integers(0, 50, S)
    n = rng.integers(0, 12, S).astype(np.int32)
    bits = rng.random(S) * 3.0 * n
    bits[rng.random(S) < 0.05] = np.nan
    psum = rng.random(S)
    least = rng.random(S).astype(np.float32)
    worst = rng.integers(-1, 2 ** 40, S).astype(np.int64)
    bad = rng.integers(0, 4, S).astype(np.int32)
    for s in (0, S // 2, S - 1):      # equality on all three: selected
        n[s], bad[s] = min_n, min_bad
        bits[s] = min_bpc * float(min_n)
    n[1], bad[1], bits[1] = min_n + 4, min_bad, min_bpc * float(min_n + 4)
    n[2], bad[2], bits[2] = min_n + 4, min_bad, np.nextafter(min_bpc * float(min_n + 4), 0.0)      # one ulp short: not selected
    return start, end, n, bits, psum, least, worst, bad


@pytest.mark.parametrize("S", [BLOCK + 1, SCAN_THREADS * BLOCK + 7])
def test_segment_select_is_segment_select_host(S):
    rule = dict(min_n=3, min_bad=1, min_bpc=1.5)
    records = random_records(S, S, **rule)
    want = ratebulk.segment_select_host(*records, **rule)
    m = len(want[0])
    assert 0 < m < S and set([0, 1, S // 2, S - 1]) <= set(want[0].tolist()) and 2 not in want[0]
    p = Pick(records)
    assert p.n_ws >= 8 * -(-S // BLOCK)
    args = (rule["min_n"], rule["min_bad"], rule["min_bpc"])
    assert p.run(*args, 0, null_out=True) == 0 and int(p.count.item()) == m      # the counting call
    runs = []
    for capacity in (m, m, m // 2):
        assert p.run(*args, capacity, room=m) == 0
        assert p.holds(want, capacity), capacity
        runs.append([raw(t).copy() for t in p.out])
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], runs[1]))
    # nothing selected: nothing written
    none = ratebulk.segment_select_host(*records, min_n=100, min_bad=0, min_bpc=0.0)
    assert len(none[0]) == 0 and p.run(100, 0, 0.0, 4) == 0 and p.holds(none, 4)


def test_segment_select_errors_return_before_any_launch():
    S = 300
    records = random_records(S, 5, 3, 1, 1.5)
    p = Pick(records)
    size = p.lib.kl_segment_select_workspace_bytes
    assert size(0) == 0 and size(2 ** 40 + 1) == 0 and p.n_ws > 0
    cases = [{name: None} for name in Pick.SRC + Pick.OUT + ("count", "ws")] + [dict(S=0), dict(S=2 ** 40 + 1)]
    cases += [dict(shift={name: 2}) for name in ("seg_n", "seg_min", "seg_bad", "sel_n", "sel_min", "sel_bad")]
    cases += [dict(shift={name: 4}) for name in ("seg_start", "seg_end", "seg_bits", "seg_psum", "seg_worst", "sel_index",
                                                 "sel_start", "sel_end", "sel_bits", "sel_psum", "sel_worst", "count", "ws")]
    for case in cases:
        assert p.run(3, 1, 1.5, S, **case) == KL_ERR_ARG, case
        assert p.untouched(), case
    for wrong in ((0, 1, 1.5), (3, -1, 1.5), (3, 1, -0.5), (3, 1, float("nan"))):
        assert p.run(*wrong, S) == KL_ERR_ARG and p.untouched(), wrong
    assert p.run(3, 1, 1.5, S, ws_bytes=p.n_ws - 1) == KL_ERR_WORKSPACE and p.untouched()
    assert p.run(3, 1, 1.5, S) == 0 and p.holds(ratebulk.segment_select_host(*records, min_n=3, min_bad=1, min_bpc=1.5), S)


# ---------------------------------------------------------------------------------------------- engine
def test_engine_wrappers_count_first():
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    n = 3 * BLOCK + 17
    corpus, offsets = bounds_corpus(n, 4)
    rng = np.random.default_rng(4)
    probs = (rng.random(n) ** 4).astype(np.float32)
    rank = rng.integers(-1, 6, n).astype(np.int32)
    want = ratebulk.word_bounds_host(corpus, offsets, DELIM)
    corpus_d, offsets_d, probs_d, rank_d = up(corpus), up(offsets), up(probs), up(rank)
    start, end = lm.word_bounds(corpus_d, offsets_d, up(DELIM))
    assert start.is_cuda and end.is_cuda and start.dtype == end.dtype == torch.int64
    assert np.array_equal(start.cpu().numpy(), want[0]) and np.array_equal(end.cpu().numpy(), want[1])
    none = lm.word_bounds(up(np.full(50, 4, dtype=np.int32)), up(np.array([0, 50])), up(DELIM))
    assert [tuple(t.shape) for t in none] == [(0,), (0,)]
    for with_rank, rank_t in ((rank, rank_d), (None, None)):
        ref = ratebulk.segments_host(probs, with_rank, offsets, want[0], want[1], 0.05, 1)
        rec = lm.rate_segments(probs_d, rank_t, offsets_d, start, end, 0.05, 1)
        assert all(t.is_cuda and tuple(t.shape) == (len(want[0]),) for t in rec)
        got = [t.cpu().numpy() for t in rec]
        assert [g.dtype for g in got] == [r.dtype for r in ref]
        for k in (0, 3, 4, 5):
            assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8))
        for k in (1, 2):
            assert (np.abs(got[k] - ref[k]) <= 1e-12 * np.maximum(1.0, np.abs(ref[k])) + ref[0] * 2.0 ** -50).all()
    rule = dict(min_n=2, min_bad=1, min_bpc=2.0)
    rec = lm.rate_segments(probs_d, rank_d, offsets_d, start, end, 0.05, 1)
    ref = ratebulk.segment_select_host(want[0], want[1], *[t.cpu().numpy() for t in rec], **rule)
    sel = lm.segment_select(start, end, rec, **rule)
    assert 0 < len(ref[0]) < len(want[0]) and len(sel) == 9 and all(t.is_cuda for t in sel)
    for g, r in zip(sel, ref):
        g = g.cpu().numpy()
        assert g.dtype == r.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(r).view(np.uint8))
    assert [tuple(t.shape) for t in lm.segment_select(start, end, rec, min_n=10 ** 6)] == [(0,)] * 9
    for wrong in (dict(min_n=0), dict(min_bad=-1), dict(min_bpc=-1.0), dict(min_bpc=float("nan"))):
        with pytest.raises(ValueError):
            lm.segment_select(start, end, rec, **wrong)
    with pytest.raises(ValueError):
        lm.rate_segments(probs_d, rank_d, offsets_d, start, end, 0.05, -1)
    with pytest.raises(ValueError):
        lm.rate_segments(probs_d, rank_d, offsets_d, start, end, float("nan"), 0)


# ---------------------------------------------------------------------------------------------- Rater
@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_rater_suspect_words_and_rate_segments(precision):
    """the small rater of test_rate_batch_bf16_matches_the_oracle_rater and its nine texts -- an empty one, a single character,
    one of 3 * length + 5 characters --, two contexts, four streams"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = contract_texts()
    assert sorted(len(t) for t in texts)[:2] == [0, 1] and max(len(t) for t in texts) > 3 * LENGTH
    hip = small_rater(hip_factory)
    assert all(hasattr(hip.model, name) for name in ("word_bounds", "rate_segments", "segment_select"))
    rated, bits = hip.rate_alternatives(texts, contexts, k=3, streams=4, precision=precision)
    max_prob = quantile_of(rated, 0.3)
    for rule in (dict(), dict(min_chars=3, min_bits_per_char=2.0), dict(delimiters="a\n", min_suspects=2)):
        found, bits2 = hip.suspect_words(texts, contexts, k=3, streams=4, max_prob=max_prob, min_rank=1, precision=precision, **rule)
        assert (np.abs(bits2 - bits) <= 1e-12 * np.maximum(1.0, np.abs(bits))).all()
        want, words = statements_over(hip, texts, rated, rule.get("delimiters", " \n"), max_prob, 1, rule.get("min_suspects", 1),
                                      rule.get("min_bits_per_char", 0.0), rule.get("min_chars", 1))
        selected = same_words(found, want, exact=False)
        print("%s %r: %d of %d words" % (precision, rule, selected, words))
        assert 0 < selected < words
    # caller-supplied segments against rate_batch
    probs, _ = hip.rate_batch(texts, contexts, streams=4, precision=precision)
    sizes = [len(t) for t in texts]
    rng = np.random.default_rng(9)
    segments = [(5, 0, sizes[5]), (5, 3, 9), (2, 0, 1), (2, 0, 2), (8, 10, 30), (5, 4, 40)]
    for _ in range(20):
        i = int(rng.integers(2, len(texts)))
        a = int(rng.integers(0, sizes[i] + 1))
        segments.append((i, a, int(rng.integers(a, sizes[i] + 1))))
    found = hip.rate_segments(texts, segments, contexts, streams=4, precision=precision)
    assert sum(len(f) for f in found) == len(segments) and all(type(f) is ratebatch.Segments for f in found)
    for i, one in enumerate(found):
        mine = [(a, b) for t, a, b in segments if t == i]
        assert one.spans() == mine
        start, end = np.array([a for a, _ in mine], dtype=np.int64), np.array([b for _, b in mine], dtype=np.int64)
        n, ref_bits, psum, least, worst, bad = ratebulk.segments_host(probs[i], None, [0, sizes[i]], start, end)
        assert np.array_equal(one.n, n) and np.array_equal(one.worst, worst) and not one.suspects.any()
        assert np.array_equal(one.min_prob.view(np.uint32), least.view(np.uint32))
        assert np.allclose(one.bits, ref_bits, rtol=1e-12, atol=0)
        assert np.allclose(one.mean_prob[n > 0], (psum / np.maximum(n, 1))[n > 0], rtol=1e-12, atol=0) and np.isnan(one.mean_prob[n == 0]).all()
    # afterwards: a freshly reset single row
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()
    found, b = hip.suspect_words(["", "a"], precision=precision)
    assert [len(f) for f in found] == [0, 0] and b.tolist() == [0.0, 0.0]
    assert hip.rate_segments(["", "a"], [(1, 0, 1)], precision=precision)[1].n.tolist() == [0]
