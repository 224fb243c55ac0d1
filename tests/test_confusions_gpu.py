"""Confusion counts on the GPU (run with -m gpu on an MI355X): kl_confusion_counts, `HipLM.confusion_counts`, `Rater.confusions`
and `keraslm-rate confusions`.

The kernels are held to their statement (`ratebulk.confusion_counts_host`, itself held to a brute force in test_confusions.py)
bit for bit: all four outputs are integers.  The inputs are kl_align_pairs' own device outputs on the same pairs.  Every output
byte is FILL before a call, 64 elements behind each output and 64 bytes behind the workspace must keep it.  The shapes are the
smallest at which the kernels can go wrong: all lanes on a handful of table slots, thousands of distinct records, span slots
and symbols a lane less and a lane more than a wave and a workgroup, more span slots and pairs than a grid, every pair of
lengths around max_chars, texts that end on a wave's edge."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebulk, windows
from tests.test_confusions import CASES, aligned, confusion_corpus, same_confusions, table_of
from tests.test_lexicon import pooled
from tests.test_rate_bulk_gpu import device, lib_and_stream, random_text, small_rater
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up
from tests.test_witnesses import edited, noisy

pytestmark = pytest.mark.gpu

GRID_THREADS = 1024 * 256      # lanes of a launch at most: span slots per sweep
GRID_WAVES = 1024 * 4          # ... and waves: pairs per sweep of the walk over the texts
OUT = ("rules", "count", "occ", "stats")


class Counts(object):
    """kl_confusion_counts on device copies of P pairs (lists of symbols) and on what kl_align_pairs left of them on the device"""
    NAMES = ("a_pool", "a_off", "b_pool", "b_off", "dist", "n_spans", "spans")

    def __init__(self, A, B, max_dist, join=0, a_off=None):
        torch, self.dev = device()
        self.torch = torch
        self.lib, self.stream = lib_and_stream()
        self.P, self.max_dist = len(A), max_dist
        pools = list(pooled(A) + pooled(B))
        if a_off is not None:
            pools[1] = np.asarray(a_off, dtype=np.int64)
        some = lambda a: up(a) if len(a) else torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.src = [some(pools[0]), up(pools[1]), some(pools[2]), up(pools[3])]
        longest = max(len(t) for t in A + B)
        self.src += [torch.empty(self.P, dtype=torch.int32, device=self.dev), torch.empty(self.P, dtype=torch.int32, device=self.dev),
                     torch.empty(self.P * max_dist * 4, dtype=torch.int32, device=self.dev)]
        ws = torch.empty(self.lib.kl_align_pairs_workspace_bytes(self.P, longest, max_dist), dtype=torch.uint8, device=self.dev)
        code = self.lib.kl_align_pairs(ptr(self.src[0]), len(pools[0]), ptr(self.src[1]), ptr(self.src[2]), len(pools[2]), ptr(self.src[3]),
                                       self.P, longest, max_dist, join, ptr(self.src[4]), ptr(self.src[5]), ptr(self.src[6]), ptr(ws),
                                       ws.numel(), self.stream)
        torch.cuda.synchronize()
        assert code == 0
        self.host = pools + [self.src[4].cpu().numpy(), self.src[5].cpu().numpy(), self.src[6].cpu().numpy().reshape(self.P, max_dist, 4)]

    def replace(self, name, values):
        """other device data under `name`, for the call and for the statement"""
        at = self.NAMES.index(name)
        self.host[at] = np.ascontiguousarray(values)
        self.src[at] = up(self.host[at].reshape(-1))

    def want(self, max_chars, room):
        return ratebulk.confusion_counts_host(*self.host, max_chars, room)

    def run(self, max_chars, room, ws_bytes=None, ws_fill=FILL, shift=None, **override):
        torch = self.torch
        rows = max(room, 1)
        self.out = [marked(rows * 10, torch.int32), marked(rows, torch.int64), marked(rows, torch.int64), marked(4, torch.int64)]
        max_dist = override.pop("max_dist", self.max_dist)
        self.n_ws = self.lib.kl_confusion_counts_workspace_bytes(self.P, min(max(max_dist, 1), 255), len(self.host[0]))
        self.ws = torch.full((self.n_ws + 64,), ws_fill, dtype=torch.uint8, device=self.dev)
        a = dict(zip(self.NAMES + OUT, [ptr(t) for t in self.src + self.out]), n_a=len(self.host[0]), n_b=len(self.host[2]), P=self.P,
                 ws=ptr(self.ws))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_confusion_counts(a["a_pool"], a["n_a"], a["a_off"], a["b_pool"], a["n_b"], a["b_off"], a["P"], max_dist,
                                            a["dist"], a["n_spans"], a["spans"], max_chars, room, a["rules"], a["count"], a["occ"],
                                            a["stats"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes, self.stream)
        torch.cuda.synchronize()
        return code

    def is_statement(self, max_chars, room, ws_fill=FILL):
        want = self.want(max_chars, room)
        assert self.run(max_chars, room, ws_fill=ws_fill) == 0
        for t, w, name in zip(self.out, want, OUT):
            assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size), (name, max_chars, room)
        assert (raw(self.ws)[self.n_ws:] == ws_fill).all()           # nothing behind the workspace
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def rows_of(want):
    rules, count, occ, stats = want
    return [(r[0], r[1], tuple(r[2:2 + r[0]]), tuple(r[6:6 + r[1]]), c, o)
            for r, c, o in zip(rules.tolist(), count.tolist(), occ.tolist()) if r[0] >= 0]


def test_all_lanes_on_a_handful_of_slots():
    """an alphabet of two symbols: more than 3000 spans counted into four distinct records at max_chars 1, and into a few dozen
    at 4 -- every lane adds to one of a few slots, and every position of the texts to one of two"""
    rng = np.random.default_rng(30)
    A = [rng.integers(0, 2, 40).tolist() for _ in range(1800)]
    B = [edited(rng, a, 2, int(rng.integers(3, 9))) for a in A]
    look = Counts(A, B, 8)
    rules, count, occ, stats = look.is_statement(1, 32)
    assert 4 <= stats[0] < 20 and stats[1] == count.sum() > 3000 and stats[2] > 0
    assert sorted(set(occ[:stats[0]].tolist())) == sorted(int((look.host[0][np.repeat(look.host[4] >= 0, 40)] == x).sum()) for x in (0, 1))
    rules, count, occ, stats = look.is_statement(4, 64)
    assert stats[0] < 64 and stats[1] > 6000 and (count[:stats[0]] <= occ[:stats[0]]).all()


def test_thousands_of_distinct_records():
    """every span a record of its own, symbols distinct throughout: 5000 slots taken of 16384, probing chains in both tables"""
    P, per = 250, 20
    A = [list(range(1000 + 64 * p, 1000 + 64 * p + 60)) for p in range(P)]
    B = [[-x if at % 3 == 1 else x for at, x in enumerate(a)] for a in A]
    look = Counts(A, B, per)
    rules, count, occ, stats = look.is_statement(4, P * per + 7)
    assert stats.tolist() == [P * per, P * per, 0, 0] and (count[:P * per] == 1).all() and (occ[:P * per] == 1).all()
    assert rules[:P * per, 2].tolist() == [a[at] for a in A for at in range(1, 60, 3)]      # the order of first occurrence
    # the same spans, each twice: half the pairs repeat the other half
    look = Counts(A[:125] + A[:125], B[:125] + B[:125], per)
    rules, count, occ, stats = look.is_statement(4, 2500)
    assert stats.tolist() == [2500, 5000, 0, 0] and (count == 2).all() and (occ == 2).all()


@pytest.mark.parametrize("n", [63, 64, 65, 257, 1025])
def test_span_slots_and_symbols_around_waves_and_workgroups(n):
    """n span slots and n symbols: n pairs of one symbol at max_dist 1, and (up to 255) one pair of n symbols at max_dist n"""
    rng = np.random.default_rng(n)
    A = [[int(x)] for x in rng.integers(0, 5, n)]
    B = [[int(x)] for x in rng.integers(0, 5, n)]
    B[n - 1] = [A[n - 1][0] + 7]                                     # the last slot holds a record of its own
    look = Counts(A, B, 1)
    rules, count, occ, stats = look.is_statement(1, 64)
    assert stats[1] == sum(a != b for a, b in zip(A, B)) and rules[stats[0] - 1, 6] == A[n - 1][0] + 7
    if n <= 255:
        a = rng.integers(0, 4, n).tolist()
        b = list(a)
        b[n - 1] = 9                                                 # the last symbol, read alone and as the end of longer sources
        for at in range(0, n - 1, 3):
            b[at] = 4 + a[at]
        look = Counts([a], [b], n)
        rules, count, occ, stats = look.is_statement(2, 64)
        changed = sorted(set(range(0, n - 1, 3)) | {n - 1})
        assert look.host[4][0] == len(changed) and stats[1] == len(changed) - (n - 2 in changed) and stats[2] == 0


def test_more_span_slots_and_pairs_than_a_grid():
    """4200 pairs of 63 span slots: more slots than the lanes and more pairs than the waves of one launch"""
    rng = np.random.default_rng(31)
    P, K = GRID_WAVES + 104, 63
    assert P * K > GRID_THREADS
    A = [rng.integers(0, 3, 6).tolist() for _ in range(P)]
    B = [edited(rng, a, 3, int(rng.integers(0, 3))) for a in A]
    B[P - 1] = [7] + A[P - 1][1:]                                    # the last pair holds a record of its own
    look = Counts(A, B, K)
    rules, count, occ, stats = look.is_statement(2, 256)
    assert stats[1] > 2000 and rules[stats[0] - 1, 6] == 7 and count[stats[0] - 1] == 1
    assert occ[0] == sum(a[i:i + rules[0, 0]] == rules[0, 2:2 + rules[0, 0]].tolist() for a in A for i in range(6))


@pytest.mark.parametrize("max_chars", [4, 2])
def test_every_pair_of_lengths_around_max_chars(max_chars):
    """sources and targets of 0 .. 5 symbols, inside a text (an empty source is anchored in front) and at its beginning (behind)"""
    A, B, expect = [], [], []
    for inside in (True, False):
        for s in range(6):
            for t in range(6):
                first = 100 * len(A)
                source, target = list(range(first + 10, first + 10 + s)), list(range(first + 20, first + 20 + t))
                left = [first + 1] if inside else []
                A.append(left + source + [first + 2])
                B.append(left + target + [first + 2])
                anchor = 1 if s == 0 else 0
                expect.append(None if s == t == 0 else s + anchor <= max_chars and t + anchor <= max_chars)
    look = Counts(A, B, 5)
    rules, count, occ, stats = look.is_statement(max_chars, 80)
    assert stats.tolist() == [expect.count(True), expect.count(True), expect.count(False), 0]
    lengths = [(s + (s == 0), t + (s == 0)) for s in range(6) for t in range(6) if s + (s == 0) <= max_chars and t + (s == 0) <= max_chars and s + t]
    assert [tuple(r[:2]) for r in rules[:stats[0]].tolist()] == lengths * 2


def test_any_int32_is_a_symbol():
    low, high = -2 ** 31, 2 ** 31 - 1
    A = [[5, low, 6, high, 7, -1, 8, 0, 9], [high, high, high, low], [0, 0]]
    B = [[5, high, 6, low, 7, 0, 8, -1, 9], [high, low], [0, -1, 0]]
    look = Counts(A, B, 4)
    want = look.is_statement(4, 16)
    assert rows_of(want) == [(1, 1, (low,), (high,), 1, 2), (1, 1, (high,), (low,), 1, 4), (1, 1, (-1,), (0,), 1, 1), (1, 1, (0,), (-1,), 1, 3),
                             (2, 0, (high, high), (), 1, 2), (1, 2, (0,), (0, -1), 1, 3)]


def test_the_hand_made_cases_on_the_device():
    for A, B, max_dist, table, stats in CASES:
        look = Counts(*[[[ord(c) for c in s] for s in side] for side in (A, B)], max_dist)
        rules, count, occ, got = look.is_statement(4, 5)
        assert table_of(rules, count, occ) == table and tuple(got.tolist()) == stats


def test_texts_that_end_on_a_waves_edge():
    """the a-texts are 64, 128, 1 and 63 symbols: a source that would stand across a border -- the last symbol of one text, the
    first of the next -- is not counted, nor is anything in a rejected pair's text between two accepted ones"""
    x, y = 1, 2
    fill = lambda n: [10 + i % 7 for i in range(n)]
    A = [fill(61) + [x, y, x], [y] + fill(126) + [x], [y], [y] * 2 + fill(59) + [x, y], [x, y] * 32, [y, x] + fill(60) + [x, y]]
    B = [fill(61) + [3, x], [y] + fill(126) + [x], [y], [y] * 2 + fill(59) + [x, y], [4] * 100, [y, x] + fill(60) + [x, y]]
    look = Counts(A, B, 8)
    assert look.host[4].tolist() == [2, 0, 0, 0, -1, 0]
    want = look.is_statement(4, 8)
    assert rows_of(want) == [(2, 1, (x, y), (3,), 1, 3)]            # in texts 0, 3 and 5; not 0|1, 1|2, 2|3, and not text 4's 32
    # a pair that was aligned but whose offsets descend, or reach outside the pool, is skipped like a rejected one
    off = look.host[1].copy()
    off[3] = off[4] + 2                                              # pair 2 now ends inside text 4, pair 3 descends
    bad = Counts(A, B, 8)
    bad.replace("a_off", off)
    bad.replace("dist", np.array([2, 0, 0, 0, 3, 0], dtype=np.int32))
    bad.replace("n_spans", np.array([1, 0, 0, 1, 0, 0], dtype=np.int32))
    want = bad.is_statement(4, 8)
    assert rows_of(want)[0][:4] == (2, 1, (x, y), (3,)) and want[3].tolist() == [1, 1, 0, 0]
    assert rows_of(want)[0][5] == 1 + 2 + 32 + 1                     # texts 0, 2 (as its offsets now say: up into text 4), 4 and 5
    assert bad.run(4, 8, n_a=len(bad.host[0]) - 2) == 0              # the last text reaches outside the pool now
    short = ratebulk.confusion_counts_host(bad.host[0][:-2], *bad.host[1:], 4, 8)
    assert all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size) for t, w in zip(bad.out, short)) and short[2][0] == 35


def test_span_fields_outside_the_texts_are_long():
    rng = np.random.default_rng(32)
    A = [rng.integers(0, 3, 12).tolist() for _ in range(40)]
    B = [edited(rng, a, 3, int(rng.integers(1, 4))) for a in A]
    look = Counts(A, B, 4)
    clean = look.want(4, 64)
    spans, n_spans = look.host[6].copy(), look.host[5].copy()
    n_spans[:8] = [4, 4, 4, 4, 4, 9, -3, 2 ** 31 - 1]                # (more than max_dist: the slots there are; fewer than none: none)
    spans[0] = [[0, 13, 0, 1], [-1, 2, 0, 1], [3, 2, 1, 2], [2, 3, 0, 2 ** 31 - 1]]
    spans[1] = [[2, 3, -2 ** 31, 1], [2, 3, 4, 3], [5, 5, 0, 2], [0, 0, 0, len(B[1])]]      # (no character in front / behind in b)
    spans[2] = [[0, 12, 0, 1], [12, 12, 1, 1], [0, 0, 0, 0], [11, 12, 3, 3]]                # (too long, and three that are inside)
    look.replace("spans", spans)
    look.replace("n_spans", n_spans)
    rules, count, occ, stats = look.is_statement(4, 64)
    assert stats[2] >= clean[3][2] + 9 and stats[1] > 20


def test_room_below_at_and_above_the_number_of_records():
    rng = np.random.default_rng(33)
    A = [rng.integers(0, 4, 30).tolist() for _ in range(60)]
    B = [edited(rng, a, 4, int(rng.integers(0, 6))) for a in A]
    look = Counts(A, B, 6)
    full = look.want(4, 4096)
    R = int(full[3][0])
    assert R > 40
    for room in (1, R - 1, R, R + 7):
        rules, count, occ, stats = look.is_statement(4, room)
        assert stats.tolist() == full[3].tolist() and np.array_equal(rules[:R], full[0][:min(R, room)])


@pytest.mark.parametrize("max_dist", [1, 255])
def test_the_least_and_the_largest_max_dist(max_dist):
    rng = np.random.default_rng(max_dist)
    A = [rng.integers(0, 6, 300).tolist() for _ in range(5)] + [[1], []]
    B = [edited(rng, a, 6, min(max_dist, 90)) for a in A[:5]] + [[2], [3]]
    look = Counts(A, B, max_dist)
    rules, count, occ, stats = look.is_statement(3, 512)
    assert (look.host[4] >= 0).sum() >= 3 and stats[1] >= (1 if max_dist == 1 else 150) and stats[3] == 1


def test_two_calls_give_the_same_bytes():
    rng = np.random.default_rng(34)
    A = [rng.integers(0, 5, 50).tolist() for _ in range(300)]
    B = [edited(rng, a, 5, int(rng.integers(0, 9))) for a in A]
    look = Counts(A, B, 8)
    look.is_statement(4, 2048)
    first = [raw(t).copy() for t in look.out]
    look.is_statement(4, 2048, ws_fill=0x3C)                         # whatever the workspace held
    assert all(np.array_equal(x, raw(t)) for x, t in zip(first, look.out))


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(35)
    A = [rng.integers(0, 4, 20).tolist() for _ in range(9)]
    B = [edited(rng, a, 4, 2) for a in A]
    look = Counts(A, B, 4)
    size = look.lib.kl_confusion_counts_workspace_bytes
    assert size(0, 4, 10) == 0 and size(2 ** 31, 4, 10) == 0 and size(9, 0, 10) == 0 and size(9, 256, 10) == 0 and size(9, 4, 2 ** 40 + 1) == 0
    assert size(9, 4, 180) == size(9, 4, 0) >= 36 * (40 + 8) + 4 * 8 * 72 and size(2 ** 31 - 1, 255, 2 ** 40) > 2 ** 43
    cases = [dict(P=0), dict(P=2 ** 31), dict(n_a=2 ** 40 + 1), dict(n_b=2 ** 40 + 1), dict(max_dist=0), dict(max_dist=256), dict(max_dist=-1)]
    cases += [{name: None} for name in look.NAMES + OUT + ("ws",)]
    cases += [dict(shift={name: 2}) for name in ("a_pool", "b_pool", "dist", "n_spans", "spans", "rules")]
    cases += [dict(shift={name: 4}) for name in ("a_off", "b_off", "count", "occ", "stats")]
    for case in cases:
        assert look.run(4, 16, **case) == KL_ERR_ARG, case
        assert look.untouched(), case
    for max_chars, room in ((0, 16), (5, 16), (-1, 16), (4, 0)):
        assert look.run(max_chars, room) == KL_ERR_ARG and look.untouched(), (max_chars, room)
    assert look.run(4, 16, ws_bytes=look.n_ws - 1) == KL_ERR_WORKSPACE and look.untouched()
    assert look.run(4, 16, ws_bytes=0) == KL_ERR_WORKSPACE and look.untouched()
    assert look.run(4, 16, shift=dict(ws=4)) == KL_ERR_WORKSPACE and look.untouched()
    look.is_statement(4, 16)
    # a pool may be null when it holds nothing
    empty = Counts([[], []], [[], []], 2)
    assert empty.run(4, 3, a_pool=None, b_pool=None, n_a=0, n_b=0) == 0
    assert all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size) for t, w in zip(empty.out, empty.want(4, 3)))


# ---------------------------------------------------------------------------------------------- engine, Rater, command line
def test_engine_wrapper():
    from ocrd_keraslm_amd.lib import hipabi
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(36)
    A = [rng.integers(0, 4, int(rng.integers(0, 50))).tolist() for _ in range(30)]
    B = [edited(rng, a, 4, int(rng.integers(0, 9))) for a in A]
    host = pooled(A) + pooled(B)
    texts = [up(x) for x in host]
    spans = lm.align_pairs(*texts, 60, 5, 0)
    want = ratebulk.confusion_counts_host(*host, *[t.cpu().numpy() for t in spans], 3, 40)
    got = lm.confusion_counts(*texts, *spans, 3, 40)
    assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32] + [torch.int64] * 3
    assert [tuple(t.shape) for t in got] == [(40, 10), (40,), (40,), (4,)]
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    assert want[3][0] > 10
    names = ("a_pool", "a_off", "b_pool", "b_off", "dist", "n_spans", "spans", "max_chars", "room")
    for wrong in (dict(a_pool=texts[0].long()), dict(a_off=texts[1].int()), dict(b_pool=texts[2][::2]), dict(b_off=torch.from_numpy(host[3])),
                  dict(b_off=texts[3][:-1]), dict(dist=spans[0][:-1]), dict(n_spans=spans[1].long()), dict(spans=spans[2].reshape(-1)),
                  dict(spans=spans[2][:, :, :3]), dict(max_chars=0), dict(max_chars=5), dict(room=0)):
        a = dict(dict(zip(names, texts + list(spans) + [3, 40])), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.confusion_counts(*[a[name] for name in names])


def test_rater_confusions_on_the_device(monkeypatch):
    from tests.test_rater_golden import hip_factory
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "confusion_counts")
    texts, truths = confusion_corpus(4)
    texts += ["été", "modern times", "\U0001F600x"]
    truths += ["ete", "modem times", "\U0001F601x"]
    a, b = [windows.normalize(t) for t in texts], [windows.normalize(t) for t in truths]
    calls = []
    inner = hip.model.confusion_counts
    monkeypatch.setattr(hip.model, "confusion_counts", lambda *args: calls.append(args[-1]) or inner(*args))
    for room in (65536, 8):                                          # (8: fewer than there are records -- a second call with R)
        monkeypatch.setattr(type(hip), "_CONFUSION_ROOM", room)
        for max_dist, join, max_chars in ((8, 0, 4), (8, 1, 2)):
            del calls[:]
            got = hip.confusions(texts, truths, max_dist=max_dist, join=join, max_chars=max_chars)
            args = aligned(a, b, max_dist, join)
            same_confusions(got, *ratebulk.confusion_counts_host(*args, max_chars, 1000), args[4], b)
            assert len(got) > 8 and calls == ([room] if room > 8 else [8, len(got)])
    assert ("\U0001F600", "\U0001F601") in zip(got.sources, got.targets)
    del calls[:]
    none = hip.confusions([], [])
    assert len(none) == 0 and none.rules() == [] and calls == []                             # no pairs: no launch


def test_cli_confusions_on_the_device(tmp_path):
    from ocrd_keraslm_amd.scripts import run
    from tests.test_rater_golden import hip_factory
    model = str(tmp_path / "model.h5")
    small_rater(hip_factory).save(model)
    rng = np.random.default_rng(37)
    truth = tmp_path / "gt"
    truth.mkdir()
    files, texts, truths = [], [], []
    for i, size in enumerate((90, 70, 80)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        truths.append(random_text(rng, size))
        texts.append(noisy(rng, truths[-1].replace("a", "e"), 3))
        name.write_text(texts[-1])
        (truth / name.name).write_text(truths[-1])
        files.append(str(name))
    res = CliRunner().invoke(run.cli, ["confusions", "-m", model, "--truth", str(truth), "--max-dist", "30", "--counts", "--min-count", "1"] + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    ref = run._load(model)
    assert hasattr(ref.model, "confusion_counts")
    found = ref.confusions(texts, truths, max_dist=30)
    lines = [json.loads(l) for l in res.stdout.strip().split("\n")]
    kept = [i for rows in found.kept(min_count=1) for i in rows]
    assert lines == [dict(source=found.sources[i], target=found.targets[i], count=int(found.count[i]), occ=int(found.occ[i]),
                          rate=found.rate(i)) for i in kept]
    assert lines[0]["source"] == "e" and lines[0]["target"] == "a" and lines[0]["count"] > 10
    last = json.loads(res.stderr.strip().split("\n")[-1])
    assert last == dict(pairs=3, different=0, long=found.skipped["long"], empty=0, chars=240, edits=found.edits, cer=found.cer)
    table = CliRunner().invoke(run.cli, ["confusions", "-m", model, "--truth", str(truth), "--max-dist", "30"] + files)
    assert table.exit_code == 0 and table.stdout.startswith("e\ta")
