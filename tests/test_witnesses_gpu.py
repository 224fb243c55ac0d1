"""The alignment of two readings on the GPU (run with -m gpu on an MI355X): kl_align_pairs, `HipLM.align_pairs`, `Rater.align`,
`Rater.merge_witnesses` and `keraslm-rate witnesses`.

The kernel is held to its numpy statement (`ratebulk.align_pairs_host`, itself held to a full distance matrix in
test_witnesses.py) bit for bit: all three outputs are integers.  Every output byte is FILL before a call, 64 elements behind each
output must keep it, and the workspace is filled too.  The shapes are the smallest at which the kernel can go wrong: bands of a
lane less and a lane more than whole waves, distances and length differences at max_dist and one beyond, texts shorter than the
band, lengths on both sides of the switch of the two-bit cells from LDS to the workspace, more pairs than workgroups."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.test_lexicon import pooled, same_rescored
from tests.test_rate_bulk_gpu import device, lib_and_stream, random_text, small_rater
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up
from tests.test_witnesses import edited, noisy, witness_corpus

pytestmark = pytest.mark.gpu

LEN_MAX = 4096
GRID_MAX = 512             # workgroups of a launch at most
LDS_CELL_WORDS = 6144      # (n / 16 + 1) * (2 * max_dist + 1) words of two-bit cells stay in LDS up to this many


class Align(object):
    """kl_align_pairs on device copies of P pairs (lists of symbols); three outputs plus a guard band each"""
    NAMES = ("a_pool", "a_off", "b_pool", "b_off", "dist", "n_spans", "spans")

    def __init__(self, A, B):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.P = len(A)
        self.host = pooled(A) + pooled(B)
        some = lambda a: up(a) if len(a) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        self.src = [some(self.host[0]), up(self.host[1]), some(self.host[2]), up(self.host[3])]
        self.longest = max(len(t) for t in A + B)

    def want(self, max_len, max_dist, join):
        return ratebulk.align_pairs_host(*self.host, max_len, max_dist, join)

    def run(self, max_len, max_dist, join, room=None, ws_bytes=None, shift=None, **override):
        torch = self.torch
        room = max_dist if room is None else room
        self.out = [marked(self.P, torch.int32), marked(self.P, torch.int32), marked(self.P * room * 4, torch.int32)]
        self.n_ws = self.lib.kl_align_pairs_workspace_bytes(self.P, min(max(max_len, 0), LEN_MAX), min(max(max_dist, 1), 255))
        self.ws = torch.full((self.n_ws + 64,), FILL, dtype=torch.uint8, device=self.dev)
        a = dict(zip(self.NAMES, [ptr(t) for t in self.src] + [ptr(t) for t in self.out]), n_a=len(self.host[0]),
                 n_b=len(self.host[2]), P=self.P, ws=ptr(self.ws))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_align_pairs(a["a_pool"], a["n_a"], a["a_off"], a["b_pool"], a["n_b"], a["b_off"], a["P"], max_len, max_dist,
                                       join, a["dist"], a["n_spans"], a["spans"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes,
                                       self.stream)
        torch.cuda.synchronize()
        return code

    def is_statement(self, max_len, max_dist, join):
        want = self.want(max_len, max_dist, join)
        assert self.run(max_len, max_dist, join) == 0
        for t, w, name in zip(self.out, want, ("dist", "n_spans", "spans")):
            assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size), (name, max_len, max_dist, join)
        assert (raw(self.ws)[self.n_ws:] == FILL).all()              # nothing behind the workspace
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def distinct(n, first=1000):
    return list(range(first, first + n))


def substituted(text, count, every):
    """`count` substitutions `every` symbols apart, from position every - 1 on: among distinct symbols the distance is count"""
    out = list(text)
    for c in range(count):
        out[every - 1 + c * every] = -out[every - 1 + c * every]
    return out


def band_pairs(rng, K):
    """pairs for a band of K: length differences and distances at K and K + 1, texts shorter than the band, random edits"""
    n = 2 * K + 6
    text = distinct(n)
    A, B, expect = [], [], []
    for a, b, d in ((text, text[:5] + distinct(K, 5000) + text[5:], K),             # |n - m| = K
                    (text, text[:5] + distinct(K + 1, 5000) + text[5:], -1),         # |n - m| = K + 1: no DP
                    (text + distinct(K, 7000), text, K), (text + distinct(K + 1, 7000), text, -1),
                    (text, substituted(text, K, 2), K),                              # dist = K exactly
                    (text, substituted(text, K + 1, 2)[:n], -1),                     # dist = K + 1 with n == m: the DP says so
                    (distinct(K // 2), distinct(K - K // 2, 3000), K - K // 2),      # n + m = K: shorter than the band
                    (distinct(1), [], 1), ([], [], 0), (text, text, 0)):
        A.append(list(a)), B.append(list(b)), expect.append(d)
    for _ in range(6):
        a = rng.integers(0, 4, int(rng.integers(1, n))).tolist()
        A.append(a), B.append(edited(rng, a, 4, int(rng.integers(0, min(K, 12) + 2)))), expect.append(None)
    return A, B, expect


@pytest.mark.parametrize("K", [1, 31, 32, 63, 64, 127, 128, 255])
def test_band_widths_across_waves_and_workgroup_sizes(K):
    """2 K + 1 = 3, 63, 65, 127, 129, 255, 257, 511 lanes"""
    rng = np.random.default_rng(K)
    A, B, expect = band_pairs(rng, K)
    look = Align(A, B)
    for join in (1, 0):
        dist, n_spans, spans = look.is_statement(look.longest, K, join)
        assert [d for d, e in zip(dist.tolist(), expect) if e is not None] == [e for e in expect if e is not None]
    assert n_spans[4] == K and spans[4, K - 1].tolist() == [2 * K - 1, 2 * K, 2 * K - 1, 2 * K]
    assert n_spans[0] == 1 and spans[0, 0].tolist() == [5, 5, 5, 5 + K] and spans[2, 0].tolist() == [2 * K + 6, 3 * K + 6, 2 * K + 6, 2 * K + 6]


@pytest.mark.parametrize("K,edge", [(127, 383), (32, 1503)])
def test_lengths_on_both_sides_of_the_lds_workspace_switch(K, edge):
    """the two-bit cells of a pair lie in LDS while (n / 16 + 1) * (2 K + 1) <= 6144 words: n = edge is the last such length.
    With max_len = edge nothing touches the workspace; with max_len = edge + 2 the pairs of edge + 1 and edge + 2 symbols do,
    the shorter ones in the same call still do not -- same outputs either way"""
    L = 2 * K + 1
    assert (edge // 16 + 1) * L <= LDS_CELL_WORDS < ((edge + 1) // 16 + 1) * L
    rng = np.random.default_rng(edge)
    A, B = [], []
    for n in (edge - 1, edge, edge + 1, edge + 2, 40, edge + 1):
        a = rng.integers(0, 5, n).tolist()
        b = list(a)
        for at in rng.integers(0, n, 5):                    # substitutions, a deletion and an insertion: the length stays
            b[int(at)] = -1
        del b[int(rng.integers(0, n))]
        b.insert(int(rng.integers(0, n)), -2)
        A.append(a), B.append(b)
    B[5] = list(A[5])
    look = Align(A[:2] + A[4:5], B[:2] + B[4:5])
    look.is_statement(edge, K, 0)
    assert look.n_ws == 8 and (raw(look.ws) == FILL).all()
    both = Align(A, B)
    dist, n_spans, spans = both.is_statement(edge + 2, K, 0)
    assert both.n_ws >= 6 * 4 * LDS_CELL_WORDS and (raw(both.ws)[:both.n_ws] != FILL).any() and (dist[:5] > 0).all() and dist[5] == 0
    short = look.want(edge, K, 0)
    assert all(np.array_equal(s[:2], w[:2]) for s, w in zip(short, (dist, n_spans, spans)))
    both.is_statement(edge + 2, K, 2)


def test_more_pairs_than_workgroups_reuse_their_scratch():
    """three and a bit rounds of the grid; a workgroup's successive pairs alternate between 12 and 4 symbols, so that what a
    longer pair left in the cells, the texts or the spans would show in the next one"""
    rng = np.random.default_rng(20)
    P = 3 * GRID_MAX + 41
    A, B = [], []
    for p in range(P):
        long = (p // GRID_MAX + p) % 2 == 0
        a = rng.integers(0, 3, 12 if long else 4).tolist()
        A.append(a), B.append(edited(rng, a, 3, int(rng.integers(0, 5 if long else 3))))
    look = Align(A, B)
    dist, n_spans, spans = look.is_statement(look.longest, 3, 0)
    assert set(dist.tolist()) == {-1, 0, 1, 2, 3} and n_spans.max() == 3
    look.is_statement(look.longest, 4, 1)
    # fewer pairs than the arrays hold: nothing behind P is written
    want = look.want(look.longest, 3, 0)
    assert look.run(look.longest, 3, 0, P=GRID_MAX + 5) == 0
    for t, w in zip(look.out, want):
        assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), (GRID_MAX + 5) * (w.size // P))


def test_gaps_at_the_ends_and_one_long_gap():
    text = distinct(60)
    other = distinct(40, 9000)
    A = [text, text, text, text, text, text, text, other[:20], [], text, text]
    B = [text[7:], other[:7] + text, text[:-7], text + other[:7], other[:3] + text[3:-4] + other[:4], text[:30] + other[:20] + text[30:],
         text[:20] + text[40:], [], other[:20], substituted(text, 3, 1), text[:57] + substituted(text, 60, 1)[57:]]
    look = Align(A, B)
    for K in (7, 20):
        dist, n_spans, spans = look.is_statement(80, K, 0)
        assert dist.tolist() == [7, 7, 7, 7, 7] + ([20] * 4 if K == 20 else [-1] * 4) + [3, 3]
        assert spans[0, 0].tolist() == [0, 7, 0, 0] and spans[1, 0].tolist() == [0, 0, 0, 7] and spans[2, 0].tolist() == [53, 60, 53, 53]
        assert spans[3, 0].tolist() == [60, 60, 60, 67] and spans[4, :2].tolist() == [[0, 3, 0, 3], [56, 60, 56, 60]]
        assert spans[9, 0].tolist() == [0, 3, 0, 3] and spans[10, 0].tolist() == [57, 60, 57, 60]
    assert spans[5, 0].tolist() == [30, 30, 30, 50] and spans[6, 0].tolist() == [20, 40, 20, 20] and n_spans[5:9].tolist() == [1] * 4
    assert spans[7, 0].tolist() == [0, 20, 0, 0] and spans[8, 0].tolist() == [0, 0, 0, 20]


def test_the_longest_texts():
    """n = m = KL_ALIGN_LEN_MAX with max_dist 8: a substitution at both ends, an insertion and a deletion in between (the
    statement runs the same band); one symbol more is -2"""
    rng = np.random.default_rng(21)
    a = rng.integers(0, 50, LEN_MAX).tolist()
    b = list(a)
    b[0], b[-1] = -1, -2
    b.insert(1000, -3)
    del b[3000]
    b[2000] = -4
    b[2002] = -5
    assert len(b) == LEN_MAX
    look = Align([a, a[:50]], [b, a[:49]])
    dist, n_spans, spans = look.is_statement(LEN_MAX, 8, 0)
    assert dist.tolist() == [6, 1] and n_spans.tolist() == [6, 1]
    assert spans[0, 0].tolist() == [0, 1, 0, 1] and spans[0, 5].tolist() == [LEN_MAX - 1, LEN_MAX, LEN_MAX - 1, LEN_MAX]
    dist, n_spans, spans = look.is_statement(LEN_MAX, 8, 1)
    assert n_spans.tolist() == [5, 1]
    dist, n_spans, spans = look.is_statement(LEN_MAX - 1, 8, 0)
    assert dist.tolist() == [-2, 1]


def test_too_long_pairs_and_offsets_outside_the_pools():
    rng = np.random.default_rng(22)
    A = [rng.integers(0, 4, n).tolist() for n in (30, 31, 12, 30, 5, 31)]
    B = [edited(rng, a, 4, 2) for a in A]
    B[4] = rng.integers(0, 4, 31).tolist()                 # the witness alone is too long
    look = Align(A, B)
    full = look.is_statement(look.longest, 6, 0)
    dist, n_spans, spans = look.is_statement(30, 6, 0)
    too_long = [len(a) > 30 or len(b) > 30 for a, b in zip(A, B)]
    assert too_long[1] and too_long[4] and too_long[5] and not too_long[2]
    for p in range(look.P):
        if too_long[p]:
            assert dist[p] == -2 and n_spans[p] == 0 and (spans[p] == -1).all()
        else:
            assert dist[p] == full[0][p] and np.array_equal(spans[p], full[2][p])      # the neighbours are unaffected
    look.is_statement(0, 6, 0)
    # offsets are device data: descending ones, and ones beyond n_a / n_b, give -2 and nothing of the pair is read
    off = look.host[1].copy()
    off[3] = off[4] + 2
    bad = Align(A, B)
    bad.host = (look.host[0], off) + look.host[2:]
    bad.src[1] = up(off)
    dist, _, _ = bad.is_statement(look.longest, 6, 0)
    assert dist[2] == -2 and dist[3] == -2 and dist[4] == full[0][4]
    want = ratebulk.align_pairs_host(look.host[0][:-3], look.host[1], look.host[2][:-40], look.host[3], look.longest, 6, 0)
    assert look.run(look.longest, 6, 0, n_a=len(look.host[0]) - 3, n_b=len(look.host[2]) - 40) == 0
    assert all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size) for t, w in zip(look.out, want))
    assert want[0][-1] == -2 and want[0][-2] == -2 and want[0][0] == full[0][0]
    # a pool may be null when it holds nothing
    empty = Align([[], []], [[], []])
    assert empty.run(0, 2, 0, a_pool=None, b_pool=None, n_a=0, n_b=0) == 0
    assert all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size) for t, w in zip(empty.out, empty.want(0, 2, 0)))


def test_join_merges_differences_up_to_that_many_matches_apart():
    a = distinct(40)
    b = list(a)
    for at in (3, 5, 10, 13, 20, 25):                      # 1, 4, 2, 6 and 4 matches between them
        b[at] = -b[at]
    b.insert(32, -1)                                       # an insertion two matches in front of a deletion
    del b[36]
    look = Align([a, b], [b, a])
    counts = {}
    for join in (0, 1, 3):
        dist, n_spans, spans = look.is_statement(41, 9, join)
        assert dist.tolist() == [8, 8]
        counts[join] = n_spans.tolist()
    assert counts == {0: [8, 8], 1: [7, 7], 3: [5, 5]}
    assert spans[0, 0].tolist() == [3, 6, 3, 6] and spans[0, 1].tolist() == [10, 14, 10, 14] and spans[0, 4].tolist() == [32, 36, 32, 36]


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(23)
    A = [rng.integers(0, 4, 20).tolist() for _ in range(9)]
    B = [edited(rng, a, 4, 2) for a in A]
    look = Align(A, B)
    size = look.lib.kl_align_pairs_workspace_bytes
    assert size(0, 30, 4) == 0 and size(2 ** 31, 30, 4) == 0 and size(9, -1, 4) == 0 and size(9, LEN_MAX + 1, 4) == 0
    assert size(9, 30, 0) == 0 and size(9, 30, 256) == 0 and size(9, 30, 4) == 8
    assert size(9, LEN_MAX, 255) == 9 * size(1, LEN_MAX, 255) and size(10 ** 6, LEN_MAX, 255) == GRID_MAX * size(1, LEN_MAX, 255)
    cases = [dict(P=0), dict(P=2 ** 31), dict(n_a=2 ** 40 + 1), dict(n_b=2 ** 40 + 1)]
    cases += [{name: None} for name in look.NAMES + ("ws",)]
    cases += [dict(shift={name: 2}) for name in ("a_pool", "b_pool", "dist", "n_spans", "spans")]
    cases += [dict(shift={name: 4}) for name in ("a_off", "b_off")]
    for case in cases:
        assert look.run(30, 4, 0, **case) == KL_ERR_ARG, case
        assert look.untouched(), case
    for max_len, max_dist, join in ((-1, 4, 0), (LEN_MAX + 1, 4, 0), (30, 0, 0), (30, 256, 0), (30, -1, 0), (30, 4, -1)):
        assert look.run(max_len, max_dist, join, room=4) == KL_ERR_ARG and look.untouched(), (max_len, max_dist, join)
    assert look.run(30, 4, 0, ws_bytes=7) == KL_ERR_WORKSPACE and look.untouched()
    assert look.run(30, 4, 0, shift=dict(ws=4)) == KL_ERR_WORKSPACE and look.untouched()
    assert look.run(LEN_MAX, 255, 0, room=255, ws_bytes=size(9, LEN_MAX, 255) - 1) == KL_ERR_WORKSPACE and look.untouched()
    look.is_statement(30, 4, 0)


def test_two_calls_give_the_same_bytes():
    rng = np.random.default_rng(24)
    A = [rng.integers(0, 4, int(rng.integers(300, 420))).tolist() for _ in range(40)]
    B = [edited(rng, a, 4, int(rng.integers(0, 40))) for a in A]
    look = Align(A, B)
    look.is_statement(look.longest, 127, 1)                # (some pairs in LDS, some in the workspace)
    first = [raw(t).copy() for t in look.out]
    assert look.run(look.longest, 127, 1) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, look.out))


# ---------------------------------------------------------------------------------------------- engine and Rater
def codes(strings):
    return pooled([[ord(c) for c in windows.normalize(s)] for s in strings])


def test_engine_wrapper_and_rater_align():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rater_golden import hip_factory
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(25)
    A = [rng.integers(0, 4, int(rng.integers(0, 50))).tolist() for _ in range(30)]
    B = [edited(rng, a, 4, int(rng.integers(0, 9))) for a in A]
    host = pooled(A) + pooled(B)
    want = ratebulk.align_pairs_host(*host, 50, 5, 1)
    got = lm.align_pairs(*[up(a) for a in host], 50, 5, 1)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got) and [tuple(t.shape) for t in got] == [(30,), (30,), (30, 5, 4)]
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    names = ("a_pool", "a_off", "b_pool", "b_off")
    for wrong in (dict(a_pool=up(host[0]).long()), dict(a_off=up(host[1]).int()), dict(b_pool=up(host[2])[::2]), dict(b_off=torch.from_numpy(host[3])),
                  dict(b_off=up(host[3])[:-1]), dict(max_len=4097), dict(max_dist=0), dict(max_dist=256), dict(join=-1)):
        a = dict(dict(zip(names, [up(x) for x in host]), max_len=50, max_dist=5, join=1), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.align_pairs(a["a_pool"], a["a_off"], a["b_pool"], a["b_off"], a["max_len"], a["max_dist"], a["join"])
    # the Rater: normalised, code points, the used spans compacted on the device
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "align_pairs")
    texts, witnesses, _ = witness_corpus(5)
    pairs = [(i, w) for i, ws in enumerate(witnesses) for w in range(len(ws))]
    a = [texts[i] for i, _ in pairs] + ["été", "\U0001F600x", "", "abc"]
    b = [witnesses[i][w] for i, w in pairs] + ["été", "\U0001F601x", "ab", "abc"]
    for max_dist, join in ((6, 0), (40, 2)):
        got = hip.align(a, b, max_dist=max_dist, join=join)
        dist, n_spans, spans = ratebulk.align_pairs_host(*codes(a), *codes(b), 60, max_dist, join)
        assert len(got) == len(a)
        for p, one in enumerate(got):
            assert type(one) is ratebatch.Alignment and one.dist == dist[p] and one.spans.dtype == np.int32
            assert np.array_equal(one.spans, spans[p, :n_spans[p]])
    assert got[-4].dist == 0 and got[-3].spans.tolist() == [[0, 1, 0, 1]] and got[-2].strings("", "ab") == [("", "ab")]
    assert hip.align([], []) == []


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_rater_merge_witnesses_is_rescore_on_host_built_edits(precision):
    """the same alignments as the numpy statement gives, hence the same edits, and every field of the result identical to
    `rescore` called by hand on them -- it is the same code path"""
    from tests.test_rater_golden import hip_factory
    hip = small_rater(hip_factory)
    texts, witnesses, contexts = witness_corpus(6)
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.25)
    alignments, rescored, skipped = hip.merge_witnesses(texts, witnesses, contexts, max_dist=5, join=1, precision=precision, **rescoring)
    pairs = [(i, w) for i, ws in enumerate(witnesses) for w in range(len(ws))]
    a, b = [texts[i] for i, _ in pairs], [witnesses[i][w] for i, w in pairs]
    dist, n_spans, spans = ratebulk.align_pairs_host(*codes(a), *codes(b), max(len(t) for t in a + b), 5, 1)
    flat = [ratebatch.Alignment(dist[p], spans[p, :n_spans[p]]) for p in range(len(pairs))]
    edits, ref_skipped = ratebatch.witness_edits(flat, pairs, texts, witnesses)
    assert [(one.dist, one.spans.tolist()) for per in alignments for one in per] == [(one.dist, one.spans.tolist()) for one in flat]
    assert skipped == ref_skipped and skipped["different"] == 1 and len(edits) > 5
    same_rescored(rescored, hip.rescore(texts, edits, contexts, precision=precision, **rescoring))
    assert sum(len(one) for one in rescored) == len(edits) and sum(int((one.best >= 0).sum()) for one in rescored) > 0
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()


def test_cli_witnesses_on_the_device(tmp_path):
    from ocrd_keraslm_amd.scripts import run
    from tests.test_rater_golden import hip_factory
    model = str(tmp_path / "model.h5")
    small_rater(hip_factory).save(model)
    rng = np.random.default_rng(26)
    other = tmp_path / "engine2"
    other.mkdir()
    files, texts, readings = [], [], []
    for i, size in enumerate((90, 70)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        readings.append([noisy(rng, texts[-1], 4)])
        name.write_text(texts[-1])
        (other / name.name).write_text(readings[-1][0])
        files.append(str(name))
    res = CliRunner().invoke(run.cli, ["witnesses", "-m", model, "--witness", str(other), "--apply", "-s", "4", "--max-dist", "8",
                                       "--left", "10", "--ahead", "2", "--min-gain", "0.25"] + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    ref = run._load(model)
    assert hasattr(ref.model, "align_pairs")
    alignments, found, _ = ref.merge_witnesses(texts, readings, [[170], [174]], max_dist=8, left=10, ahead=2, min_gain=0.25, streams=4)
    assert sum(len(f) for f in found) > 0
    for line, text, one, per in zip(lines, texts, found, alignments):
        assert type(one) is ratebatch.Rescored and line["chars"] == len(text) and line["corrected"] == one.apply(text)
        assert [w["dist"] for w in line["witnesses"]] == [al.dist for al in per] and per[0].dist > 0
        assert line["rescored"] == [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                                    for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
