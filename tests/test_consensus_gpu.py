"""Witness consensus on the GPU (run with -m gpu on an MI355X): kl_witness_clusters, kl_witness_pool, `HipLM.witness_clusters`,
`HipLM.witness_pool`, `Rater.consensus` and `keraslm-rate consensus`.

The kernels are held to their statements (`ratebulk.witness_clusters_host`, itself held to a brute force and four invariants in
test_consensus.py, and `ratebulk.witness_pool_host`) byte for byte: all outputs are integers.  The inputs are kl_align_pairs' own
device outputs on the same pairs.  Every output byte is FILL before a call, 64 elements behind each output and 64 bytes behind
the workspace must keep it.  The shapes are the smallest at which the kernels can go wrong: 1, 2, 63 and 64 witnesses on a
wave, texts without any, the least and the largest max_dist, clusters and candidates a lane less and more than a wave, a round
of the offsets' workgroup and a block, more texts than a grid has waves, texts of 4096 characters."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.test_consensus import (NAMES, cli_files, consensus_corpus, edge_cases, expected_lines, inputs_of, random_corpus, same_as_rescored,
                                  statement_edits, syms)
from tests.test_lexicon import pooled
from tests.test_rate_bulk_gpu import device, lib_and_stream, small_rater
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up
from tests.test_witnesses import edited

pytestmark = pytest.mark.gpu

GRID_WAVES = 1024 * 4      # waves of a launch at most: texts per sweep


def aligned_on_device(A, B, max_len, max_dist, join):
    """kl_align_pairs on the pairs (lists of symbols): (dist, n_spans, spans) as host arrays"""
    torch, dev = device()
    lib, stream = lib_and_stream()
    P = len(A)
    pools = pooled(A) + pooled(B)
    some = lambda a: up(a) if len(a) else torch.zeros(1, dtype=torch.int32, device=dev)
    src = [some(pools[0]), up(pools[1]), some(pools[2]), up(pools[3])]
    out = [torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
           torch.empty(P * max_dist * 4, dtype=torch.int32, device=dev)]
    ws = torch.empty(lib.kl_align_pairs_workspace_bytes(P, max_len, max_dist), dtype=torch.uint8, device=dev)
    code = lib.kl_align_pairs(ptr(src[0]), len(pools[0]), ptr(src[1]), ptr(src[2]), len(pools[2]), ptr(src[3]), P, max_len, max_dist, join,
                              ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), ws.numel(), stream)
    torch.cuda.synchronize()
    assert code == 0
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().reshape(P, max_dist, 4)


class Clusters(object):
    """kl_witness_clusters on device copies of the witnesses of some texts (lists of symbols) and on what kl_align_pairs left of
    their pairs on the device"""
    IN = ("b_pool", "b_off", "dist", "n_spans", "spans", "pair_first", "text_off")

    def __init__(self, texts, witnesses, max_dist, join=1, base=0):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        inputs = inputs_of(texts, witnesses, max_dist, join, align=aligned_on_device, base=base)
        self.host, self.join, self.max_dist = inputs[:7], join, max_dist
        self.P, self.n_texts = len(inputs[1]) - 1, len(texts)
        self.src = [up(a.reshape(-1)) if a.size else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev) for a in self.host]

    def replace(self, name, values):
        """other device data under `name`, for the call and for the statement"""
        at = self.IN.index(name)
        self.host[at] = np.ascontiguousarray(values)
        self.src[at] = up(self.host[at].reshape(-1))

    def want(self):
        return ratebulk.witness_clusters_host(*self.host, self.join)

    def run(self, ws_bytes=None, ws_fill=FILL, shift=None, **override):
        torch = self.torch
        R = self.P * self.max_dist
        i32, i64 = torch.int32, torch.int64
        self.out = [marked(n, kind) for n, kind in ((R, i32), (R, i64), (R, i32), (R + 1, i64), (R, i64), (R + 1, i64), (2 * R, i32), (8, i64))]
        max_dist = override.pop("max_dist", self.max_dist)
        self.n_ws = self.lib.kl_witness_clusters_workspace_bytes(self.P, min(max(max_dist, 1), 255), self.n_texts)
        self.ws = torch.full((self.n_ws + 64,), ws_fill, dtype=torch.uint8, device=self.dev)
        a = dict(zip(self.IN + NAMES, [ptr(t) for t in self.src + self.out]), n_b=len(self.host[0]), P=self.P, n_texts=self.n_texts,
                 join=self.join, ws=ptr(self.ws))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_witness_clusters(a["b_pool"], a["n_b"], a["b_off"], a["P"], max_dist, a["dist"], a["n_spans"], a["spans"],
                                            a["pair_first"], a["text_off"], a["n_texts"], a["join"], *[a[name] for name in NAMES],
                                            a["ws"], self.n_ws if ws_bytes is None else ws_bytes, self.stream)
        torch.cuda.synchronize()
        return code

    def is_statement(self, ws_fill=FILL):
        want = self.want()
        assert self.run(ws_fill=ws_fill) == 0
        for t, w, name in zip(self.out, want, NAMES):
            assert same_bytes(t, w, w.size), name
        assert (raw(self.ws)[self.n_ws:] == ws_fill).all()           # nothing behind the workspace
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def corpus(rng, n_texts, count, size=30, V=4, edits=4):
    texts = [rng.integers(0, V, int(rng.integers(0, size + 1))).tolist() for _ in range(n_texts)]
    witnesses = [[edited(rng, t, V, int(rng.integers(0, edits + 1))) for _ in range(count(i) if callable(count) else count)]
                 for i, t in enumerate(texts)]
    return texts, witnesses


def test_the_random_corpus_on_the_device():
    """four batches of the CPU test's corpus: the device's alignment is the statement's, and so are its clusters"""
    kept = multi = 0
    for texts, witnesses, inputs in random_corpus()[3::4]:
        look = Clusters(texts, witnesses, inputs[4].shape[1], inputs[7], base=int(inputs[6][0]))
        assert all(np.array_equal(g, w) for g, w in zip(look.host, inputs[:7]))
        want = look.is_statement()
        kept += int(want[7][0])
        multi += int((np.diff(want[3][:want[7][0] + 1]) >= 2).sum())
    assert kept > 400 and multi > 100


@pytest.mark.parametrize("count", [1, 2, 63, 64])
def test_witnesses_of_a_text_on_a_wave(count):
    """texts of 200 characters with `count` witnesses of up to two edits each, but two that have none: the lanes in use, and the
    last of them"""
    rng = np.random.default_rng(40 + count)
    texts = [[9] + rng.integers(0, 4, 200).tolist() for _ in range(7)]
    witnesses = [[[9] + edited(rng, t[1:], 4, int(rng.integers(0, 3))) for _ in range(0 if i in (2, 6) else count)] for i, t in enumerate(texts)]
    witnesses[4][count - 1] = texts[4][:100] + [7, 7] + texts[4][100:]      # the last lane holds a reading of its own
    look = Clusters(texts, witnesses, 5, join=0)
    want = look.is_statement()
    assert want[7][0] >= 4 and want[7][7] == 0 and (count == 1 or want[6].max() >= 2)
    assert any(look.host[0][want[4][c]:want[4][c] + 2].tolist() == [7, 7] for c in range(int(want[7][1])))


@pytest.mark.parametrize("max_dist", [1, 255])
def test_the_least_and_the_largest_max_dist(max_dist):
    rng = np.random.default_rng(max_dist)
    texts, witnesses = corpus(rng, 6, 3, size=300 if max_dist > 1 else 12, V=6, edits=min(max_dist, 90))
    texts += [[1], []]
    witnesses += [[[2], [1]], [[3]]]
    look = Clusters(texts, witnesses, max_dist)
    want = look.is_statement()
    assert (look.host[2] >= 0).sum() >= 8 and want[7][0] >= (2 if max_dist == 1 else 60)


def test_the_hand_made_edges_on_the_device():
    for name, texts, witnesses, max_dist, join in edge_cases():
        look = Clusters(texts, witnesses, max_dist, join, base=11)
        want = look.is_statement()
        assert want[7][7] == 0, name
    # 65 witnesses: the text is counted and nothing of it read, its neighbour is as before
    name, texts, witnesses, max_dist, join = edge_cases()[-1]
    look = Clusters(texts, [witnesses[0] + witnesses[0][:1], witnesses[1]], max_dist, join)
    want = look.is_statement()
    assert want[7].tolist()[:2] == [1, 3] and want[7][7] == 1
    for wrong in ([0, 68, 67], [0, -1, 68], [2, 65, 69]):            # pair ranges that descend, are negative, reach outside
        look.replace("pair_first", np.array(wrong, dtype=np.int64))
        assert look.is_statement()[7][7] >= 1


@pytest.mark.parametrize("n", [63, 65, 255, 257, 1023, 1025])
def test_clusters_and_candidates_around_waves_rounds_and_blocks(n):
    """n texts with a cluster and a candidate each, and -- up to 255 -- one text with n clusters of two candidates"""
    rng = np.random.default_rng(n)
    texts = [[5] + rng.integers(0, 4, 2).tolist() for _ in range(n)]
    witnesses = [[[t[0], t[1] + 4, t[2]]] for t in texts]
    witnesses[n - 1] = [[5, 9, 9, 9]]                                # the last cluster holds a reading of its own
    look = Clusters(texts, witnesses, 3)
    want = look.is_statement()
    assert want[7].tolist()[:3] == [n, n, n + 2] and want[4][n - 1] == 3 * (n - 1) + 1
    if n <= 255:
        text = rng.integers(0, 4, 3 * n + 1).tolist()
        one, two = list(text), list(text)
        for at in range(1, 3 * n, 3):
            one[at], two[at] = 4, 5
        look = Clusters([text], [[one, two, text]], n, join=0)
        want = look.is_statement()
        assert want[7].tolist()[:4] == [n, 2 * n, 2 * n, 1] and (want[6][:3 * n] == np.tile([2, 1, 1], n)).all()


def test_more_texts_than_a_grid():
    """4200 tiny texts, every fifth without a witness: more texts than the waves of one launch, offsets over seventeen rounds"""
    rng = np.random.default_rng(41)
    texts, witnesses = corpus(rng, GRID_WAVES + 104, lambda i: 0 if i % 5 == 4 else 1 + i % 2, size=6, V=3, edits=2)
    witnesses[-1] = [texts[-1] + [8]]
    texts[-1], witnesses[-1] = [1] + texts[-1], [[1] + w for w in witnesses[-1]]
    look = Clusters(texts, witnesses, 3)
    want = look.is_statement()
    S = int(want[7][0])
    assert S > 1000 and want[7][5] > 1000 and want[0][S - 1] == len(texts) - 1 and look.host[0][want[4][want[7][1] - 1]] == 8


def test_texts_of_4096_characters():
    rng = np.random.default_rng(42)
    texts = [rng.integers(0, 5, 4096).tolist() for _ in range(2)]
    witnesses = [[edited(rng, t, 5, 40)[:4096] for _ in range(3)] for t in texts]
    witnesses[1][2] = texts[1][:4095] + [9]                          # a difference in the last character
    look = Clusters(texts, witnesses, 64)
    want = look.is_statement()
    S = int(want[7][0])
    assert (look.host[2] >= 1).all() and S > 100 and want[1][S - 1] + want[2][S - 1] == 2 * 4096


def test_two_calls_give_the_same_bytes():
    rng = np.random.default_rng(43)
    texts, witnesses = corpus(rng, 200, lambda i: i % 5)
    look = Clusters(texts, witnesses, 4)
    look.is_statement()
    first = [raw(t).copy() for t in look.out]
    look.is_statement(ws_fill=0x3C)                                  # whatever the workspace held
    assert all(np.array_equal(x, raw(t)) for x, t in zip(first, look.out))


def test_garbage_in_the_spans_rejects_the_pair_and_no_more():
    """span fields outside their texts, slots that descend, span counts outside 0 .. max_dist and offsets that descend -- all
    on indices inside the allocated arrays, so that a missing check shows as a wrong output"""
    rng = np.random.default_rng(12)
    texts = [rng.integers(0, 3, 12).tolist() for _ in range(20)]
    witnesses = [[edited(rng, t, 3, 2), edited(rng, t, 3, 3)] for t in texts]
    look = Clusters(texts, witnesses, 4)
    clean = look.want()
    n_spans, spans = look.host[3].copy(), look.host[4].copy()
    assert (look.host[2][::2] >= 0).all() and (n_spans[:16:2] >= 1).all()
    n_spans[0:16:2] = [2, 2, 2, 2, 5, -1, 2, 2]
    spans[0, :2] = [[1, 2, 1, 2], [1, 3, 2, 3]]
    spans[2, :2] = [[1, 13, 1, 2], [-1, -1, -1, -1]]
    spans[4, :2] = [[1, 2, 1, 2], [3, 4, 1, 2]]
    spans[6, :2] = [[2, 3, 2, 1], [5, 5, 5, 5]]
    spans[12, :2] = [[1, 2, 1, 2], [3, 4, 3, 40]]
    spans[14, :2] = [[-2, 2, 1, 2], [3, 4, 3, 4]]
    look.replace("n_spans", n_spans)
    look.replace("spans", spans)
    want = look.is_statement()
    assert want[7][4] == clean[7][4] + 8
    off = look.host[1].copy()
    off[21] = off[22] + 1                                            # pair 20 reaches into pair 21, pair 21 descends
    look.replace("b_off", off)
    assert look.is_statement()[7][4] >= want[7][4] + 1
    text_off = look.host[6].copy()
    text_off[15] = text_off[14] - 3                                  # a text of a negative size: its witnesses cannot fit
    look.replace("text_off", text_off)
    assert look.is_statement()[7][4] >= want[7][4] + 1
    assert look.run(n_b=len(look.host[0]) - 5) == 0                  # the last witness reaches outside the pool now
    short = ratebulk.witness_clusters_host(look.host[0][:-5], *look.host[1:], look.join)
    assert all(same_bytes(t, w, w.size) for t, w in zip(look.out, short))


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(44)
    texts, witnesses = corpus(rng, 9, 2)
    look = Clusters(texts, witnesses, 4)
    size = look.lib.kl_witness_clusters_workspace_bytes
    assert size(0, 4, 9) == 0 and size(2 ** 31, 4, 9) == 0 and size(18, 0, 9) == 0 and size(18, 256, 9) == 0 and size(18, 4, 0) == 0
    assert size(18, 4, 2 ** 31) == 0 and size(18, 4, 9) >= 64 + 3 * 9 * 8 and size(18, 255, 9) == size(18, 1, 9)
    cases = [dict(P=0), dict(P=2 ** 31), dict(n_texts=0), dict(n_texts=2 ** 31), dict(n_b=2 ** 40 + 1), dict(max_dist=0), dict(max_dist=256),
             dict(max_dist=-1), dict(join=-1)]
    cases += [{name: None} for name in look.IN + NAMES + ("ws",)]
    cases += [dict(shift={name: 2}) for name in ("b_pool", "dist", "n_spans", "spans", "span_text", "span_len", "votes")]
    cases += [dict(shift={name: 4}) for name in ("b_off", "pair_first", "text_off", "span_start", "span_first", "cand_src", "cand_off", "stats")]
    for case in cases:
        assert look.run(**case) == KL_ERR_ARG, case
        assert look.untouched(), case
    assert look.run(ws_bytes=look.n_ws - 1) == KL_ERR_WORKSPACE and look.untouched()
    assert look.run(ws_bytes=0) == KL_ERR_WORKSPACE and look.untouched()
    assert look.run(shift=dict(ws=4)) == KL_ERR_WORKSPACE and look.untouched()
    look.is_statement()
    # the pool may be null when it holds nothing: two empty witnesses of an empty text agree with it
    empty = Clusters([[]], [[[], []]], 2)
    assert empty.run(b_pool=None, n_b=0) == 0
    assert all(same_bytes(t, w, w.size) for t, w in zip(empty.out, empty.want())) and empty.want()[7].tolist() == [0] * 8


def test_witness_pool_is_its_statement():
    torch, dev = device()
    lib, stream = lib_and_stream()
    rng = np.random.default_rng(45)
    for C, n_b in ((1, 10), (5, 30), (700, 3000)):
        b_ids = rng.integers(1, 50, n_b).astype(np.int32)
        off = np.concatenate([[0], np.cumsum(rng.integers(0 if C > 1 else 1, 9, C))]).astype(np.int64)
        src = rng.integers(0, n_b - 8, C).astype(np.int64)
        src[1::3] = [n_b - 3, -2, n_b + 5, -40][C % 4]               # some reach outside, or lie outside: 0 there
        n_pool = int(off[-1])
        tail = np.full(7, 123, dtype=np.int64)                       # (the arrays may be longer than C and C + 1)
        args = [up(b_ids), up(np.concatenate([src, tail])), up(np.concatenate([off, tail]))]
        want = ratebulk.witness_pool_host(b_ids, src, off, C, n_pool)

        def call(**wrong):
            pool = marked(n_pool, torch.int32)
            a = dict(b_ids=ptr(args[0]), n_b=n_b, src=ptr(args[1]), off=ptr(args[2]), C=C, pool=ptr(pool), n_pool=n_pool)
            for name, value in wrong.items():
                a[name] = shifted(a[name], value[0]) if isinstance(value, tuple) else value
            code = lib.kl_witness_pool(a["b_ids"], a["n_b"], a["src"], a["off"], a["C"], a["pool"], a["n_pool"], stream)
            torch.cuda.synchronize()
            return code, pool

        code, pool = call()
        assert code == 0 and same_bytes(pool, want, n_pool) and (C == 1 or ((want == 0).any() and (want > 0).any()))
        for wrong in (dict(C=0), dict(C=2 ** 40 + 1), dict(n_b=2 ** 40 + 1), dict(n_pool=2 ** 40 + 1), dict(b_ids=None), dict(src=None),
                      dict(off=None), dict(pool=None), dict(b_ids=(2,)), dict(src=(4,)), dict(off=(4,)), dict(pool=(2,))):
            code, pool = call(**wrong)
            assert code == KL_ERR_ARG and (raw(pool) == FILL).all(), wrong
    assert lib.kl_witness_pool(None, 0, ptr(args[1]), ptr(args[2]), 3, None, 0, stream) == 0      # nothing to write: no launch


# ---------------------------------------------------------------------------------------------- engine, Rater, command line
def test_engine_wrappers():
    from ocrd_keraslm_amd.lib import hipabi
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(46)
    texts, witnesses = corpus(rng, 12, lambda i: i % 4)
    pairs = [(i, k) for i, ws in enumerate(witnesses) for k in range(len(ws))]
    a_side, b_side = pooled([texts[i] for i, _ in pairs]), pooled([witnesses[i][k] for i, k in pairs])
    pair_first = np.concatenate([[0], np.cumsum([len(ws) for ws in witnesses])]).astype(np.int64)
    text_off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    on_device = [up(x) for x in a_side + b_side]
    aligned = lm.align_pairs(*on_device, 40, 5, 1)
    want = ratebulk.witness_clusters_host(*b_side, *[t.cpu().numpy() for t in aligned], pair_first, text_off, 1)
    args = on_device[2:] + list(aligned) + [up(pair_first), up(text_off), 1]
    got = lm.witness_clusters(*args)
    R = len(pairs) * 5
    assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32, torch.int64, torch.int32, torch.int64, torch.int64,
                                                                      torch.int64, torch.int32, torch.int64]
    assert [tuple(t.shape) for t in got] == [(R,), (R,), (R,), (R + 1,), (R,), (R + 1,), (2 * R,), (8,)]
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    S, C, n_pool = (int(x) for x in want[7][:3])
    assert S > 5 and C >= S
    b_ids = (b_side[0] + 3).astype(np.int32)
    pool = lm.witness_pool(up(b_ids), got[4], got[5], C, n_pool)
    assert pool.is_cuda and pool.dtype == torch.int32 and np.array_equal(pool.cpu().numpy(), ratebulk.witness_pool_host(b_ids, want[4], want[5], C, n_pool))
    assert lm.witness_pool(up(b_ids), got[4], got[5], 1, 0).numel() == 0
    names = ("b_pool", "b_off", "dist", "n_spans", "spans", "pair_first", "text_off", "join")
    for wrong in (dict(b_pool=args[0].long()), dict(b_off=args[1].int()), dict(b_off=args[1][:-1]), dict(dist=args[2][:-1]),
                  dict(n_spans=args[3].long()), dict(spans=args[4].reshape(-1)), dict(spans=args[4][:, :, :3]), dict(pair_first=args[5].int()),
                  dict(text_off=args[6][:-1]), dict(pair_first=torch.from_numpy(pair_first)), dict(join=-1)):
        a = dict(dict(zip(names, args)), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.witness_clusters(*[a[name] for name in names])
    for wrong in (dict(C=0), dict(C=R + 1), dict(n_pool=-1), dict(b_ids=up(b_ids).long()), dict(cand_src=got[4].int())):
        a = dict(dict(b_ids=up(b_ids), cand_src=got[4], cand_off=got[5], C=C, n_pool=n_pool), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.witness_pool(a["b_ids"], a["cand_src"], a["cand_off"], a["C"], a["n_pool"])


RESCORING = dict(streams=16, left=12, ahead=3, min_gain=0.25)


def test_rater_consensus_with_one_witness_is_merge_witnesses_on_the_device():
    """the rows and the chunks of the two calls are the same, and two `rescore` calls on the same edits agree exactly (asserted
    here first): spans, candidates, best, gain and costs are held exactly"""
    from tests.test_rater_golden import hip_factory
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "witness_clusters")
    texts, witnesses, contexts = consensus_corpus(6, 1)
    texts += ["x été", "modern times", "a\U0001F600xb"]
    witnesses += [["x ete"], ["modem times"], ["a\U0001F601xb"]]
    contexts += [[180], [181], [182]]
    for precision in ("bf16", "split"):
        alignments, rescored, skipped = hip.merge_witnesses(texts, witnesses, contexts, max_dist=5, join=1, precision=precision, **RESCORING)
        again = hip.merge_witnesses(texts, witnesses, contexts, max_dist=5, join=1, precision=precision, **RESCORING)[1]
        for one, ref in zip(again, rescored):
            assert np.array_equal(one.cost0, ref.cost0) and np.array_equal(one.cost, ref.cost)
        found, dists, counts = hip.consensus(texts, witnesses, contexts, max_dist=5, join=1, precision=precision, **RESCORING)
        same_as_rescored(found, rescored)
        assert counts == skipped and sum(len(one) for one in found) > 8
        assert [d.tolist() for d in dists] == [[one.dist for one in per] for per in alignments]
    assert found[-1].candidates == ["\U0001F601"] and found[-3].candidates == ["ete"]


def from_alignments(rater):
    """`Rater.align`'s `Alignment`s as the arrays kl_align_pairs leaves: the host chain's first step"""
    def align(A, B, max_len, max_dist, join):
        flat = rater.align(["".join(chr(x) for x in a) for a in A], ["".join(chr(x) for x in b) for b in B], max_dist=max_dist, join=join)
        spans = np.full((len(A), max_dist, 4), -1, dtype=np.int32)
        for p, one in enumerate(flat):
            spans[p, :len(one)] = one.spans
        return (np.array([one.dist for one in flat], dtype=np.int32), np.array([len(one) for one in flat], dtype=np.int32), spans)
    return align


def test_rater_consensus_with_three_witnesses_is_the_host_chain_on_the_device():
    """the host chain: `align`, its `Alignment` objects, `witness_clusters_host`, `rescore`.  The same choices, the same votes,
    and -- the rows being the same and two `rescore` calls agreeing exactly -- the same costs"""
    from tests.test_rater_golden import hip_factory
    hip = small_rater(hip_factory)
    for count in (3, None):
        texts, witnesses, contexts = consensus_corpus(7, count)
        edits, votes0, votes, dist, skipped = statement_edits(texts, witnesses, 6, 1, align=from_alignments(hip))
        assert len(edits) > 8
        want = hip.rescore(texts, edits, contexts, **RESCORING)
        again = hip.rescore(texts, edits, contexts, **RESCORING)
        for one, ref in zip(again, want):
            assert np.array_equal(one.cost0, ref.cost0) and np.array_equal(one.cost, ref.cost)
        found, dists, counts = hip.consensus(texts, witnesses, contexts, max_dist=6, join=1, **RESCORING)
        same_as_rescored(found, want)
        assert counts == skipped and np.concatenate(dists).tolist() == dist.tolist()
        assert np.concatenate([one.votes0 for one in found]).tolist() == votes0
        assert np.concatenate([one.votes for one in found]).tolist() == votes
    voted = hip.consensus(texts, witnesses, contexts, max_dist=6, join=1, vote_bits=1.5, **RESCORING)[0]
    for one, ref in zip(voted, found):
        assert np.array_equal(one.cost0, ref.cost0 - 1.5 * ref.votes0) and np.array_equal(one.cost, ref.cost - 1.5 * ref.votes)
    bare = hip.consensus(texts, witnesses, contexts, max_dist=6, join=1, want_costs=False, **RESCORING)[0]
    same_as_rescored(bare, want, costs=False)
    none = hip.consensus(["abcdef", "abcdef"], [["abcdef"], ["xbcdef", "hgfhgfhgf"]], max_dist=3)
    assert [len(one) for one in none[0]] == [0, 0] and none[2] == dict(different=1, first=1, long=0)


def test_cli_consensus_on_the_device(tmp_path):
    from ocrd_keraslm_amd.scripts import run
    from tests.test_rater_golden import hip_factory
    model = str(tmp_path / "model.h5")
    small_rater(hip_factory).save(model)
    dirs, files, texts, readings = cli_files(tmp_path, np.random.default_rng(9))
    witness = [x for d in dirs for x in ("--witness", str(d))]
    res = CliRunner().invoke(run.cli, ["consensus", "-m", model, "--max-dist", "8", "--vote-bits", "0.5", "--min-gain", "0.25", "--apply"]
                             + witness + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    ref = run._load(model)
    assert hasattr(ref.model, "witness_clusters")
    found, dists, skipped = ref.consensus(texts, readings, [[170], [174], [178]], max_dist=8, vote_bits=0.5, min_gain=0.25)
    sources = [[str(d / name.rsplit("/", 1)[1]) for d in (dirs if i != 1 else dirs[1:2])] for i, name in enumerate(files)]
    assert [json.loads(l) for l in res.stdout.strip().split("\n")] == expected_lines(files, texts, found, dists, sources)
    assert json.loads(res.stderr.strip().split("\n")[-1]) == skipped and sum(len(one) for one in found) > 3
