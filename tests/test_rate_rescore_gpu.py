"""Rescoring caller-supplied replacements on the GPU (run with -m gpu on an MI355X): kl_span_windows, kl_span_pick,
`HipLM.span_windows`, `HipLM.span_pick` and `Rater.rescore`.

kl_span_windows and kl_span_pick are held to their numpy statements (`ratebulk.span_windows_host`, `ratebulk.span_pick_host`,
themselves held to brute force in test_rate_rescore.py) bit for bit, with a guard band behind every output, and -- for spans of
one character with uniform candidates -- to kl_edit_windows.  `Rater.rescore(precision="bf16")` is held, bit for bit, to
`lm.rate_window_bulk` on the host statement's windows, uploaded in the same chunks from zero states, and to
`Rater.corrections`; `precision="split"` to the CPU double within the first-order bound of the project's 2e-5 on a
split-precision probability: |cost - cost_oracle| <= 2 * sum over the scored positions of 2e-5 / (p_oracle * ln 2)."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk
from tests.test_rate_bulk_gpu import device, lib_and_stream
from tests.test_rate_corrections import variant_corpus, wide_rater, wide_texts
from tests.test_rate_corrections_gpu import KL_ERR_ARG, suspects_for
from tests.test_rate_rescore import (NAMES, RESCORE_SPLIT, check_rescored, corrections_as_edits, decided_spans, edit_arrays,
                                     flat_costs, oracle_span_costs, pack, pick_cases, random_edits, span_cases, span_corpus, wide_edits)
from tests.test_rate_suspects_gpu import GUARD, MARK, marked, words
from tests.test_rate_window_gpu import ptr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 0, 1, 3), (37, 3, 5, 4, 2, 10), (300, 8, 40, 7, 5, 64)]      # (S, candidates at most, left, ahead, M, T)
SPAN_NAMES = ("span_text", "span_start", "span_len", "span_first", "pool", "cand_off")


class Spans(object):
    """kl_span_windows on device copies of host arrays; every output is followed by a guard band and prefilled with the marker"""

    def __init__(self, corpus, offsets, text_ctx, arrays, T, rows=None):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        torch = self.torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
        self.src = dict(corpus=up(corpus), offsets=up(offsets), text_ctx=up(text_ctx) if self.n_ctx else None)
        # (an empty pool still has an address: one id that no candidate names)
        self.src.update((name, up(arrays[name] if len(arrays[name]) else np.zeros(1, dtype=arrays[name].dtype))) for name in SPAN_NAMES)
        self.n_corpus, self.n_texts, self.T = len(corpus), len(offsets) - 1, T
        self.S, self.C, self.n_pool = len(arrays["span_text"]), len(arrays["cand_off"]) - 1, len(arrays["pool"])
        self.N = self.S + self.C
        self.rows = self.N if rows is None else rows
        self.sizes = dict(idx=self.rows * T, ctx=self.rows * T * self.n_ctx, tgt=self.rows * T, valid=self.rows)
        self.fresh()

    def fresh(self):
        self.out = dict((name, marked(self.torch, self.dev, n, self.torch.int32)) for name, n in self.sizes.items())

    def run(self, left, ahead, max_len, shift=None, **override):
        a = dict((name, ptr(t) if t is not None else None) for name, t in self.src.items())
        a.update((name, ptr(t)) for name, t in self.out.items())
        if not self.n_ctx:
            a["ctx"] = None
        a.update(n_corpus=self.n_corpus, n_texts=self.n_texts, n_ctx=self.n_ctx, S=self.S, n_pool=self.n_pool, C=self.C, row0=0,
                 rows=self.rows, left=left, ahead=ahead, max_len=max_len, T=self.T)
        a.update(override)
        for name, by in (shift or {}).items():      # (a misaligned pointer)
            a[name] = C.c_void_p(a[name].value + by)
        code = self.lib.kl_span_windows(a["corpus"], a["n_corpus"], a["offsets"], a["n_texts"], a["text_ctx"], a["n_ctx"],
                                        a["span_text"], a["span_start"], a["span_len"], a["span_first"], a["S"], a["pool"],
                                        a["n_pool"], a["cand_off"], a["C"], a["row0"], a["rows"], a["left"], a["ahead"],
                                        a["max_len"], a["T"], a["idx"], a["ctx"], a["tgt"], a["valid"], self.stream)
        self.torch.cuda.synchronize()
        return code

    def results(self):
        return dict((name, words(t)) for name, t in self.out.items())

    def untouched(self):
        return all((w == MARK).all() for w in self.results().values())


def held_to(got, want):
    """every word of every output is the statement's -- no marker is left --, and nothing behind it is touched"""
    for name, ref in want.items():
        ref = np.ascontiguousarray(ref).reshape(-1).view(np.uint32)
        assert got[name].size == ref.size + GUARD
        assert np.array_equal(got[name][:ref.size], ref), name
        assert (got[name][ref.size:] == MARK).all(), name


def twice_equal_to(v, want, *args, **kw):
    runs = []
    for _ in range(2):
        v.fresh()
        assert v.run(*args, **kw) == 0
        runs.append(v.results())
        held_to(runs[-1], want)
    assert all(np.array_equal(runs[0][name], runs[1][name]) for name in want)


# ---------------------------------------------------------------------------------------------- kl_span_windows
@pytest.mark.parametrize("n_ctx", [0, 2, 3])
@pytest.mark.parametrize("S,most,left,ahead,M,T", SHAPES)
def test_span_windows_is_span_windows_host(S, most, left, ahead, M, T, n_ctx):
    corpus, offsets, text_ctx = span_corpus(n_ctx)
    spans = span_cases(corpus, offsets, left, ahead, M, S=S, max_cands=most)
    a = pack(spans)
    assert len(spans) == S and np.diff(a["span_first"]).max() <= most
    N = S + len(a["cand_off"]) - 1
    host = lambda ids, row0, rows: dict(zip(NAMES, ratebulk.span_windows_host(
        ids, offsets, text_ctx, row0=row0, rows=rows, left=left, ahead=ahead, max_len=M, T=T, **a)))
    want = host(corpus, 0, N)
    assert want["valid"].any() and (S == 1 or not want["valid"].all())
    if T == left + ahead + M - 1 and S > 1:      # a fed row that fills the whole row
        assert (want["tgt"][:, T - 1] >= 0).any()
    twice_equal_to(Spans(corpus, offsets, text_ctx, a, T), want, left, ahead, M)
    # the row space in two chunks, the second beginning inside a span
    row0 = 1 if S == 1 else 2
    assert a["span_first"][1] + 1 > row0
    twice_equal_to(Spans(corpus, offsets, text_ctx, a, T, rows=row0), host(corpus, 0, row0), left, ahead, M)
    twice_equal_to(Spans(corpus, offsets, text_ctx, a, T, rows=N - row0), host(corpus, row0, N - row0), left, ahead, M, row0=row0)
    if S > 1:      # a corpus that ends in front of offsets[n_texts]: spans beyond n_read, positions that read as 0
        short = len(corpus) - 5
        assert short < offsets[-1]
        cut = host(corpus[:short], 0, N)
        assert not np.array_equal(cut["valid"], want["valid"])
        twice_equal_to(Spans(corpus, offsets, text_ctx, a, T), cut, left, ahead, M, n_corpus=short)


@pytest.mark.parametrize("n_ctx", [0, 2])
def test_span_windows_longest_hypothesis(n_ctx):
    """one text of 1100 ids, a span of one id at position 1000 and a candidate of 64 ids, left = 959, ahead = 2, M = 64,
    T = 1024 = left + ahead + M - 1: a hypothesis of 959 + 64 + 2 = T + 1 ids, the longest the staging array has to hold
    (left = 960 would need T = 1025, which the entry point rejects)"""
    rng = np.random.default_rng(78)
    corpus = rng.integers(1, 200, 1100).astype(np.int32)
    offsets = np.array([0, 1100], dtype=np.int64)
    text_ctx = rng.integers(1, 200, (1, n_ctx)).astype(np.int32) if n_ctx else None
    left, ahead, M, T = 959, 2, 64, 1024
    long_ = [int(v) for v in rng.integers(1, 200, 64)]
    spans = [(0, 1000, 1, [long_, [7]]), (0, 1097, 64, [long_[::-1]]), (0, 300, 0, [long_])]
    a = pack(spans)
    N = len(spans) + 4
    want = dict(zip(NAMES, ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=0, rows=N, left=left, ahead=ahead,
                                                      max_len=M, T=T, **a)))
    assert want["valid"].tolist() == [1, 1, 1, 0, 0, 1, 1]
    assert want["tgt"][1, T - 1] >= 0 and want["tgt"][0, T - 1] == -1 and want["idx"][1, left:left + 64].tolist() == long_
    v = Spans(corpus, offsets, text_ctx, a, T)
    twice_equal_to(v, want, left, ahead, M)
    v.fresh()
    assert v.run(960, ahead, M) == KL_ERR_ARG and v.untouched()


@pytest.mark.parametrize("S,K,left,ahead,T", [(37, 3, 5, 4, 10), (300, 8, 40, 7, 64)])
def test_span_windows_of_one_character_are_edit_windows(S, K, left, ahead, T):
    """every suspect of `variant_suspects` -- positions outside the corpus and alternatives of -1 included -- as a span of one
    character with the 2K + 1 candidates [a_0] .. [a_K-1], [], [a_0, w] .. [a_K-1, w]"""
    from tests.test_rate_insertions_gpu import Edits
    n_ctx = 2
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = suspects_for(corpus, offsets, S, K)
    assert (alts < 0).any() and (pos < 0).any() and (pos >= len(corpus)).any()
    R = 2 * K + 2
    old = Edits(corpus, offsets, text_ctx, pos, alts, T, R)
    assert old.run(left, ahead, 1) == 0
    inside = (pos >= 0) & (pos < len(corpus))
    w = np.where(inside, corpus[np.where(inside, pos, 0)], 0)
    text = np.clip(np.searchsorted(offsets, pos, side="right") - 1, 0, len(offsets) - 2)
    spans = [(int(text[s]), int(pos[s]), 1, [[int(a)] for a in alts[s]] + [[]] + [[int(a), int(w[s])] for a in alts[s]])
             for s in range(S)]
    new = Spans(corpus, offsets, text_ctx, pack(spans), T)
    assert new.N == S * R and new.run(left, ahead, 2) == 0
    a, b = old.results(), new.results()
    assert not old.untouched() and a["valid"][:S * R].any() and not a["valid"][:S * R].all()
    assert all(np.array_equal(a[name], b[name]) for name in NAMES)


def test_span_windows_argument_errors():
    """KL_ERR_ARG before any launch: the outputs keep their markers"""
    S, left, ahead, M, T, n_ctx = 37, 5, 4, 2, 10, 2
    corpus, offsets, text_ctx = span_corpus(n_ctx)
    v = Spans(corpus, offsets, text_ctx, pack(span_cases(corpus, offsets, left, ahead, M, S=S)), T)
    names = ("corpus", "offsets", "text_ctx", "idx", "ctx", "tgt", "valid") + SPAN_NAMES
    cases = [{name: None} for name in names]      # (text_ctx and ctx: null while n_ctx > 0; pool: null while n_pool > 0)
    cases += [dict(S=0), dict(n_texts=0), dict(rows=0), dict(rows=-1), dict(row0=-1), dict(row0=1), dict(rows=v.N + 1),
              dict(C=v.C - 1), dict(C=-1), dict(left=0), dict(ahead=-1), dict(T=left + ahead + M - 2), dict(T=1025),
              dict(max_len=0), dict(max_len=65), dict(max_len=M + 1), dict(n_ctx=-1), dict(n_ctx=9),
              dict(rows=2 ** 22 + 1, C=2 ** 23), dict(n_corpus=2 ** 40 + 1)]
    long_names = ("offsets", "span_start", "span_first", "cand_off")
    cases += [dict(shift={name: 4 if name in long_names else 2}) for name in names]
    for case in cases:
        assert v.run(**dict(dict(left=left, ahead=ahead, max_len=M), **case)) == KL_ERR_ARG, case
        assert v.untouched(), case
    assert v.run(left, ahead, M) == 0 and not v.untouched()
    # spans without a single candidate: no pool to name
    bare = Spans(corpus, offsets, text_ctx, pack([(7, int(offsets[7]) + 9, 1, []), (7, int(offsets[7]) + 12, 2, [])]), T)
    assert bare.C == 0 and bare.run(left, ahead, M, pool=None) == 0
    assert bare.results()["valid"][:2].tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------- kl_span_pick
def run_pick(cost, valid, first, min_gain, want_costs=True):
    torch, dev = device()
    lib, stream = lib_and_stream()
    S, N = len(first) - 1, len(cost)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    src = (up(cost), up(valid), up(first))
    best = marked(torch, dev, S, torch.int32)
    gain = marked(torch, dev, 2 * S, torch.int32)
    out = marked(torch, dev, 2 * N, torch.int32)
    code = lib.kl_span_pick(ptr(src[0]), ptr(src[1]), ptr(src[2]), S, N - S, float(min_gain), ptr(best), ptr(gain),
                            ptr(out) if want_costs else None, stream)
    torch.cuda.synchronize()
    return code, dict(best=words(best), gain=words(gain), cost=words(out))


def test_span_pick_is_span_pick_host():
    cost, valid, first = pick_cases()
    assert np.diff(first).max() == 300
    one = (np.array([5.0, 3.0, 3.0]), np.array([1, 1, 1], dtype=np.int32), np.array([0, 2], dtype=np.int64))
    with np.errstate(invalid="ignore"):
        for case in ((cost, valid, first), one):
            for min_gain in (-np.inf, 0.0, 1.0, np.inf, np.nan):
                best, gain, out = ratebulk.span_pick_host(*case, min_gain=min_gain)
                assert min_gain != -np.inf or (best >= 0).any()
                runs = []
                for _ in range(2):
                    code, got = run_pick(*case, min_gain=min_gain)
                    assert code == 0
                    held_to(got, dict(best=best, gain=gain, cost=out))
                    runs.append(got)
                assert all(np.array_equal(runs[0][name], runs[1][name]) for name in runs[0])
            code, got = run_pick(*case, min_gain=0.0, want_costs=False)
            best, gain, _ = ratebulk.span_pick_host(*case, min_gain=0.0)
            assert code == 0 and (got["cost"] == MARK).all()
            held_to(dict(best=got["best"], gain=got["gain"]), dict(best=best, gain=gain))


def test_span_pick_argument_errors():
    torch, dev = device()
    lib, stream = lib_and_stream()
    cost, valid, first = pick_cases()
    S, N = len(first) - 1, len(cost)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(cost=up(cost), valid=up(valid), span_first=up(first))
    out = dict(best=marked(torch, dev, S, torch.int32), gain=marked(torch, dev, 2 * S, torch.int32),
               cost_out=marked(torch, dev, 2 * N, torch.int32))
    t.update(out)

    def run(shift=None, **override):
        a = dict((name, ptr(x)) for name, x in t.items())
        a.update(S=S, C=N - S)
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = C.c_void_p(a[name].value + by)
        code = lib.kl_span_pick(a["cost"], a["valid"], a["span_first"], a["S"], a["C"], 0.0, a["best"], a["gain"], a["cost_out"],
                                stream)
        torch.cuda.synchronize()
        return code

    cases = [{name: None} for name in ("cost", "valid", "span_first", "best", "gain")] + [dict(S=0), dict(C=-1)]
    cases += [dict(shift={name: 2 if name in ("valid", "best") else 4}) for name in t]
    for case in cases:
        assert run(**case) == KL_ERR_ARG, case
        assert all((words(x) == MARK).all() for x in out.values()), case
    assert run() == 0 and not any((words(x) == MARK).all() for x in out.values())


# ---------------------------------------------------------------------------------------------- the engine's wrappers
def test_engine_span_windows_and_span_pick():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rate_window_gpu import make_model
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 2)
    S, left, ahead, M, T = 37, 5, 4, 2, 12
    corpus, offsets, text_ctx = span_corpus(2)
    a = pack(span_cases(corpus, offsets, left, ahead, M, S=S))
    N = S + len(a["cand_off"]) - 1
    up = lambda x: torch.from_numpy(x).to(dev)
    where, spans = [up(corpus), up(offsets), up(text_ctx)], [up(a[name]) for name in SPAN_NAMES]
    args = dict(left=left, ahead=ahead, max_len=M, T=T)
    want = ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=0, rows=N, **dict(a, **args))
    got = lm.span_windows(*(where + spans), row0=0, rows=N, **args)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
    for g, r in zip(got, want):
        assert tuple(g.shape) == r.shape and np.array_equal(g.cpu().numpy(), r)
    # a chunk of the row space, as `Rater.rescore` takes it; no contexts
    part = lm.span_windows(where[0], where[1], None, *spans, row0=7, rows=20, **args)
    assert tuple(part[1].shape) == (20, T, 0)
    for g, r in zip((part[0], part[2], part[3]), (want[0], want[2], want[3])):
        assert np.array_equal(g.cpu().numpy(), r[7:27])
    # spans without candidates: an empty pool
    none = pack([(7, int(offsets[7]) + 9, 1, []), (7, int(offsets[7]) + 12, 2, [])])
    bare = lm.span_windows(*(where + [up(none[name]) for name in SPAN_NAMES]), row0=0, rows=2, **args)
    assert bare[3].cpu().numpy().tolist() == [1, 1]
    for bad in (dict(spans=[spans[0].to(torch.int64)] + spans[1:]), dict(spans=spans[:1] + [spans[1].to(torch.int32)] + spans[2:]),
                dict(spans=spans[:3] + [spans[3][:-1]] + spans[4:]), dict(spans=spans[:4] + [spans[4].cpu()] + spans[5:]),
                dict(where=[where[0], where[1], where[2][:-1]]), dict(T=left + ahead + M - 2), dict(rows=0), dict(rows=N + 1),
                dict(row0=-1), dict(max_len=65), dict(left=0)):
        call = dict(dict(where=where, spans=spans, row0=0, rows=N), **args)
        call.update(bad)
        with pytest.raises(hipabi.KlError):
            lm.span_windows(*(call.pop("where") + call.pop("spans")), **call)
    # span_pick
    cost, valid, first = pick_cases()
    with np.errstate(invalid="ignore"):
        for min_gain in (-np.inf, 1.0):
            best, gain, out = ratebulk.span_pick_host(cost, valid, first, min_gain)
            got = lm.span_pick(up(cost), up(valid), up(first), min_gain)
            assert [t.dtype for t in got] == [torch.int32, torch.float64, torch.float64] and all(t.is_cuda for t in got)
            assert np.array_equal(got[0].cpu().numpy(), best)
            assert np.array_equal(got[1].cpu().numpy().view(np.uint64), gain.view(np.uint64))
            assert np.array_equal(got[2].cpu().numpy().view(np.uint64), out.view(np.uint64))
        bare = lm.span_pick(up(cost), up(valid), up(first), 1.0, want_costs=False)
        assert bare[2] is None and np.array_equal(bare[0].cpu().numpy(), best)
    for bad in ((up(cost.astype(np.float32)), up(valid), up(first)), (up(cost), up(valid.astype(np.int64)), up(first)),
                (up(cost), up(valid), up(first.astype(np.int32))), (up(cost)[:-1], up(valid), up(first)),
                (up(cost)[:3], up(valid)[:3], up(first)), (up(cost), up(valid), up(first)[:1]), (cost, up(valid), up(first))):
        with pytest.raises((hipabi.KlError, AttributeError)):
            lm.span_pick(*bad, min_gain=0.0)


# ---------------------------------------------------------------------------------------------- Rater
def test_rescore_bf16_is_rate_window_bulk_on_the_host_windows():
    """first all rows in one chunk of more than 512 rows, then chunks of at most 24 rows with spans of their own"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    texts = texts + [texts[4][::-1], texts[6][::-1], texts[3][::-1] + texts[4]]
    contexts = contexts + [[175], [190], [180]]
    hip = wide_rater(hip_factory)
    lm = hip.model
    assert hasattr(lm, "span_windows") and lm.pwidth == 512
    left, ahead = 6, 3
    edits = random_edits(texts, seed=32, per_text=20, deep=left + 5)
    corpus, offsets, text_ctx, a, M = edit_arrays(hip, texts, contexts, edits)
    S, N = len(edits), len(edits) + len(a["cand_off"]) - 1
    T = max(left + ahead + M - 1, ratebulk.MIN_T)
    hip.model.reset_states(1)
    before = np.asarray(hip.rate(texts[4], contexts[4]), dtype=np.float64)
    for streams, min_gain in ((1024, 0.5), (4, -np.inf)):
        found = hip.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=min_gain, precision="bf16")
        assert lm.states.shape[0] == 1 and not lm.states.cpu().numpy().any()
        kept = check_rescored(found, texts, edits, min_gain)
        chunks = ratebulk.span_chunks(a["span_first"], streams)
        assert (N > 512 and chunks == [(0, N)]) if streams == 1024 else (max(b - a_ for a_, b in chunks) > streams)
        cost, valid = [], []
        for row0, row1 in chunks:
            x, z, y, ok = ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=row0, rows=row1 - row0, left=left, ahead=ahead,
                                                     max_len=M, T=T, **a)
            lm.reset_states(len(x))
            lm.rate_bits_read(reset=True)
            lm.rate_window_bulk(x, z, y, want_probs=False)
            cost.append(lm.rate_bits_read(reset=True))
            valid.append(ok)
        cost, valid = np.concatenate(cost), np.concatenate(valid)
        assert (cost[valid == 0] == 0.0).all() and (cost[valid == 1] > 0.0).all()      # (a dummy stream takes no bits)
        best, gain, cost = ratebulk.span_pick_host(cost, valid, a["span_first"], min_gain)
        assert np.array_equal(flat_costs(found, edits).view(np.uint64), cost.view(np.uint64))
        assert kept == (best >= 0).sum() > 0 and (best == -1).any()
        bare = hip.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=min_gain, want_costs=False)
        for full, b in zip(found, bare):
            assert b.cost is None and b.cost0 is None
            assert np.array_equal(full.best, b.best) and np.array_equal(full.gain.view(np.uint64), b.gain.view(np.uint64))
        lm.reset_states(1)
    # afterwards: a split-precision rate as before the bulk calls
    after = np.asarray(hip.rate(texts[4], contexts[4]), dtype=np.float64)
    assert np.abs(after - before).max() < 1e-6
    # no edits; only spans that cannot hold a prediction
    for some, few in ((texts, []), (["", "a", "abc"], [(1, 0, 1, ["b"]), (2, 0, 2, ["h", ""])])):
        found = hip.rescore(some, few, want_costs=True)
        check_rescored(found, some, few, 1.0)
        assert all((f.best == -1).all() and np.isinf(f.cost0).all() and np.isinf(f.cost).all() for f in found)


def test_rescore_bf16_equals_corrections():
    """every predicted character a suspect, written as a span of one character with the k substitutions, "" and the k strings
    alternative + written: the costs of `corrections(deletions=True, insertions=True)` at the same `streams`, bit for bit"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    hip = wide_rater(hip_factory)
    k, left, ahead = 3, 6, 3
    for streams in (1024, 64):
        want, _ = hip.corrections(texts, contexts, k=k, streams=streams, max_prob=1.0, min_rank=0, left=left, ahead=ahead,
                                  deletions=True, insertions=True, min_gain=-np.inf, precision="bf16")
        edits = corrections_as_edits(hip, texts, want)
        assert len(edits) == sum(max(len(t) - 1, 0) for t in texts)
        found = hip.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=-np.inf, precision="bf16")
        for one, cor in zip(found, want):
            cost = np.concatenate([one.cost0[:, None], one.cost.reshape(len(one), 2 * k + 1)], axis=1)
            assert np.array_equal(cost.view(np.uint64), cor.cost.view(np.uint64))
            _, best, gain = ratebulk.variant_pick_host(cor.cost, np.isfinite(cor.cost))
            assert np.array_equal(one.best, best - 1) and np.array_equal(one.gain.view(np.uint64), gain.view(np.uint64))


def test_rescore_split_against_the_double():
    """the texts, edits and settings test_rescore_split_contract_edits_keep_the_oracle_within_the_share checks on the CPU: every
    cost within the first-order bound of the double's, the +inf pattern the double's, and the same candidate chosen wherever the
    double's margin exceeds the two rows' bounds.
    Measured on an MI355X: 52 spans, 18 with a valid candidate, 2 too close to call, largest |cost - cost_oracle| 0.0059 of its
    bound."""
    from ocrd_keraslm_amd.lib import hipabi
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    oracle = wide_rater(OracleLM)
    hip = wide_rater(hip_factory)
    edits = wide_edits(texts)
    found = hip.rescore(texts, edits, contexts, precision="split", **RESCORE_SPLIT)
    assert hip.model.precision == hipabi.KL_PREC_SPLIT and hip.model.states.shape[0] == 1
    check_rescored(found, texts, edits, RESCORE_SPLIT["min_gain"])
    cost, bound, first = oracle_span_costs(oracle, texts, contexts, edits, RESCORE_SPLIT["left"], RESCORE_SPLIT["ahead"])
    got = flat_costs(found, edits)
    assert np.array_equal(np.isinf(got), np.isinf(cost))
    fin = np.isfinite(cost)
    ratio = np.abs(got[fin] - cost[fin]) / bound[fin]
    has, best, sure = decided_spans(cost, bound, first)
    taken = [0] * len(found)
    chosen = []
    for i, _, _, _ in edits:
        chosen.append(int(found[i].best[taken[i]]))
        taken[i] += 1
    chosen = np.array(chosen)
    print("spans %d, with a valid candidate %d, too close to call %d, max |cost - cost_oracle| / bound = %.3g"
          % (len(edits), has.sum(), (has & ~sure).sum(), ratio.max()))
    assert has.sum() >= 15 and (has & ~sure).sum() <= 0.25 * has.sum()
    assert ratio.max() <= 1.0, ratio.max()
    assert np.array_equal(chosen[has & sure], best[has & sure]) and (chosen[~has] == -1).all()
