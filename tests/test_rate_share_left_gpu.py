"""A suspect's left context read once for all its variants, on the GPU (run with -m gpu on an MI355X): kl_prefix_windows,
kl_state_fanout, `HipLM.prefix_windows`, `HipLM.fan_states` and `Rater.corrections(share_left=True)`.

The two entry points are held to their numpy statements (`ratebulk.prefix_windows_host`, `ratebulk.fan_states_host`, themselves
held to brute force in test_rate_share_left.py) bit for bit, with guard bands in front of and behind every output.
`Rater.corrections(share_left=True, precision="bf16")` is held, bit for bit, to `lm.rate_window_bulk` over the host statements'
windows in the same batches and chunks, the state carried by get_states / np.repeat / set_states; `precision="split"` to the CPU
double within the bound test_rate_corrections_gpu.py uses for the unshared call."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk, windows
from tests.test_rate_bulk_gpu import device, lib_and_stream
from tests.test_rate_corrections import SPLIT, decided, gap_threshold, oracle_costs, same_suspects, wide_rater, wide_texts
from tests.test_rate_corrections_gpu import global_suspects
from tests.test_rate_suspects_gpu import GUARD, MARK, words
from tests.test_rate_window_gpu import ptr

pytestmark = pytest.mark.gpu

KL_ERR_ARG = 5
SIZES = [0, 1, 2, 1, 0, 7, 150, 3]
LONG = 6


def prefix_corpus(n_ctx, seed=5, tail=3):
    """texts of SIZES characters end to end (ids 1 .. 9; one of 150, longer than the largest `left` here) and `tail` ids behind
    the last text; per-text contexts"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    corpus = rng.integers(1, 10, int(offsets[-1]) + tail).astype(np.int32)
    text_ctx = rng.integers(1, 200, (len(SIZES), n_ctx)).astype(np.int32) if n_ctx else None
    return corpus, offsets, text_ctx


def prefix_positions(corpus, offsets, left, S, seed=9):
    """S = 1: the first position of the long text with the whole of `left` in front of it.  Else: that one, the one before,
    the long text's first and last character, every position of the short texts, -1, n_corpus, offsets[-1], then random ones"""
    lo, hi = int(offsets[LONG]), int(offsets[LONG + 1])
    if S == 1:
        return np.array([lo + left], dtype=np.int64)
    pos = [lo + left, lo + left - 1, lo, hi - 1, -1, len(corpus), int(offsets[-1])]
    pos += [j for i, size in enumerate(SIZES) if size <= 7 for j in range(int(offsets[i]), int(offsets[i + 1]))]
    rng = np.random.default_rng(seed)
    pos = np.concatenate([np.array(pos, dtype=np.int64), rng.integers(-2, len(corpus) + 2, max(S - len(pos), 0))])
    assert len(pos) >= S
    return pos[:S].astype(np.int64)


def guarded(torch, dev, n, dtype):
    """(buffer, view): n words of `dtype` (4-byte elements) with GUARD marker words in front and behind, all prefilled with the marker"""
    buf = torch.from_numpy(np.full(n + 2 * GUARD, MARK, dtype=np.uint32)).to(dev)
    return buf, buf[GUARD:GUARD + n].view(dtype)


class Prefix(object):
    """kl_prefix_windows on device copies of host arrays; guard bands around every output"""

    def __init__(self, corpus, offsets, text_ctx, pos, T):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        up = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.n_ctx = 0 if text_ctx is None else text_ctx.shape[1]
        self.src = dict(corpus=up(corpus), offsets=up(offsets), sel_pos=up(pos), text_ctx=up(text_ctx) if self.n_ctx else None)
        self.n_corpus, self.n_texts, self.S, self.T = len(corpus), len(offsets) - 1, len(pos), T
        self.sizes = dict(idx=self.S * T, ctx=self.S * T * self.n_ctx, tgt=self.S * T, valid=self.S)
        self.fresh()

    def fresh(self):
        self.out = dict((name, guarded(self.torch, self.dev, n, self.torch.int32)) for name, n in self.sizes.items())

    def run(self, left, shift=None, **override):
        a = dict((name, ptr(t) if t is not None else None) for name, t in self.src.items())
        a.update((name, ptr(view)) for name, (_, view) in self.out.items())
        if not self.n_ctx:
            a["ctx"] = None
        a.update(n_corpus=self.n_corpus, n_texts=self.n_texts, n_ctx=self.n_ctx, S=self.S, left=left, T=self.T)
        a.update(override)
        for name, by in (shift or {}).items():      # (a misaligned pointer)
            a[name] = C.c_void_p(a[name].value + by)
        code = self.lib.kl_prefix_windows(a["corpus"], a["n_corpus"], a["offsets"], a["n_texts"], a["text_ctx"], a["n_ctx"],
                                          a["sel_pos"], a["S"], a["left"], a["T"], a["idx"], a["ctx"], a["tgt"], a["valid"],
                                          self.stream)
        self.torch.cuda.synchronize()
        return code

    def results(self):
        return dict((name, words(buf)) for name, (buf, _) in self.out.items())

    def untouched(self):
        return all((w == MARK).all() for w in self.results().values())


# ---------------------------------------------------------------------------------------------- kl_prefix_windows
@pytest.mark.parametrize("n_ctx", [0, 2, 3])
@pytest.mark.parametrize("S", [1, 37])
@pytest.mark.parametrize("extra", [-1, 2])
@pytest.mark.parametrize("left", [2, 4, 7, 64])
def test_prefix_windows_is_prefix_windows_host(left, extra, S, n_ctx):
    T = left + extra
    corpus, offsets, text_ctx = prefix_corpus(n_ctx)
    pos = prefix_positions(corpus, offsets, left, S)
    want = dict(zip(("idx", "ctx", "tgt", "valid"), ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos, left, T)))
    assert want["valid"].any() and (S == 1 or not want["valid"].all())
    p = Prefix(corpus, offsets, text_ctx, pos, T)
    runs = []
    for _ in range(2):
        p.fresh()
        assert p.run(left) == 0
        got = p.results()
        for name, ref in want.items():
            ref = ref.reshape(-1).view(np.uint32)
            assert got[name].size == ref.size + 2 * GUARD
            assert (got[name][:GUARD] == MARK).all(), name                          # nothing in front of the output
            assert np.array_equal(got[name][GUARD:GUARD + ref.size], ref), name      # every word is written: no marker is left
            assert (got[name][GUARD + ref.size:] == MARK).all(), name               # ... and nothing behind it
        runs.append(got)
    assert all(np.array_equal(runs[0][name], runs[1][name]) for name in want)


def test_prefix_windows_argument_errors():
    """KL_ERR_ARG before any launch: the outputs keep their markers"""
    S, left, T, n_ctx = 37, 7, 9, 2
    corpus, offsets, text_ctx = prefix_corpus(n_ctx)
    p = Prefix(corpus, offsets, text_ctx, prefix_positions(corpus, offsets, left, S), T)
    names = ("corpus", "offsets", "text_ctx", "sel_pos", "idx", "ctx", "tgt", "valid")
    cases = [{name: None} for name in names]                                    # (text_ctx and ctx: null while n_ctx > 0)
    cases += [dict(S=0), dict(S=-1), dict(n_texts=0), dict(left=1), dict(left=0), dict(left=T + 2), dict(T=1025), dict(T=0),
              dict(n_ctx=-1), dict(n_ctx=9), dict(n_corpus=2 ** 40 + 1), dict(S=2 ** 22 + 1)]
    cases += [dict(shift={name: 4 if name in ("offsets", "sel_pos") else 2}) for name in names]
    for case in cases:
        assert p.run(**dict(dict(left=left), **case)) == KL_ERR_ARG, case
        assert p.untouched(), case
    assert p.run(left) == 0 and not p.untouched()
    assert p.run(T + 1) == 0      # (T = left - 1 is the shortest row)


# ---------------------------------------------------------------------------------------------- kl_state_fanout
PARENT = [0, 0, 3, -1, 4, 4, 4, 7]


@pytest.mark.parametrize("row_floats", [2 * 2 * 512, 4])
def test_state_fanout_is_fan_states_host(row_floats):
    torch, dev = device()
    lib, stream = lib_and_stream()
    n_src, rows = 5, len(PARENT)
    src = (0.5 * np.arange(1, n_src * row_floats + 1)).astype(np.float32).reshape(n_src, row_floats)
    src.view(np.uint32)[1, :4] = [0x7fc00001, 0xffc00002, 0x80000000, 0x00000001]      # (a bit copy: NaN payloads, -0.0, a denormal)
    assert len(set(src.reshape(-1).view(np.uint32).tolist())) == src.size              # distinct values
    want = ratebulk.fan_states_host(src, PARENT)
    assert not want[3].any() and not want[7].any() and np.array_equal(want[1].view(np.uint32), src[0].view(np.uint32))
    src_d = torch.from_numpy(src).to(dev)
    parent_d = torch.from_numpy(np.array(PARENT, dtype=np.int32)).to(dev)
    buf, dst = guarded(torch, dev, rows * row_floats, torch.float32)

    def run(**o):
        a = dict(src=ptr(src_d), n_src=n_src, parent=ptr(parent_d), rows=rows, row_floats=row_floats, dst=ptr(dst))
        for name, by in o.pop("shift", {}).items():
            a[name] = C.c_void_p(a[name].value + by)
        a.update(o)
        code = lib.kl_state_fanout(a["src"], a["n_src"], a["parent"], a["rows"], a["row_floats"], a["dst"], stream)
        torch.cuda.synchronize()
        return code

    # KL_ERR_ARG before the launch: dst keeps its markers
    cases = [dict(src=None), dict(parent=None), dict(dst=None), dict(rows=0), dict(rows=-1), dict(n_src=0), dict(row_floats=0),
             dict(row_floats=row_floats + 2), dict(row_floats=-4), dict(rows=2 ** 31 - 1, row_floats=8),
             dict(shift=dict(src=4)), dict(shift=dict(dst=4)), dict(shift=dict(dst=8)), dict(shift=dict(parent=2)),
             dict(dst=ptr(src_d)), dict(dst=C.c_void_p(src_d.data_ptr() + 4 * row_floats * (n_src - 1))),
             dict(src=C.c_void_p(dst.data_ptr() + 4 * row_floats * (rows - 1)))]
    for case in cases:
        assert run(**case) == KL_ERR_ARG, case
        assert (words(buf) == MARK).all(), case
    before = words(src_d).copy()
    for _ in range(2):
        assert run() == 0
        got = words(buf)
        ref = want.reshape(-1).view(np.uint32)
        assert (got[:GUARD] == MARK).all() and (got[GUARD + ref.size:] == MARK).all()
        assert np.array_equal(got[GUARD:GUARD + ref.size], ref)
    assert np.array_equal(words(src_d), before)
    # src directly behind dst is no overlap
    both = torch.zeros((rows + n_src) * row_floats, dtype=torch.float32, device=dev)
    both[rows * row_floats:] = src_d.reshape(-1)
    assert run(dst=ptr(both), src=C.c_void_p(both.data_ptr() + 4 * rows * row_floats)) == 0
    assert np.array_equal(words(both)[:rows * row_floats], want.reshape(-1).view(np.uint32))


# ---------------------------------------------------------------------------------------------- the engine methods
def test_engine_prefix_windows_and_fan_states():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rate_window_gpu import make_model
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 2)
    S, left, T = 37, 7, 6
    corpus, offsets, text_ctx = prefix_corpus(2)
    pos = prefix_positions(corpus, offsets, left, S)
    up = lambda a: torch.from_numpy(a).to(dev)
    src = [up(corpus), up(offsets), up(text_ctx), up(pos)]
    want = ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos, left, T)
    got = lm.prefix_windows(*src, left=left, T=T)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
    for g, r in zip(got, want):
        assert tuple(g.shape) == r.shape and np.array_equal(g.cpu().numpy(), r)
    # a slice of the selection, as `Rater.corrections` passes its batches; no contexts
    part = lm.prefix_windows(src[0], src[1], None, src[3][5:9], left, T)
    assert tuple(part[1].shape) == (4, T, 0)
    for g, r in zip((part[0], part[2], part[3]), (want[0], want[2], want[3])):
        assert np.array_equal(g.cpu().numpy(), r[5:9])
    with pytest.raises(hipabi.KlError):
        lm.prefix_windows(src[0], src[1], src[2], src[3].to(torch.int32), left, T)
    with pytest.raises(hipabi.KlError):
        lm.prefix_windows(*src, left=left, T=left - 2)
    with pytest.raises(hipabi.KlError):
        lm.prefix_windows(*src, left=1, T=T)
    # fan_states: rows of a state array to the streams that continue from them; the result is the engine's states
    rng = np.random.default_rng(1)
    lm.set_states(rng.standard_normal((5, 2 * lm.depth, lm.width)).astype(np.float32))
    pre = lm.states
    before = lm.get_states()
    parent = np.array(PARENT, dtype=np.int32)
    out = lm.fan_states(pre, up(parent))
    assert out is lm.states and out is not pre and tuple(out.shape) == (8, 2 * lm.depth, lm.pwidth)
    want = ratebulk.fan_states_host(before, parent)
    assert np.array_equal(lm.get_states().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(pre[:, :, :lm.width].cpu().numpy(), before)
    # the same number of rows again: the same buffer; from that buffer itself: another one
    again = lm.fan_states(pre, up(parent[::-1].copy()))
    assert again.data_ptr() == out.data_ptr()
    assert np.array_equal(lm.get_states().view(np.uint32), ratebulk.fan_states_host(before, parent[::-1]).view(np.uint32))
    turned = lm.get_states()
    third = lm.fan_states(again, up(np.arange(8, dtype=np.int32)[::-1].copy()))
    assert third.data_ptr() != again.data_ptr()
    assert np.array_equal(lm.get_states().view(np.uint32), turned[::-1].view(np.uint32))
    for bad in ((pre.to(torch.float64), up(parent)), (pre, up(parent.astype(np.int64))), (pre[:, :1], up(parent)),
                (pre, up(parent[:0].copy())), (before, up(parent))):
        with pytest.raises(hipabi.KlError):
            lm.fan_states(*bad)


# ---------------------------------------------------------------------------------------------- Rater
def test_share_left_bf16_is_rate_window_bulk_on_the_host_windows():
    """every predicted character a suspect.  streams 1024: one prefix batch and one suffix chunk of more than 512 rows (run as
    1024 at width 512); streams 64: prefix batches of 60 suspects that feed five chunks of 60 rows each, shorter last ones"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    texts = texts + [texts[4][::-1], texts[6][::-1]]
    contexts = contexts + [[175], [190]]
    hip = wide_rater(hip_factory)
    lm = hip.model
    assert hasattr(lm, "prefix_windows") and lm.pwidth == 512
    k, left, ahead, deletions = 3, 6, 3, True
    R = k + 2
    T, short_T = max(left + ahead, ratebulk.MIN_T), max(1 + ahead, ratebulk.MIN_T)
    text_ctx = np.asarray([windows.clamp_context(c) for c in contexts], dtype=np.int32)

    def bulk_bits(x, z, y):
        lm.rate_bits_read(reset=True)
        lm.rate_window_bulk(x, z, y, want_probs=False)
        return lm.rate_bits_read(reset=True)

    for streams, min_gain in ((1024, 0.5), (64, -np.inf)):
        args = dict(k=k, streams=streams, max_prob=1.0, min_rank=0, precision="bf16")
        found, bits = hip.corrections(texts, contexts, left=left, ahead=ahead, deletions=deletions, min_gain=min_gain,
                                      share_left=True, **args)
        assert lm.states.shape[0] == 1 and not lm.states.cpu().numpy().any()
        stats = dict(hip.shared_left)
        want, want_bits = hip.suspects(texts, contexts, **args)
        assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
        same_suspects(found, want)
        corpus, offsets, pos, alts = global_suspects(hip, texts, found)
        S = len(pos)
        assert S == sum(max(len(t) - 1, 0) for t in texts)
        full, short = ratebulk.left_groups(pos, offsets, left)
        assert len(full) == sum(max(len(t) - left, 0) for t in texts) and len(full) and len(short)
        chunk = max(1, streams // R)
        batches = ratebulk.prefix_batches(len(full), streams, R)
        assert stats == dict(suspects=S, shared=len(full), prefix_windows=len(batches),
                             suffix_windows=sum(len(c) for _, _, c in batches), unshared_windows=-(-len(short) // chunk))
        if streams == 64:
            assert len(batches) > 1 and len(batches[0][2]) > 1 and len(full) % chunk and len(short) % chunk
        else:
            assert len(batches) == 1 and len(full) * R > 512
        cost, valid = np.zeros((S, R)), np.zeros((S, R), dtype=np.int32)
        # the short group: one window per variant, in chunks of its own
        for a in range(0, len(short), chunk):
            at = short[a:a + chunk]
            x, z, y, ok = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos[at], alts[at], left, ahead, 1, T)
            lm.reset_states(len(x))
            cost[at], valid[at] = bulk_bits(x, z, y).reshape(-1, R), ok.reshape(-1, R)
        # the full group: a prefix window per batch, its states repeated for the variants' short rows of every chunk
        for a, b, chunks in batches:
            x, z, y, ok = ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos[full[a:b]], left, left - 1)
            assert ok.all()
            lm.reset_states(b - a)
            assert not bulk_bits(x, z, y).any()      # (no targets: no bits)
            pre = lm.get_states()
            assert pre.shape[0] == b - a and pre.any(axis=(1, 2)).all()
            for c, d in chunks:
                at = full[c:d]
                x, z, y, ok = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos[at], alts[at], 1, ahead, 1, short_T)
                lm.set_states(np.repeat(pre[c - a:d - a], R, axis=0))
                cost[at], valid[at] = bulk_bits(x, z, y).reshape(-1, R), ok.reshape(-1, R)
        assert (cost[valid == 0] == 0.0).all() and (cost[valid == 1] > 0.0).all()      # (a dummy stream takes no bits)
        cost, best, gain = ratebulk.variant_pick_host(cost, valid)
        got = np.concatenate([f.cost for f in found])
        assert got.shape == (S, R) and np.array_equal(got.view(np.uint64), cost.view(np.uint64))
        best_id = np.where(best == 0, -1, np.where(best == k + 1, -2, alts[np.arange(S), np.clip(best - 1, 0, k - 1)]))
        drop = (best == 0) | ~(gain >= min_gain)
        best_id[drop], gain[drop] = -1, 0.0
        assert np.array_equal(np.concatenate([f.best_id for f in found]), best_id)
        assert np.array_equal(np.concatenate([f.gain for f in found]).view(np.uint64), gain.view(np.uint64))
        assert (best_id >= 0).any() and ((best_id == -1).any() or min_gain == -np.inf)
        lm.reset_states(1)


def test_share_left_split_against_the_double():
    """test_corrections_split_against_the_double with share_left=True: the texts, seed and settings
    test_split_contract_texts_keep_the_oracle_within_the_cap checks on the CPU, every finite cost within `oracle_costs`' bound
    (the project's SPLIT_BOUND on every scored probability), the same choice wherever the double's is decided.
    Measured on an MI355X: 18 suspects, all of them shared (one prefix window, two suffix chunks), none too close to call,
    largest |cost - cost_oracle| 0.0055 of its bound."""
    from ocrd_keraslm_amd.lib import hipabi
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    oracle = wide_rater(OracleLM)
    hip = wide_rater(hip_factory)
    rated, _ = oracle.rate_alternatives(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"])
    max_prob, gap = gap_threshold(np.concatenate([r.probs[1:] for r in rated]))
    assert gap >= 1e-4
    found, bits = hip.corrections(texts, contexts, max_prob=max_prob, precision="split", share_left=True, **SPLIT)
    assert hip.model.precision == hipabi.KL_PREC_SPLIT and hip.model.states.shape[0] == 1
    assert not hip.model.states.cpu().numpy().any()
    stats = hip.shared_left
    assert 0 < stats["shared"] <= stats["suspects"] and stats["prefix_windows"] >= 1 and stats["suffix_windows"] >= 2
    want, want_bits = hip.suspects(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"], max_prob=max_prob,
                                   min_rank=SPLIT["min_rank"], precision="split")
    same_suspects(found, want)
    assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
    ref, _ = oracle.corrections(texts, contexts, max_prob=max_prob, precision="split", **SPLIT)
    total = sum(len(f) for f in found)
    assert total >= 10 and total == stats["suspects"]
    for one, r in zip(found, ref):
        assert np.array_equal(one.positions, r.positions)
    costs = oracle_costs(oracle, texts, contexts, found, SPLIT["left"], SPLIT["ahead"], SPLIT["deletions"])
    k = SPLIT["k"]
    worst, open_ = 0.0, 0
    for one, (cost, bound) in zip(found, costs):
        assert np.array_equal(np.isinf(one.cost), np.isinf(cost))
        fin = np.isfinite(cost)
        if fin.any():
            ratio = np.abs(one.cost[fin] - cost[fin]) / bound[fin]
            worst = max(worst, float(ratio.max()))
        sure = decided(cost, bound)
        open_ += int((~sure).sum())
        _, best, _ = ratebulk.variant_pick_host(cost, fin)
        _, got, _ = ratebulk.variant_pick_host(one.cost, np.isfinite(one.cost))
        assert np.array_equal(got[sure], best[sure])
        # what the call returned follows from its own costs (min_gain 0.0: a proposal that does not read worse)
        _, b, g = ratebulk.variant_pick_host(one.cost, np.isfinite(one.cost))
        keep = (b > 0) & (g >= SPLIT["min_gain"])
        ids = np.where(b == k + 1, -2, one.alt_ids[np.arange(len(one)), np.clip(b - 1, 0, k - 1)]) if len(one) else b
        assert np.array_equal(one.best_id, np.where(keep, ids, -1)) and np.array_equal(one.gain, np.where(keep, g, 0.0))
    print("suspects %d (%d shared), too close to call %d, max |cost - cost_oracle| / bound = %.3g"
          % (total, stats["shared"], open_, worst))
    assert open_ <= 0.1 * total
    assert worst <= 1.0, worst


def test_share_left_below_four_characters_is_the_unshared_route_on_the_device():
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    hip = wide_rater(hip_factory)
    args = dict(k=3, streams=64, max_prob=1.0, min_rank=0, left=3, ahead=3, deletions=True, min_gain=0.0, precision="bf16")
    want, want_bits = hip.corrections(texts, contexts, **args)
    found, bits = hip.corrections(texts, contexts, share_left=True, **args)
    assert hip.shared_left is None and sum(len(f) for f in found) > 64 // 5
    assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
    same_suspects(found, want)
    for one, ref in zip(found, want):
        for name in ("cost", "best_id", "gain", "best_op"):
            a, b = getattr(one, name), getattr(ref, name)
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
