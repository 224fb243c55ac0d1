"""Insertion hypotheses on the GPU (run with -m gpu on an MI355X): kl_edit_windows, `HipLM.variant_windows(insertions=True)` and
`Rater.corrections(insertions=True)`.

kl_edit_windows is held to its numpy statement (`ratebulk.variant_windows_host(insertions=1)`, itself held to brute force in
test_rate_insertions.py) bit for bit, with a guard band behind every output, and with insertions = 0 to kl_variant_windows.
`Rater.corrections(precision="bf16", insertions=True)` is held, bit for bit, to `lm.rate_window_bulk` on the host statement's
windows, uploaded in the same chunks from zero states; `precision="split"` to the CPU double within the first-order bound of
the project's 2e-5 on a split-precision probability: |cost - cost_oracle| <= 2 * sum over the scored positions of
2e-5 / (p_oracle * ln 2)."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
from tests.test_rate_corrections import (SPLIT, SPLIT_BOUND, gap_threshold, same_suspects, variant_corpus, wide_rater,
                                         wide_texts)
from tests.test_rate_corrections_gpu import KL_ERR_ARG, Variants, global_suspects, suspects_for
from tests.test_rate_bulk_gpu import device
from tests.test_rate_suspects_gpu import GUARD, MARK

pytestmark = pytest.mark.gpu

Cor = ratebatch.Corrections
SHAPES = [(1, 1, 1, 0, 3), (37, 3, 5, 4, 10), (300, 8, 40, 7, 64)]      # (S, K, left, ahead, T); the second: T = left + ahead + 1
NAMES = ("idx", "ctx", "tgt", "valid")


class Edits(Variants):
    """kl_edit_windows on the device copies, guard bands and marker prefill of `Variants`"""

    def run(self, left, ahead, deletions, insertions=1, shift=None, **override):
        from tests.test_rate_window_gpu import ptr
        a = dict((name, ptr(t) if t is not None else None) for name, t in self.src.items())
        a.update((name, ptr(t)) for name, t in self.out.items())
        if not self.n_ctx:
            a["ctx"] = None
        a.update(n_corpus=self.n_corpus, n_texts=self.n_texts, n_ctx=self.n_ctx, S=self.S, K=self.K, left=left, ahead=ahead,
                 deletions=deletions, insertions=insertions, T=self.T)
        a.update(override)
        for name, by in (shift or {}).items():      # (a misaligned pointer)
            a[name] = C.c_void_p(a[name].value + by)
        code = self.lib.kl_edit_windows(a["corpus"], a["n_corpus"], a["offsets"], a["n_texts"], a["text_ctx"], a["n_ctx"],
                                        a["sel_pos"], a["sel_alt_id"], a["S"], a["K"], a["left"], a["ahead"], a["deletions"],
                                        a["insertions"], a["T"], a["idx"], a["ctx"], a["tgt"], a["valid"], self.stream)
        self.torch.cuda.synchronize()
        return code


def twice_equal_to(v, want, *args):
    """two runs on fresh markers: every word of every output is the statement's, nothing behind it is touched, and the runs agree"""
    runs = []
    for _ in range(2):
        v.fresh()
        assert v.run(*args) == 0
        got = v.results()
        for name, ref in want.items():
            ref = ref.reshape(-1).view(np.uint32)
            assert got[name].size == ref.size + GUARD
            assert np.array_equal(got[name][:ref.size], ref), name      # every word is written: no marker is left
            assert (got[name][ref.size:] == MARK).all(), name           # ... and nothing behind the output
        runs.append(got)
    assert all(np.array_equal(runs[0][name], runs[1][name]) for name in want)


# ---------------------------------------------------------------------------------------------- kl_edit_windows
@pytest.mark.parametrize("n_ctx", [0, 2, 3])
@pytest.mark.parametrize("deletions", [0, 1])
@pytest.mark.parametrize("S,K,left,ahead,T", SHAPES)
def test_edit_windows_is_variant_windows_host(S, K, left, ahead, T, deletions, n_ctx):
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = suspects_for(corpus, offsets, S, K)
    assert len(pos) == S and alts.shape == (S, K)
    R = 2 * K + 1 + deletions
    want = dict(zip(NAMES, ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T,
                                                         insertions=1)))
    ok = want["valid"].reshape(S, R)
    assert ok[:, K + 1 + deletions:].any() and (S == 1 or not ok[:, K + 1 + deletions:].all())
    if T == left + ahead + 1 and S > 1:      # a fed row that fills the whole row
        assert (want["tgt"][:, T - 1] >= 0).any()
    twice_equal_to(Edits(corpus, offsets, text_ctx, pos, alts, T, R), want, left, ahead, deletions)


@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("deletions", [0, 1])
def test_edit_windows_longest_hypothesis(deletions, n_ctx):
    """one text of 1100 ids, three suspects near position 1050, left = 1000, ahead = 23, T = 1024: a hypothesis of
    1000 + 2 + 23 = T + 1 ids, the longest the staging array has to hold"""
    rng = np.random.default_rng(77)
    corpus = rng.integers(1, 200, 1100).astype(np.int32)
    offsets = np.array([0, 1100], dtype=np.int64)
    text_ctx = rng.integers(1, 200, (1, n_ctx)).astype(np.int32) if n_ctx else None
    pos = np.array([1049, 1050, 1052], dtype=np.int64)
    alts = rng.integers(1, 200, (3, 1)).astype(np.int32)
    left, ahead, T, K = 1000, 23, 1024, 1
    R = 2 * K + 1 + deletions
    want = dict(zip(NAMES, ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T,
                                                         insertions=1)))
    rows = want["tgt"].reshape(3, R, T)
    assert want["valid"].all() and (rows[:, R - 1, T - 1] >= 0).all() and (rows[:, 0, T - 1] == -1).all()
    assert (want["idx"].reshape(3, R, T)[:, R - 1, 1000] == alts[:, 0]).all()
    twice_equal_to(Edits(corpus, offsets, text_ctx, pos, alts, T, R), want, left, ahead, deletions)


@pytest.mark.parametrize("deletions", [0, 1])
def test_edit_windows_without_insertions_is_variant_windows(deletions):
    S, K, left, ahead, T, n_ctx = 37, 3, 5, 4, 10, 2
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = suspects_for(corpus, offsets, S, K)
    R = K + 1 + deletions
    old = Variants(corpus, offsets, text_ctx, pos, alts, T, R)
    new = Edits(corpus, offsets, text_ctx, pos, alts, T, R)
    assert old.run(left, ahead, deletions) == 0 and new.run(left, ahead, deletions, insertions=0) == 0
    a, b = old.results(), new.results()
    assert not old.untouched() and all(np.array_equal(a[name], b[name]) for name in NAMES)
    want = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T)
    for name, ref in zip(NAMES, want):
        assert np.array_equal(b[name][:ref.size], ref.reshape(-1).view(np.uint32)), name


def test_edit_windows_argument_errors():
    """KL_ERR_ARG before any launch: the outputs keep their markers"""
    S, K, left, ahead, T, n_ctx = 37, 3, 5, 4, 10, 2
    corpus, offsets, text_ctx = variant_corpus(n_ctx)
    pos, alts = suspects_for(corpus, offsets, S, K)
    R = 2 * K + 2
    v = Edits(corpus, offsets, text_ctx, pos, alts, T, R)
    names = ("corpus", "offsets", "text_ctx", "sel_pos", "sel_alt_id", "idx", "ctx", "tgt", "valid")
    cases = [{name: None} for name in names]                                    # (text_ctx and ctx: null while n_ctx > 0)
    cases += [dict(S=0), dict(n_texts=0), dict(K=0), dict(K=9), dict(left=0), dict(ahead=-1), dict(T=left + ahead - 1),
              dict(T=1025), dict(n_ctx=-1), dict(n_ctx=9), dict(deletions=-1), dict(deletions=2)]
    cases += [dict(n_corpus=2 ** 40 + 1), dict(S=2 ** 22 // (K + 2) + 1)]
    cases += [dict(shift={name: 4 if name in ("offsets", "sel_pos") else 2}) for name in names]
    # what the new entry adds: the flag's range, a row one longer, more rows per suspect
    cases += [dict(insertions=-1), dict(insertions=2), dict(T=left + ahead), dict(S=2 ** 22 // R + 1)]
    assert 2 ** 22 // R + 1 <= 2 ** 22 // (K + 2)      # (rows that kl_variant_windows would take)
    for case in cases:
        assert v.run(**dict(dict(left=left, ahead=ahead, deletions=1), **case)) == KL_ERR_ARG, case
        assert v.untouched(), case
    assert v.run(left, ahead, 1, insertions=0, T=left + ahead, S=1) == 0 and not v.untouched()      # (enough without insertions)
    v.fresh()
    assert v.run(left, ahead, 1) == 0 and not v.untouched()


def test_engine_variant_windows_with_insertions():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rate_window_gpu import make_model
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 2)
    S, K, left, ahead, T = 37, 3, 5, 4, 12
    corpus, offsets, text_ctx = variant_corpus(2)
    pos, alts = suspects_for(corpus, offsets, S, K)
    up = lambda a: torch.from_numpy(a).to(dev)
    src = [up(corpus), up(offsets), up(text_ctx), up(pos), up(alts)]
    for deletions in (False, True):
        want = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, int(deletions), T, insertions=1)
        got = lm.variant_windows(*src, left=left, ahead=ahead, deletions=deletions, T=T, insertions=True)
        assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
        for g, r in zip(got, want):
            assert tuple(g.shape) == r.shape and np.array_equal(g.cpu().numpy(), r)
        # a slice of the selection, as `Rater.corrections` passes its chunks; no contexts
        part = lm.variant_windows(src[0], src[1], None, src[3][5:9], src[4][5:9], left, ahead, deletions, T, insertions=True)
        R = 2 * K + 1 + int(deletions)
        assert tuple(part[1].shape) == (4 * R, T, 0)
        for g, r in zip((part[0], part[2], part[3]), (want[0], want[2], want[3])):
            assert np.array_equal(g.cpu().numpy(), r[5 * R:9 * R])
        # the positional call of before: no insertion rows
        plain = lm.variant_windows(src[0], src[1], src[2], src[3], src[4], left, ahead, deletions, T)
        assert tuple(plain[0].shape) == (S * (K + 1 + int(deletions)), T)
    for bad in (dict(T=left + ahead, insertions=True), dict(T=T, insertions=2), dict(T=T, insertions=-1)):
        with pytest.raises(hipabi.KlError):
            lm.variant_windows(*src, left=left, ahead=ahead, deletions=False, **bad)
    lm.variant_windows(*src, left=left, ahead=ahead, deletions=False, T=left + ahead + 1, insertions=True)


# ---------------------------------------------------------------------------------------------- Rater
def picked(cost, valid, alts, k, deletions, min_gain):
    """(cost with +inf, best_id, best_op, gain) that follow from costs by `variant_pick_host` and min_gain"""
    cost, best, gain = ratebulk.variant_pick_host(cost, valid)
    S = len(best)
    first = k + 1 + deletions
    best_id = np.full(S, Cor.NO_PROPOSAL, dtype=np.int32)
    best_op = np.full(S, Cor.OP_NONE, dtype=np.int32)
    for s in range(S):
        v = int(best[s])
        if v == 0 or not gain[s] >= min_gain:
            gain[s] = 0.0
        elif v <= k:
            best_id[s], best_op[s] = alts[s, v - 1], Cor.OP_SUBSTITUTE
        elif v < first:
            best_id[s], best_op[s] = Cor.DELETE, Cor.OP_DELETE
        else:
            best_id[s], best_op[s] = alts[s, v - first], Cor.OP_INSERT
    return cost, best_id, best_op, gain


def test_corrections_bf16_with_insertions_is_rate_window_bulk_on_the_host_windows():
    """every predicted character a suspect, R = 8 variants each: first all suspects in one chunk (752 rows), then chunks of 8
    suspects with a shorter last one"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    hip = wide_rater(hip_factory)
    lm = hip.model
    assert hasattr(lm, "variant_windows") and lm.pwidth == 512
    k, left, ahead, deletions = 3, 6, 3, True
    R = 2 * k + 2
    T = max(left + ahead + 1, ratebulk.MIN_T)
    text_ctx = np.asarray([windows.clamp_context(c) for c in contexts], dtype=np.int32)
    # (min_gain 3.0: on the double a dozen of the 94 suspects gain less, the others more -- dropping a character of a text the
    # model knows little about saves about log2(voc_size) bits)
    for streams, min_gain in ((1024, 3.0), (64, -np.inf)):
        args = dict(k=k, streams=streams, max_prob=1.0, min_rank=0, precision="bf16")
        found, bits = hip.corrections(texts, contexts, left=left, ahead=ahead, deletions=deletions, min_gain=min_gain,
                                      insertions=True, **args)
        # the state afterwards: a reset single row
        assert lm.states.shape[0] == 1 and not lm.states.cpu().numpy().any()
        want, want_bits = hip.suspects(texts, contexts, **args)
        assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
        same_suspects(found, want)
        corpus, offsets, pos, alts = global_suspects(hip, texts, found)
        S = len(pos)
        assert S == sum(max(len(t) - 1, 0) for t in texts)
        chunk = max(1, streams // R)
        assert (S * R > 512 and chunk >= S) if streams == 1024 else (S > chunk and S % chunk)
        cost, valid = [], []
        for a in range(0, S, chunk):
            x, z, y, ok = ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos[a:a + chunk], alts[a:a + chunk], left,
                                                        ahead, 1, T, insertions=1)
            lm.reset_states(len(x))
            lm.rate_bits_read(reset=True)
            lm.rate_window_bulk(x, z, y, want_probs=False)
            cost.append(lm.rate_bits_read(reset=True))
            valid.append(ok)
        cost, valid = np.concatenate(cost).reshape(S, R), np.concatenate(valid).reshape(S, R)
        assert (cost[valid == 0] == 0.0).all() and (cost[valid == 1] > 0.0).all()      # (a dummy stream takes no bits)
        cost, best_id, best_op, gain = picked(cost, valid, alts, k, 1, min_gain)
        got = np.concatenate([f.cost for f in found])
        assert got.shape == (S, R) and np.array_equal(got.view(np.uint64), cost.view(np.uint64))
        # at least one insertion variant is valid and finite (every one is: no suspect is a first character, k < voc_size)
        assert np.isfinite(got[:, k + 2:]).any() and valid[:, k + 2:].all()
        assert np.array_equal(np.concatenate([f.best_id for f in found]), best_id)
        assert np.array_equal(np.concatenate([f.best_op for f in found]), best_op)
        assert all(f.best_op.dtype == np.int32 for f in found)
        assert np.array_equal(np.concatenate([f.gain for f in found]).view(np.uint64), gain.view(np.uint64))
        assert (best_op != Cor.OP_NONE).any() and ((best_op == Cor.OP_NONE).any() or min_gain == -np.inf)
        lm.reset_states(1)
    # nothing but texts without a prediction; no suspects
    for some, kw in ((["", "a"], {}), (texts[:5], dict(max_prob=0.0))):
        found, b = hip.corrections(some, k=k, deletions=True, insertions=True, **kw)
        assert [len(f) for f in found] == [0] * len(some)
        assert all(f.cost.shape == (0, R) and f.best_id.dtype == f.best_op.dtype == np.int32 and f.gain.dtype == np.float64
                   for f in found)


def oracle_edit_costs(oracle, texts, contexts, found, left, ahead, deletions):
    """test_rate_corrections.oracle_costs with the insertion rows: for the suspects and alternatives of `found` the double's
    cost of every variant and the first-order bound on a split-precision cost, 2 * sum over the scored positions of
    SPLIT_BOUND / (p_oracle * ln 2).  Returns per text (cost [m, R] with +inf where invalid, bound [m, R])."""
    out = []
    for text, ctx, one in zip(texts, contexts, found):
        k = one.alt_ids.shape[1]
        R = 2 * k + 1 + int(deletions)
        m = len(one)
        if not m:
            out.append((np.zeros((0, R)), np.zeros((0, R))))
            continue
        ids = windows.encode(windows.normalize(text), oracle.mapping[0])
        x, z, y, ok = ratebulk.variant_windows_host(ids, [0, len(ids)], np.asarray([windows.clamp_context(ctx)], dtype=np.int32),
                                                    one.positions, one.alt_ids, left, ahead, int(deletions),
                                                    max(left + ahead + 1, ratebulk.MIN_T), insertions=1)
        oracle.model.reset_states(len(x))
        full = np.asarray(oracle.model.forward_window(x, z, want_probs=True), dtype=np.float64)
        p = np.take_along_axis(full, np.maximum(y, 0)[:, :, None], axis=2)[:, :, 0]
        scored = y >= 0
        cost = -np.where(scored, np.log2(np.maximum(p, 1e-99)), 0.0).sum(axis=1)
        bound = 2.0 * np.where(scored, SPLIT_BOUND / (np.maximum(p, 1e-99) * np.log(2.0)), 0.0).sum(axis=1)
        cost[ok == 0] = np.inf
        out.append((cost.reshape(m, R), bound.reshape(m, R)))
    oracle.model.reset_states(1)
    return out


def test_corrections_split_with_insertions_against_the_double():
    """the texts, seed and settings of test_rate_corrections_gpu's split-precision test, insertions on.  The double's costs are
    taken over the HIP run's own suspects and alternatives (the same hypotheses on both sides); the pick the call returned is
    held to the call's own costs, not to the double's pick.
    Measured on an MI355X: 18 suspects, 54 insertion variants, largest |cost - cost_oracle| 0.0055 of its bound."""
    from ocrd_keraslm_amd.lib import hipabi
    from tests.oracle_engine import OracleLM
    from tests.test_rater_golden import hip_factory
    texts, contexts = wide_texts()
    oracle = wide_rater(OracleLM)
    hip = wide_rater(hip_factory)
    rated, _ = oracle.rate_alternatives(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"])
    max_prob, gap = gap_threshold(np.concatenate([r.probs[1:] for r in rated]))
    assert gap >= 1e-4
    found, bits = hip.corrections(texts, contexts, max_prob=max_prob, precision="split", insertions=True, **SPLIT)
    assert hip.model.precision == hipabi.KL_PREC_SPLIT and hip.model.states.shape[0] == 1
    want, want_bits = hip.suspects(texts, contexts, k=SPLIT["k"], streams=SPLIT["streams"], max_prob=max_prob,
                                   min_rank=SPLIT["min_rank"], precision="split")
    same_suspects(found, want)
    assert np.array_equal(bits.view(np.uint64), want_bits.view(np.uint64))
    total = sum(len(f) for f in found)
    assert total >= 10
    k, deletions = SPLIT["k"], int(SPLIT["deletions"])
    costs = oracle_edit_costs(oracle, texts, contexts, found, SPLIT["left"], SPLIT["ahead"], deletions)
    worst, inserted = 0.0, 0
    for one, (cost, bound) in zip(found, costs):
        assert one.cost.shape == (len(one), 2 * k + 1 + deletions)
        assert np.array_equal(np.isinf(one.cost), np.isinf(cost))      # the +inf pattern
        fin = np.isfinite(cost)
        inserted += int(fin[:, k + 1 + deletions:].sum())
        if fin.any():
            ratio = np.abs(one.cost[fin] - cost[fin]) / bound[fin]
            worst = max(worst, float(ratio.max()))
        # what the call returned follows from its own costs (min_gain 0.0: a proposal that does not read worse)
        _, best_id, best_op, gain = picked(one.cost, np.isfinite(one.cost), one.alt_ids, k, deletions, SPLIT["min_gain"])
        assert np.array_equal(one.best_id, best_id) and np.array_equal(one.best_op, best_op) and np.array_equal(one.gain, gain)
    print("suspects %d, insertion variants %d, max |cost - cost_oracle| / bound = %.3g" % (total, inserted, worst))
    assert inserted > 0
    assert worst <= 1.0, worst
