"""The device beam of `Rater.generate` on the CPU: `genbeam.expand_host` (the numpy statement of kl_beam_expand's total
order) against the host path's own bookkeeping (rater.py, `generate`: argsort, searchsorted, insort by float key, truncate),
and `Rater.generate(..., device_beam=True)` on a CPU double that offers `beam_expand` / `beam_generate` through genbeam
against the untouched host loop -- strings, the switch, and the pool's free list."""
from bisect import bisect_left

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import Node, Rater, genbeam
from tests.edge_walk_cases import chained_reference
from tests.oracle_engine import OracleLM

ROWS, FAN, FLOOR = 256, 10, 0.004


def host_bookkeeping(fringe, preds, i_c):
    """rater.py generate's loop body, verbatim but for the nodes' values (ids instead of characters) and states"""
    next_fringe, keys = [], []
    for j, n in enumerate(fringe):
        pred = preds[j]
        pred_best = np.argsort(pred)[-10:]
        pred_best = pred_best[np.searchsorted(pred[pred_best], 0.004):]
        costs = -np.log(pred[pred_best])
        base = n.cum_cost
        for best, cost in zip(pred_best, costs):
            if best not in i_c:
                continue
            if len(keys) >= 256 and base + cost > keys[-1]:
                continue
            node = Node(parent=n, state=j, value=int(best), cost=cost)
            pos = bisect_left(keys, node.cum_cost)
            keys.insert(pos, node.cum_cost)
            next_fringe.insert(pos, node)
            if len(keys) > 256:
                keys.pop()
                next_fringe.pop()
    return next_fringe


def softmax_rows(rng, n, V, scale):
    z = rng.standard_normal((n, V)) * scale
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def test_expand_host_chained_equals_the_host_bookkeeping():
    V = 40
    rng = np.random.default_rng(5)
    i_c = {i: chr(0x40 + i) for i in range(1, V) if i != 7}      # id 0 and id 7 are not to be generated
    valid = np.zeros(V, dtype=np.uint8)
    valid[list(i_c)] = 1
    # two roots of equal cost: with bitwise-equal rows all their continuations tie pairwise, and so do the children's
    fringe = [Node(state=None, value=1, cost=0.0), Node(state=None, value=2, cost=0.0)]
    cum = np.full(ROWS, np.inf, dtype=np.float32)
    cum[:2] = 0.0
    ties_seen = truncated = 0
    for step in range(8):
        probs = softmax_rows(rng, ROWS, V, 2.0)
        live = len(fringe)
        if step in (0, 1, 3):      # tied parents get the same row: exact ties between different rows
            for r in range(1, live):
                if fringe[r].cum_cost == fringe[r - 1].cum_cost:
                    probs[r] = probs[r - 1]
                    ties_seen += 1
        want = host_bookkeeping(fringe, probs[:live], i_c)
        idx, slot_in, cum_next, parent, n_live = genbeam.expand_host(probs, cum, valid, ROWS, FAN, FLOOR,
                                                                     slot_new=np.arange(1000, 1000 + ROWS), zero_slot=7)
        assert n_live == len(want)
        truncated += n_live == ROWS
        assert [(n.state, n.value) for n in want] == list(zip(parent[:n_live].tolist(), idx[:n_live].tolist()))
        want_cum = np.array([n.cum_cost for n in want])
        assert want_cum.dtype == np.float32                      # (the host path accumulates in float32)
        assert cum_next.dtype == np.float32 and np.array_equal(want_cum, cum_next[:n_live])
        assert np.array_equal(slot_in[:n_live], 1000 + parent[:n_live])
        assert (idx[n_live:] == 0).all() and (slot_in[n_live:] == 7).all() and (parent[n_live:] == -1).all()
        assert np.isinf(cum_next[n_live:]).all()
        fringe, cum = want, cum_next
    assert ties_seen > 10 and truncated >= 5


def test_expand_host_tie_rule_floor_and_invalid_ids():
    """within a row equal probabilities go by smaller id first; p == floor is kept, the float32 below it dropped; an invalid
    id among the `fan` largest occupies its place"""
    floor = np.float32(0.004)
    below = np.nextafter(floor, np.float32(0))
    p = np.zeros((2, 12), dtype=np.float32)
    p[0, [0, 3, 5, 8, 9]] = [0.5, 0.2, 0.2, floor, below]      # id 0 (invalid) is the most likely
    p[1, [1, 2, 4, 6]] = [0.3, 0.3, 0.3, 0.1]                  # fan 3: the three equal ones, ids ascending; 0.1 is out
    cum = np.array([0.0, np.inf], dtype=np.float32)
    idx, _slot, c, parent, n_live = genbeam.expand_host(p, cum, None, 2, 5, floor)
    assert n_live == 2 and idx.tolist() == [3, 5] and parent.tolist() == [0, 0]      # (2 rows: truncated to the two cheapest)
    # rows 0 and 2 hold the same row at the same cost: the later row's candidates go in front, pair by pair
    idx, _slot, c, parent, n_live = genbeam.expand_host(np.vstack([p, p, p]), np.array([0, np.inf, 0, np.inf, np.inf, np.inf], dtype=np.float32),
                                                        None, 6, 5, floor)
    assert list(zip(parent.tolist(), idx.tolist())) == [(2, 3), (2, 5), (0, 3), (0, 5), (2, 8), (0, 8)] and n_live == 6
    idx, _slot, c, parent, n_live = genbeam.expand_host(p[[1, 0, 0, 0]], np.array([0, np.inf, np.inf, np.inf], dtype=np.float32),
                                                        None, 4, 3, floor)
    assert n_live == 3 and idx.tolist() == [1, 2, 4, 0] and parent.tolist() == [0, 0, 0, -1]
    idx, _slot, c, parent, n_live = genbeam.expand_host(np.tile(p[:1], (8, 1)), np.r_[np.float32(0), np.full(7, np.inf, np.float32)],
                                                        None, 8, 5, floor)
    assert n_live == 3 and idx[:3].tolist() == [3, 5, 8]      # floor itself kept, the value below dropped, id 0 holds a place
    assert c[2] == np.float32(0) + (-np.log(floor))


# ---------------------------------------------------------------------- Rater.generate on a CPU double
class BeamOracle(OracleLM):
    """OracleLM (float32, as the HIP engine delivers) that offers the device beam's two calls through genbeam"""

    def __init__(self, *args, **kwargs):
        kwargs.setdefault("dtype", np.float32)
        super().__init__(*args, **kwargs)
        self.beam_generates = 0
        self.expands = 0
        self.fail_at = None

    def beam_expand(self, probs, cum_in, slot_new, zero_slot, fan, floor, valid=None):
        self.expands += 1
        if self.fail_at is not None and self.expands >= self.fail_at:
            raise RuntimeError("engine failure in the middle of the search")
        return genbeam.expand_host(probs, cum_in, valid, len(cum_in), fan, floor, slot_new, zero_slot)

    def beam_generate(self, *args):
        self.beam_generates += 1
        return genbeam.run_steps(self, *args)


class BeamWalkOracle(BeamOracle):
    """... and `walk_host` (the prefix warm-up's one call)"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.walk_calls = []

    def walk_host(self, lens, idx, target, ctx, slot_in, slot_step, head_k=0, timeout=20.0):
        lens = [int(k) for k in lens]
        tprob, _last = chained_reference(self.cfg, self.w, self.pool, lens, idx, target, ctx, slot_in, slot_step)
        self.walk_calls.append(lens)
        return tprob, None


def make_rater(factory, seed, emb_std):
    chars = [chr(c) for c in range(0x41, 0x41 + 60)]          # (tests/test_generate_equivalence.py's model)
    r = Rater(engine_factory=factory)
    r.width, r.depth, r.length = 16, 1, 8
    r.stateful, r.incremental = False, True
    r.mapping = ({c: i + 1 for i, c in enumerate(chars)}, {i + 1: c for i, c in enumerate(chars)})
    r.voc_size = len(chars) + 1
    r.configure()
    r.model.init_weights(seed=seed, emb_std=emb_std)
    r.status = 2
    return r


@pytest.mark.parametrize("factory", [BeamOracle, BeamWalkOracle])
@pytest.mark.parametrize("seed,emb_std", [(1, 0.05), (2, 0.5), (3, 1.5)])
def test_generate_device_beam_equals_host_path(factory, seed, emb_std):
    r = make_rater(factory, seed, emb_std)
    want = r.generate("ABC", 20, [17], 5, device_beam=False)
    want_costs = list(r.generate_costs)
    assert r.model.beam_generates == 0 and len(want) == 5 and all(len(s) == 21 and s[0] == "C" for s in want)
    steps_host = len(r.model.step_calls)
    got = r.generate("ABC", 20, [17], 5, device_beam=True)
    assert r.model.beam_generates == 1
    assert got == want
    # (both accumulate in float32; the double's float32 products depend on the batch, 256 rows against the live ones)
    assert r.generate_costs == pytest.approx(want_costs, rel=1e-5)
    if factory is BeamWalkOracle:      # the prefix in ONE call, then 20 steps of 256 rows
        assert r.model.walk_calls == [[2]]
        assert r.model.step_calls[steps_host:] == [256] * 20
    # a one-character prefix needs no warm-up; length 0 returns the prefix's last character on both paths
    assert r.generate("Q", 6, [17], 3, device_beam=True) == r.generate("Q", 6, [17], 3, device_beam=False)
    assert r.generate("AB", 0, [17], 3, device_beam=True) == r.generate("AB", 0, [17], 3, device_beam=False) == ["B"]
    if factory is BeamWalkOracle:
        assert r.model.walk_calls == [[2]]


def test_device_beam_is_off_by_default_and_switched_by_attribute_argument_and_environment(monkeypatch):
    monkeypatch.delenv("KERASLM_DEVICE_BEAM", raising=False)
    r = make_rater(BeamOracle, 2, 0.5)
    assert r.device_beam is False
    want = r.generate("AB", 5, [17], 2)
    assert r.model.beam_generates == 0
    r.device_beam = True
    assert r.generate("AB", 5, [17], 2) == want and r.model.beam_generates == 1
    assert r.generate("AB", 5, [17], 2, device_beam=False) == want and r.model.beam_generates == 1      # the argument wins
    monkeypatch.setenv("KERASLM_DEVICE_BEAM", "1")
    assert Rater(engine_factory=BeamOracle).device_beam is True
    # an engine without beam_expand: the host loop, whatever the switch says
    plain = make_rater(lambda *a: OracleLM(*a, dtype=np.float32), 2, 0.5)
    assert plain.generate("AB", 5, [17], 2, device_beam=True) == want


@pytest.mark.parametrize("factory", [BeamOracle, BeamWalkOracle])
def test_device_beam_returns_its_slots_also_when_the_engine_raises(factory):
    r = make_rater(factory, 2, 0.5)
    pool = r._state_pool()
    before = list(pool.free)
    r.generate("ABCD", 6, [17], 2, device_beam=True)
    assert sorted(pool.free) == sorted(before) and pool.capacity >= 2 * ROWS
    r.model.fail_at = r.model.expands + 3
    with pytest.raises(RuntimeError, match="in the middle"):
        r.generate("ABCD", 6, [17], 2, device_beam=True)
    assert sorted(pool.free) == sorted(before)
    r.model.fail_at = None
    before = list(pool.free)
    r.generate("A", 4, [17], 2, device_beam=True)
    assert pool.free == before      # (no warm-up states: the very same list)


def test_backtrack_spells_from_the_back_pointers():
    parent = np.array([[0, 0, -1], [1, 0, 0], [2, 0, -1]], dtype=np.int32)
    idx = np.array([[1, 2, 0], [3, 1, 2], [1, 3, 0]], dtype=np.int32)
    i_c = {1: "a", 2: "b", 3: "c"}
    assert genbeam.backtrack((parent, idx), 5, i_c, "X") == ["Xaba", "Xbcc"]
    assert genbeam.backtrack((parent, idx), 1, i_c, "X") == ["Xaba"]
    assert genbeam.backtrack((parent[:0], idx[:0]), 3, i_c, "X") == ["X"]


def test_cli_generate_has_the_switch():
    from click.testing import CliRunner
    from ocrd_keraslm_amd.scripts.run import cli
    res = CliRunner().invoke(cli, ["generate", "--help"])
    assert res.exit_code == 0 and "--device-beam" in res.output
