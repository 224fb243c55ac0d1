"""Edge walk of the lattice decoder on the CPU: `Rater.rate_best(..., edge_walk=True)` computes an edge's probabilities ahead
of the bookkeeping (lattice_beam.walk_edge) and must choose exactly what the stepwise decoder chooses.

  * the reference-generated fixtures of tests/golden/rater_seam.json (the assertions of tests/test_rater_golden.py except the
    `calls` lists -- the walk asks the model differently, that is its point);
  * random lattices: edge_walk=True equals edge_walk=False -- paths, beams, costs, logged messages;
  * an engine with `walk_host` (a recording stub answered by chained oracle steps): one call per edge, chunks above the slot
    budget, no single steps, every intermediate slot back in the pool;
  * StatePool.refs(0)."""
import gc
from math import ceil

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import lattice_beam
from ocrd_keraslm_amd.lib.rater import StatePool
from tests.edge_walk_cases import KeepLogger, WalkOracle, random_segments, run_pages
from tests.oracle_engine import OracleLM
from tests.test_rater_golden import SEAM, lattice, make_rater

TOL = 1e-9      # the CPU tolerance of tests/test_rater_golden.py


def _golden_pages(r, case, lattices):
    traceback = None
    pages = []
    for segs in lattices:
        g, s, e = lattice(segs)
        path, entropy, traceback = r.rate_best(g, s, e, start_traceback=traceback, context=[17], lm_weight=case["lm_weight"],
                                               beam_width=case["beam_width"], beam_clustering_dist=case["dist"], edge_walk=True)
        pages.append((path, entropy, traceback))
    path, entropy, traceback = r.next_path(traceback[0], ([], traceback[1]))
    pages.append((path, entropy, traceback))
    return pages


@pytest.mark.parametrize("factory", [OracleLM, WalkOracle], ids=["chained", "walk_host"])
def test_rate_best_edge_walk_matches_reference(factory):
    r = make_rater(factory, False, True)
    for case in SEAM["rate_best"]:
        for (path, entropy, tb), ref in zip(_golden_pages(r, case, SEAM["lattices"]), case["pages"]):
            assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[a, b] for a, b, _ in ref["path"]]
            scores = np.array([s for _, _, s in path])
            assert np.abs(scores - np.array([s for _, _, s in ref["path"]])).max(initial=0) < TOL
            assert abs(entropy - ref["entropy"]) < max(TOL * 100, 1e-8)
            assert len(tb[0]) == len(ref["beam"])
            assert np.abs(np.array([n.cum_cost for n in tb[0]]) - np.array(ref["beam"])).max(initial=0) < max(TOL * 100, 1e-8)


@pytest.mark.parametrize("factory", [OracleLM, WalkOracle], ids=["chained", "walk_host"])
def test_rate_best_edge_walk_exact_ties_match_reference(factory):
    r = make_rater(factory, False, True)
    for case in SEAM["rate_best_ties"]:
        for (path, entropy, tb), ref in zip(_golden_pages(r, case, SEAM["tie_lattices"]), case["pages"]):
            assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[a, b] for a, b, _, _ in ref["path"]]
            assert [alt.index for _, alt, _ in path] == [i for _, _, i, _ in ref["path"]]
            assert [n.extras[1].index if n.extras else -1 for n in tb[0]] == [i for _, i in ref["beam"]]
            assert len(tb[0]) == len(ref["beam"])
            assert abs(entropy - ref["entropy"]) < max(TOL * 100, 1e-8)


def test_edge_walk_is_off_by_default_and_the_argument_overrides_the_attribute(monkeypatch):
    segs = [random_segments(3, n_edges=6, empty=False)]
    seen = []
    real = lattice_beam.walk_edge
    monkeypatch.setattr(lattice_beam, "walk_edge", lambda *a, **k: seen.append(1) or real(*a, **k))
    r = make_rater(OracleLM, False, True)
    assert r.edge_walk is False
    off = run_pages(r, segs)
    assert not seen                          # off by default
    r.edge_walk = True
    on = run_pages(r, segs)                  # argument None: the attribute decides
    assert len(seen) == 6
    del seen[:]
    run_pages(r, segs, edge_walk=False)      # the argument wins
    assert not seen
    assert [p["path"] for p in on] == [p["path"] for p in off]


SEEDS = list(range(100, 120))


@pytest.mark.parametrize("dist", [0, 5], ids=["plain", "clustering"])
@pytest.mark.parametrize("beam_width", [3, 10])
@pytest.mark.parametrize("factory", [OracleLM, WalkOracle], ids=["chained", "walk_host"])
def test_random_lattices_edge_walk_equals_stepwise(factory, beam_width, dist):
    """20 lattices of 30 edges, 1-6 alternatives of 0-10 characters, unmapped characters among them"""
    some_unmapped = some_empty = False
    for seed in SEEDS:
        segs = random_segments(seed)
        results, logs = [], []
        for walk in (False, True):
            r = make_rater(factory, False, True)
            r.logger = KeepLogger()
            results.append(run_pages(r, [segs], beam_width=beam_width, dist=dist, edge_walk=walk, finish=False))
            logs.append(r.logger.errors)
        for a, b in zip(*results):
            assert a["path"] == b["path"], seed
            assert a["beam"] == b["beam"], seed
            assert a["hyps"] == b["hyps"] and len(a["hyps"][0]) == len(segs), seed
            assert len(a["costs"]) == len(b["costs"])
            assert np.abs(np.array(a["costs"]) - np.array(b["costs"])).max(initial=0) <= 1e-12, seed
            assert np.abs(np.array(a["scores"]) - np.array(b["scores"])).max(initial=0) <= 1e-12, seed
            assert abs(a["entropy"] - b["entropy"]) <= 1e-12, seed
        assert logs[0] == logs[1], seed
        some_unmapped = some_unmapped or bool(logs[0])
        some_empty = some_empty or any(v is not None and v[1] == len(segs[-1]) - 1 for v in results[0][0]["beam"])
    assert some_unmapped, "the seeds must exercise the unmapped-character report"
    assert some_empty, "the seeds must bring an empty alternative into a beam"


def _walk_rater(budget=None):
    r = make_rater(WalkOracle, False, True)
    r.edge_walk = True
    r.edge_walk_slots = budget
    return r


@pytest.mark.parametrize("dist", [0, 5], ids=["plain", "clustering"])
def test_walk_host_is_called_once_per_edge_and_in_chunks_above_the_budget(dist, monkeypatch):
    segs, more = random_segments(7, empty=False), random_segments(8, empty=False)
    plain = run_pages(make_rater(OracleLM, False, True), [segs, more], dist=dist)
    # ---- under the budget (the default: WALK_SCRATCH_BYTES in slots of this model): exactly one call per edge
    r = _walk_rater()
    assert lattice_beam.walk_slot_budget(r._state_pool().slot_bytes) == lattice_beam.WALK_SCRATCH_BYTES // (2 * 2 * 32 * 4)
    whole = run_pages(r, [segs, more], dist=dist)
    assert len(r.model.walk_calls) == len(segs) + len(more)
    assert r.model.steps_taken == 0
    # ---- above it: chunks of budget // longest rows, in track order
    budget = 40
    edges = []
    real = lattice_beam.walk_edge

    def spy(tracks, walk, **kw):
        table = real(tracks, walk, **kw)
        rows = [i for i in range(len(tracks)) if tracks.length[tracks.alt[i]] > 0]
        edges.append((len(rows), max(tracks.length[tracks.alt[i]] for i in rows), table.calls))
        return table

    monkeypatch.setattr(lattice_beam, "walk_edge", spy)
    r = _walk_rater(budget)
    chunked = run_pages(r, [segs, more], dist=dist)
    assert len(edges) == len(segs) + len(more)
    assert any(calls > 1 for _, _, calls in edges)
    for rows, longest, calls in edges:
        assert calls == ceil(rows / max(1, budget // longest))
    assert len(r.model.walk_calls) == sum(calls for _, _, calls in edges)
    at = 0
    for rows, longest, calls in edges:
        per = max(1, budget // longest)
        for k in range(calls):
            n, lens = r.model.walk_calls[at + k]
            assert n == min(per, rows - k * per) and max(lens) <= longest
        at += calls
    assert r.model.steps_taken == 0
    for a, b, c in zip(plain, whole, chunked):
        for other in (b, c):
            assert a["path"] == other["path"] and a["beam"] == other["beam"] and a["hyps"] == other["hyps"]
            assert np.abs(np.array(a["costs"]) - np.array(other["costs"])).max(initial=0) <= 1e-12


def test_intermediate_slots_return_to_the_pool():
    r = _walk_rater()
    pool = r._state_pool()
    results = run_pages(r, [random_segments(11, empty=False), random_segments(12)], dist=5, finish=False)
    assert results
    del results
    gc.collect()
    # (run_pages keeps no node: every StateRef is gone, so everything but the zero slot must be free again, each slot once)
    assert len(pool.free) == pool.capacity - 1
    assert len(set(pool.free)) == len(pool.free)
    assert pool.zero_slot not in pool.free
    taken = pool.take_slots(5)
    assert len(taken) == 5 and len(pool.free) == pool.capacity - 6
    pool.release_slots(taken)
    assert len(pool.free) == pool.capacity - 1 and pool.take_slots(0) == []


def test_state_pool_refs_of_nothing_leaks_nothing():
    pool = StatePool(OracleLM(2, 32, 10), 2, initial=16)
    before = list(pool.free)
    assert pool.refs(0) == ([], [])
    assert pool.refs(-1) == ([], [])
    assert pool.free == before
    refs, slots = pool.refs(3)
    assert len(refs) == 3 and len(pool.free) == len(before) - 3
    del refs
    gc.collect()
    assert sorted(pool.free) == sorted(before)
