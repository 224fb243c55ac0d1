"""Lattices decoded in lockstep on the CPU: `lattice_batch.edge_decode_host` (the statement that defines kl_edge_decode) against
`lattice_beam.decode_edge(table=...)`, `_finish` and the truncation to the beam width on random single edges, and
`Rater.rate_best_batch` against `rate_best(edge_walk=True)` per lattice -- random lattices of different lengths, carried
tracebacks, per-lattice contexts, history clustering, the unmapped-character report, the golden fixtures."""
from math import log

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import lattice_batch, lattice_beam
from ocrd_keraslm_amd.lib.node import Node
from tests.edge_walk_cases import KeepLogger, WalkOracle, random_segments, run_pages, summary
from tests.oracle_engine import OracleLM
from tests.test_rater_golden import SEAM, lattice, make_rater

TOL = 1e-9      # the CPU tolerance of tests/test_rater_golden.py


# ---------------------------------------------------------------------------------------------------------------- single edges
class _Alt(object):
    def __init__(self, text, conf, index):
        self.Unicode, self.conf, self.index = text, conf, index


class _Elem(object):
    id = "e"


class _State(object):
    """a state handle of the double: a pool slot and a vector"""

    def __init__(self, slot, vec):
        self.slot, self.vec = slot, vec


def _close(a, b):
    d = a.vec - b.vec
    return float(np.dot(d, d)) < 25.0


def random_edge(rng, n_in, alts, n_pre=0, twin_of=None, tie_pre=False, lm_weight=0.5, spread=1.0):
    """One edge as both sides need it.  alts: [(text, conf)].  Every track gets random step probabilities and a final state
    far from all others, except: twin_of=(a, b) -- alternatives a and b have EQUAL text and every hypothesis' two tracks
    end in identical states."""
    c_i = dict((c, k + 1) for k, c in enumerate("abcdefghij"))
    incoming = []
    slot = [1]

    def state(vec=None):
        slot[0] += 1
        return _State(slot[0], vec if vec is not None else rng.normal(0, 100.0, 4))

    for _ in range(n_in):
        n = Node(state=state(), value="a", cost=float(rng.uniform(0, 4 * spread)))
        incoming.append(n)
    alternatives = [_Alt(t, c, k) for k, (t, c) in enumerate(alts)]
    tracks = lattice_beam.EdgeTracks(incoming, alternatives, _Elem(), c_i, lm_weight, KeepLogger())
    n = len(tracks)
    table = lattice_beam.EdgeTable(n)
    n_alt = len(alts)
    for i in range(n):
        k = tracks.length[tracks.alt[i]]
        table.prob[i] = [float(np.float32(p)) for p in rng.uniform(0.02, 1.0, k) ** (2 * spread)]
        table.final[i] = state() if k else None
    if twin_of:
        a, b = twin_of
        for p in range(n_in):
            table.final[p * n_alt + b] = _State(table.final[p * n_alt + b].slot, table.final[p * n_alt + a].vec.copy())
    pre = []
    for j in range(n_pre):
        text = alts[j % n_alt][0] if j % 2 == 0 else "zz"
        node = Node(state=state(), value=text, cost=float(rng.uniform(2, 12)), extras=(_Elem(), _Alt(text, 1.0, 0)))
        pre.append(node)
    pre.sort(key=lambda nd: nd.cum_cost)
    if tie_pre:
        # an entry of exactly the cost a finishing track will have: track 0's full walk
        c = float(incoming[0].cum_cost)
        for p in table.prob[0]:
            c += -log(p if p > 1e-99 else 1e-99, 2) * lm_weight + tracks.conf_term[0]
        text = "zz"
        pre.append(Node(state=state(), value=text, cost=c, extras=(_Elem(), _Alt(text, 1.0, 0))))
        pre.sort(key=lambda nd: nd.cum_cost)
    return tracks, table, pre


def both_sides(tracks, table, pre, batch_size, max_batches, beam_width, clustering):
    """(reference survivors [(kind, ref, cost)], consumed) and the statement's, from the same edge"""
    n_alt = len(tracks.alternatives)
    n = len(tracks)
    # ---- the statement's inputs, from the untouched tracks
    eb = lattice_batch.EdgeBatch()
    alt_class, pre_class = lattice_batch._classes(tracks, pre)
    final_slot = [table.final[i].slot if table.final[i] is not None else 0 for i in range(n)]
    eb.add_edge([h.cum_cost for h in tracks.incoming], [h.state.slot for h in tracks.incoming], tracks.length, tracks.conf_term,
                alt_class, final_slot, [p.cum_cost for p in pre], pre_class, [p.state.slot for p in pre], max_batches)
    arrays = eb.arrays()
    probs = [p for i in range(n) for p in table.prob[i]]
    cost = lattice_batch.edge_costs_host(probs, arrays["pair_alt"].tolist(), arrays["alt_conf"].tolist(), tracks.lm_weight)
    by_slot = dict((h.state.slot, h.state) for h in list(tracks.incoming) + pre)
    by_slot.update((s.slot, s) for s in table.final if s is not None)
    close = (lambda a, b: _close(by_slot[a], by_slot[b])) if clustering else None
    count, status, ref, out_cost, consumed, _when = lattice_batch.decode_batch_host(arrays, cost, batch_size, beam_width, close)
    got = [(int(ref[0, k]), float(out_cost[0, k])) for k in range(int(count[0]))]
    assert int(status[0]) == 0
    # ---- the reference: decode_edge on the table, _finish, truncation
    finished = lattice_beam.FinishedBeam(pre)
    lattice_beam.decode_edge(tracks, finished, None, batch_size, max_batches, _close if clustering else None, table=table)
    want = []
    for kind, r in finished.items[:beam_width]:
        if kind == "node":
            want.append((-1 - [id(p) for p in pre].index(id(r)), float(r.cum_cost)))
        else:
            want.append((r, float(tracks.cum[r])))
    return want, list(tracks.pos), got, consumed.tolist()


def _texts(rng, n_alt, max_len, allow_empty=False):
    out = []
    for a in range(n_alt):
        k = int(rng.integers(0 if allow_empty and a == n_alt - 1 else 1, max_len + 1))
        out.append(("".join("abcdefghij"[int(c)] for c in rng.integers(0, 10, k)), float(rng.uniform(0.05, 1.0))))
    return out


@pytest.mark.parametrize("beam_width", [1, 3, 10])
@pytest.mark.parametrize("batch_size", [1, 3, 128])
def test_edge_decode_host_equals_decode_edge_on_random_edges(batch_size, beam_width):
    fired = dict(drop=0, cut=0, pre=0)
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        alts = _texts(rng, int(rng.integers(1, 7)), 8, allow_empty=seed % 5 == 0)
        n_pre = int(rng.integers(0, 4)) if seed % 3 == 0 else 0
        tracks, table, pre = random_edge(rng, int(rng.integers(1, 11)), alts, n_pre=n_pre, tie_pre=seed % 6 == 0,
                                         spread=3.0 if seed % 2 else 1.0)
        max_batches = 3 * max(len(t) for t, _ in alts) if seed % 4 else 2
        want, pos, got, consumed = both_sides(tracks, table, pre, batch_size, max(1, max_batches), beam_width, False)
        assert got == want, seed           # references, order and costs bit for bit
        assert consumed == pos, seed
        fired["pre"] += any(r < 0 for r, _ in want)
        fired["cut"] += any(p < tracks.length[tracks.alt[i]] for i, p in enumerate(pos))
    assert fired["cut"], "some edge must leave tracks on their way (margins or max_batches)"
    if beam_width == 10:
        assert fired["pre"], "some pre-existing entry must survive"


def test_edge_decode_host_equal_cost_entry_at_the_destination():
    """a pre-existing entry of exactly a finishing track's cost: insort_left puts the track in front"""
    rng = np.random.default_rng(5)
    tracks, table, pre = random_edge(rng, 2, [("abc", 0.9), ("de", 0.8)], tie_pre=True)
    want, pos, got, consumed = both_sides(tracks, table, pre, 128, 9, 10, False)
    assert got == want and consumed == pos
    costs = [c for _, c in want]
    k = [r for r, _ in want].index(0)
    assert want[k + 1][0] < 0 and costs[k] == costs[k + 1]


def test_edge_decode_host_empty_alternative_keeps_the_parents_slot():
    rng = np.random.default_rng(6)
    tracks, table, pre = random_edge(rng, 3, [("abc", 0.9), ("", 0.5)])
    want, pos, got, consumed = both_sides(tracks, table, pre, 128, 9, 10, True)
    assert got == want and consumed == pos
    assert got[0][0] % 2 == 1 and consumed[got[0][0]] == 0       # an empty alternative costs nothing: it heads the beam


def test_edge_decode_host_waiting_margin_drops_a_track():
    """+2.5 against the head of the waiting list: a hopeless alternative never finishes"""
    rng = np.random.default_rng(7)
    tracks, table, pre = random_edge(rng, 2, [("abcdef", 0.9), ("abcdeg", 0.9)])
    for i in (1, 3):
        table.prob[i][0] = 1e-4          # 6.6 bits behind after its first character
    want, pos, got, consumed = both_sides(tracks, table, pre, 1, 18, 10, False)
    assert got == want and consumed == pos
    assert consumed[1] == 1 and consumed[3] == 1 and got and all(r % 2 == 0 for r, _ in got)


def test_edge_decode_host_finished_margin_breaks():
    """+15 against the best finished entry: a planted confidence of 1e-6 (10 bits per character) stops the edge"""
    rng = np.random.default_rng(8)
    tracks, table, pre = random_edge(rng, 1, [("a", 0.9), ("abcdef", 1e-6)])
    want, pos, got, consumed = both_sides(tracks, table, pre, 1, 18, 10, False)
    assert got == want and consumed == pos
    assert [r for r, _ in got] == [0] and 0 < consumed[1] < 6


def test_edge_decode_host_cut_by_max_batches():
    rng = np.random.default_rng(9)
    tracks, table, pre = random_edge(rng, 4, [("abcdefgh", 0.9), ("abcd", 0.8), ("ab", 0.7)])
    want, pos, got, consumed = both_sides(tracks, table, pre, 2, 5, 10, False)
    assert got == want and consumed == pos
    assert sum(consumed) <= 10 and any(p < tracks.length[tracks.alt[i]] for i, p in enumerate(pos))


@pytest.mark.parametrize("batch_size", [1, 128])
def test_edge_decode_host_clustering_twins_and_far_pairs(batch_size):
    rng = np.random.default_rng(10)
    # twins: alternatives 0 and 2 have equal texts and identical final states -- only the cheaper of each pair survives
    tracks, table, pre = random_edge(rng, 3, [("abc", 0.9), ("abd", 0.8), ("abc", 0.5)], twin_of=(0, 2), spread=0.05)
    want, pos, got, consumed = both_sides(tracks, table, pre, batch_size, 60, 10, True)
    assert got == want and consumed == pos
    by_parent = [r // 3 for r, _ in got if r % 3 != 1]
    assert len(by_parent) == len(set(by_parent)) == 3
    # the same pair far apart: both stay
    tracks, table, pre = random_edge(rng, 3, [("abc", 0.9), ("abd", 0.8), ("abc", 0.5)], spread=0.05)
    want, pos, got, consumed = both_sides(tracks, table, pre, batch_size, 60, 10, True)
    assert got == want and consumed == pos
    assert len(got) == 9
    # twins against pre-existing entries of the same text
    tracks, table, pre = random_edge(rng, 2, [("abc", 0.9), ("abc", 0.5)], n_pre=3, twin_of=(0, 1))
    for node in pre:
        if node.value == "abc":
            node.state.vec = table.final[0].vec.copy()
    want, pos, got, consumed = both_sides(tracks, table, pre, batch_size, 60, 10, True)
    assert got == want and consumed == pos


# ---------------------------------------------------------------------------------------------------------------- the batch
_STEP_MEMO = {}


class RowwiseWalkOracle(WalkOracle):
    """WalkOracle whose walk answers every row ON ITS OWN: one-row oracle steps, memoised by (state, character, context) --
    all raters of this module carry the same weights.  Why: BLAS rounds a row of a matrix product differently depending on
    how many rows the product has, so the f64 double's probabilities of a track differ in the last bit between a walk of one
    edge and a walk of twenty (measured: 3 of 20 seeds end one ulp apart), and the comparison below is bitwise.  The number
    and shape of the calls are recorded as WalkOracle records them."""

    def walk_host(self, lens, idx, target, ctx, slot_in, slot_step, head_k=0, timeout=20.0):
        from oracle import lstm_oracle as O
        lens = [int(k) for k in lens]
        n = len(lens)
        idx, target, slot_step = np.asarray(idx).reshape(-1), np.asarray(target).reshape(-1), np.asarray(slot_step).reshape(-1)
        ctx = np.asarray(ctx).astype(np.int64).reshape(n, self.cfg.n_ctx)
        slot_in = np.asarray(slot_in).reshape(-1)
        assert len(set(slot_step.tolist())) == len(slot_step), "slot_step entries must be distinct"
        assert not set(slot_step.tolist()) & set(slot_in.tolist()), "slot_step must not name a slot_in"
        tprob = np.zeros(sum(lens), dtype=np.float64)
        last = np.zeros(n, dtype=np.int64)
        at = 0
        for i, k in enumerate(lens):
            state = self.pool[slot_in[i]]
            for t in range(k):
                key = (state.tobytes(), int(idx[at]), ctx[i].tobytes())
                hit = _STEP_MEMO.get(key)
                if hit is None:
                    probs, new = O.step_batch(self.cfg, self.w, idx[at:at + 1].astype(np.int64), ctx[i:i + 1],
                                              [state[j][None, :] for j in range(state.shape[0])])
                    hit = _STEP_MEMO[key] = (probs[0].copy(), np.stack([v[0] for v in new]))
                tprob[at] = hit[0][target[at]]
                state = hit[1]
                self.pool[slot_step[at]] = state
                at += 1
            last[i] = slot_step[at - 1]
        self.walk_calls.append((n, lens))
        heads = self.pool[last, :head_k].copy() if head_k else None
        return tprob, heads


SEEDS = list(range(200, 220))
CUTS = (3, 7, 30)


def _pages(seed):
    """two pages of one chain: the first cut to 3, 7 or 30 edges"""
    first = random_segments(seed, empty=False)[:CUTS[seed % 3]]
    second = random_segments(seed + 1000, n_edges=4 + seed % 5, empty=False)
    return [first, second]


def _batch_pages(rater, chains, contexts, beam_width, dist):
    """every chain's pages through rate_best_batch with the tracebacks carried; [summary per page] per chain"""
    out = [[] for _ in chains]
    tracebacks = None
    for page in range(len(chains[0])):
        built = [lattice(chain[page]) for chain in chains]
        results = rater.rate_best_batch([g for g, _, _ in built], [s for _, s, _ in built], [e for _, _, e in built],
                                        start_tracebacks=tracebacks, contexts=contexts, beam_width=beam_width,
                                        beam_clustering_dist=dist)
        tracebacks = [tb for _, _, tb in results]
        for o, (path, entropy, tb) in zip(out, results):
            o.append(summary(path, entropy, tb))
    return out


@pytest.mark.parametrize("dist", [0, 5], ids=["plain", "clustering"])
def test_rate_best_batch_equals_rate_best_per_lattice(dist):
    chains = [_pages(seed) for seed in SEEDS]
    contexts = [[17 + seed % 4] for seed in SEEDS]
    batch = make_rater(RowwiseWalkOracle, False, True)
    batch.logger = KeepLogger()
    got = _batch_pages(batch, chains, contexts, 10, dist)
    rounds = sum(max(len(chain[page]) for chain in chains) for page in range(2))
    assert len(batch.model.walk_calls) == rounds                 # one walk per ROUND, not per edge
    assert rounds < sum(len(p) for chain in chains for p in chain)
    assert batch.model.steps_taken == 0
    messages = []
    for chain, ctx, mine in zip(chains, contexts, got):
        single = make_rater(RowwiseWalkOracle, False, True)
        single.logger = KeepLogger()
        want = run_pages(single, chain, beam_width=10, dist=dist, edge_walk=True, context=ctx, finish=False)
        messages.extend(single.logger.errors)
        assert mine == want                                      # paths, hypotheses, beams; costs, scores and entropy bitwise
    assert messages and set(batch.logger.errors) == set(messages) and len(batch.logger.errors) == len(messages)


def test_rate_best_batch_one_context_for_all_and_none():
    segs = [random_segments(seed, n_edges=5, empty=False) for seed in (3, 4)]
    for contexts, single_ctx in (([23], (23,)), (None, None)):
        r = make_rater(RowwiseWalkOracle, False, True)
        built = [lattice(s) for s in segs]
        results = r.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built], contexts=contexts)
        for s, (path, entropy, tb) in zip(segs, results):
            one = make_rater(RowwiseWalkOracle, False, True)
            g, a, b = lattice(s)
            kw = {"context": list(single_ctx)} if single_ctx else {}
            assert summary(path, entropy, tb) == summary(*one.rate_best(g, a, b, edge_walk=True, **kw))


def test_rate_best_batch_above_the_slot_budget_walks_in_chunks():
    segs = [random_segments(seed, n_edges=4, unmapped=False, empty=False) for seed in (5, 6, 7)]
    r = make_rater(RowwiseWalkOracle, False, True)
    built = [lattice(s) for s in segs]
    slot = r._state_pool().slot_bytes
    results = r.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built], slot_budget_bytes=40 * slot)
    assert len(r.model.walk_calls) > 4
    assert all(sum(lens) <= 40 or n == 1 for n, lens in r.model.walk_calls)
    for s, (path, entropy, tb) in zip(segs, results):
        one = make_rater(RowwiseWalkOracle, False, True)
        g, a, b = lattice(s)
        assert summary(path, entropy, tb) == summary(*one.rate_best(g, a, b, edge_walk=True))


def test_rate_best_batch_on_an_engine_without_walk_host():
    """OracleLM has neither walk_host nor the decode: chained steps per edge, decode_edge on their table"""
    segs = [random_segments(seed, n_edges=6) for seed in (8, 9)]
    r = make_rater(OracleLM, False, True)
    r.logger = KeepLogger()
    built = [lattice(s) for s in segs]
    results = r.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built], contexts=[17],
                                beam_clustering_dist=5)
    logs = []
    for s, (path, entropy, tb) in zip(segs, results):
        one = make_rater(OracleLM, False, True)
        one.logger = KeepLogger()
        assert [summary(path, entropy, tb)] == run_pages(one, [s], dist=5, edge_walk=True, finish=False)
        logs.extend(one.logger.errors)
    assert set(r.logger.errors) == set(logs)


def _golden_batch(r, cases, lattices):
    """all cases' chains in one batch per parameter set; {case number: pages as test_rater_golden lists them}"""
    out = {}
    groups = {}
    for k, case in enumerate(cases):
        groups.setdefault((case["lm_weight"], case["beam_width"], case["dist"]), []).append(k)
    for (lm_weight, beam_width, dist), members in groups.items():
        tracebacks = None
        pages = dict((k, []) for k in members)
        for segs in lattices:
            built = [lattice(segs) for _ in members]
            results = r.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built],
                                        start_tracebacks=tracebacks, contexts=[17], lm_weight=lm_weight, beam_width=beam_width,
                                        beam_clustering_dist=dist)
            tracebacks = [tb for _, _, tb in results]
            for k, res in zip(members, results):
                pages[k].append(res)
        for k, tb in zip(members, tracebacks):
            pages[k].append(r.next_path(tb[0], ([], tb[1])))
        out.update(pages)
    return out


def test_golden_lattices_as_one_batch():
    r = make_rater(RowwiseWalkOracle, False, True)
    pages = _golden_batch(r, SEAM["rate_best"], SEAM["lattices"])
    for k, case in enumerate(SEAM["rate_best"]):
        for (path, entropy, tb), ref in zip(pages[k], case["pages"]):
            assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[a, b] for a, b, _ in ref["path"]]
            scores = np.array([s for _, _, s in path])
            assert np.abs(scores - np.array([s for _, _, s in ref["path"]])).max(initial=0) < TOL
            assert abs(entropy - ref["entropy"]) < max(TOL * 100, 1e-8)
            assert len(tb[0]) == len(ref["beam"])
            assert np.abs(np.array([n.cum_cost for n in tb[0]]) - np.array(ref["beam"])).max(initial=0) < max(TOL * 100, 1e-8)
    pages = _golden_batch(r, SEAM["rate_best_ties"], SEAM["tie_lattices"])
    for k, case in enumerate(SEAM["rate_best_ties"]):
        for (path, entropy, tb), ref in zip(pages[k], case["pages"]):
            assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[a, b] for a, b, _, _ in ref["path"]]
            assert [alt.index for _, alt, _ in path] == [i for _, _, i, _ in ref["path"]]
            assert [n.extras[1].index if n.extras else -1 for n in tb[0]] == [i for _, i in ref["beam"]]
            assert len(tb[0]) == len(ref["beam"])
            assert abs(entropy - ref["entropy"]) < max(TOL * 100, 1e-8)


def test_edges_beyond_the_kernels_capacity_are_decoded_from_the_same_walk(monkeypatch):
    """an edge of more tracks than the kernel holds goes through decode_edge(table=) on the round's walk (here: the limit
    lowered to 25 tracks, so that rounds mix both kinds)"""
    monkeypatch.setattr(lattice_batch, "MAX_TRACKS", 25)
    segs = [random_segments(seed, n_edges=8) for seed in (31, 32, 33)]
    r = make_rater(RowwiseWalkOracle, False, True)
    r.logger = KeepLogger()
    built = [lattice(s) for s in segs]
    results = r.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built], contexts=[17],
                                beam_clustering_dist=5)
    assert len(r.model.walk_calls) == 8
    logs = []
    for s, (path, entropy, tb) in zip(segs, results):
        one = make_rater(RowwiseWalkOracle, False, True)
        one.logger = KeepLogger()
        assert [summary(path, entropy, tb)] == run_pages(one, [s], dist=5, edge_walk=True, finish=False)
        logs.extend(one.logger.errors)
    assert sorted(r.logger.errors) == sorted(logs)
