"""Many lattices decoded in lockstep (`Rater.rate_best_batch`): round r takes the r-th edge (lattice_beam.lattice_edges order)
of every lattice that still has one, walks ALL those edges' tracks in one engine call and decodes all of them in one more.

Three layers:

  * `edge_decode_host` -- THE STATEMENT.  One edge's bookkeeping as a plain function over arrays: exactly
    `lattice_beam.decode_edge(table=...)`, `_finish` and the truncation to `beam_width`, with everything a `Node`, an
    `EdgeTracks` or a state handle would carry replaced by numbers (costs, lengths, text-class ids, pool slots).  It defines
    the device kernel `kl_edge_decode` (csrc/edge_decode.hip), which must agree with it bit for bit, and it is what an engine
    without that kernel (the tests' CPU doubles) runs.
  * `EdgeBatch` -- the arrays of E edges, concatenated: what `edge_decode_host` reads per edge and the kernel reads per
    workgroup.
  * `decode_lattices` -- the driver: `EdgeTracks` per edge as in `rate_best`, one walk (several only above the slot budget), one
    decode, `Node`s for the survivors only.

Unmapped characters.  The single-lattice decoder reports one when the first track of an alternative reaches it, and names the
alternative by `alt.index` or -- where that is 0 or None -- by the track's place in the batch it is advanced in.  The batch
reproduces that: the decode returns how many characters every track consumed and, per (track, step) pair, a stamp
`batch number * 1024 + place in the batch`; per edge the consumed unmapped characters are then visited in stamp order and
reported once per alternative and character, with the single call's message text.  An edge's messages equal the single
call's, in its order; edges are reported round by round (the r-th edges of all lattices, then the next).

References of the survivors: a track number (>= 0), or -1 - j for the j-th entry another in-edge had already left at the
destination."""
from __future__ import annotations

from math import log

import numpy as np

from . import lattice_beam
from .lattice_beam import FINISHED_MARGIN, LOOKAHEAD, WAITING_MARGIN

MAX_TRACKS = 1024                  # tracks per edge the device kernel holds in LDS (above: that edge is decoded on the host)
MAX_PRE = 64                       # ... and entries already at the destination
BATCH_SCRATCH_BYTES = 1 << 30      # HBM the intermediate states of ONE ROUND's walk may occupy (rate_best_batch's default budget)


def batch_slot_budget(slot_bytes, budget_bytes=None):
    """(row, step) pairs one walk call of a round may be asked for: what the budget holds in pool slots.  The default of
    1 GiB is 131072 slots at depth 2, width 512 (8 KiB per slot): 256 lattices whose edges carry 60 tracks of 8 characters
    (122880 pairs) pass in one call; the pool of a 288 GB part holds it many times over."""
    return max(1, int(budget_bytes or BATCH_SCRATCH_BYTES) // max(1, int(slot_bytes)))


# ------------------------------------------------------------------------------------------------------------ the statement
def _bisect_left(keys, n, x):
    """bisect.bisect_left on keys[:n], spelled out: the first waiting list is NOT sorted, so the position is whatever
    this very sequence of probes finds (the kernel makes the same probes)"""
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if keys[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def edge_costs_host(probs, pair_alt, alt_conf, lm_weight):
    """cost of every (track, step) pair as `EdgeTracks.advance` adds it: -log2(max(p, 1e-99)) * lm_weight + conf[alt], in
    doubles, the logarithm as math.log(p, 2) (= log(p) / log(2))"""
    return [-log(p if p > 1e-99 else 1e-99, 2) * lm_weight + alt_conf[a]
            for p, a in zip(np.asarray(probs, dtype=np.float64).tolist(), list(pair_alt))]


def edge_decode_host(cum_in, slot_in, alt_len, alt_class, step_off, step_cost, final_slot, pre_cost, pre_class, pre_slot,
                     batch_size, max_batches, beam_width, close=None, when=None):
    """One edge.  n_in incoming hypotheses (cum_in f64, slot_in), n_alt alternatives (alt_len, alt_class; their confidence
    term is already part of step_cost), tracks hypothesis-major, alternative-minor: track i = (i // n_alt, i % n_alt), its
    k-th step costs step_cost[step_off[i] + k] and after its last step its state is in final_slot[i] (a track with an empty
    alternative has no steps and keeps slot_in of its parent).  pre_*: what other in-edges left at the destination, in beam
    order.  close(slot_a, slot_b) -> bool, or None (no history clustering).  when: a list as long as step_cost, or None;
    entry step_off[i] + k receives `batch number * 1024 + place in the batch` when track i takes its k-th step (a batch never
    holds more than 1024 tracks where the kernel runs).
    Returns ([(reference, cumulative cost)] -- the first beam_width finished entries --, [characters consumed per track])."""
    n_in, n_alt = len(cum_in), len(alt_len)
    n = n_in * n_alt
    cum = [float(cum_in[i // n_alt]) for i in range(n)]
    length = [int(alt_len[i % n_alt]) for i in range(n)]
    pos = [0] * n
    batch_size, max_batches = int(batch_size), int(max_batches)
    cap = max_batches * batch_size
    waiting = list(range(n))
    wkeys = [cum[i] + LOOKAHEAD * length[i] for i in range(n)]
    fkeys = [float(c) for c in pre_cost]
    frefs = [-1 - j for j in range(len(fkeys))]

    def klass(ref):
        return alt_class[ref % n_alt] if ref >= 0 else pre_class[-1 - ref]

    def slot(ref):
        if ref < 0:
            return pre_slot[-1 - ref]
        return final_slot[ref] if length[ref] else slot_in[ref // n_alt]

    def finish(i):
        if close is not None:
            for k in range(len(frefs)):
                other = frefs[k]
                if klass(other) == klass(i) and close(slot(i), slot(other)):
                    if fkeys[k] < cum[i]:
                        return
                    at = fkeys.index(fkeys[k])      # the FIRST entry of equal cost goes
                    del fkeys[at]
                    del frefs[at]
                    break
        at = _bisect_left(fkeys, len(fkeys), cum[i])
        fkeys.insert(at, cum[i])
        frefs.insert(at, i)

    for number in range(max_batches):
        batch, taken = [], 0
        for i in reversed(waiting):
            taken += 1
            if pos[i] == length[i]:
                finish(i)
            else:
                batch.append(i)
                if len(batch) >= batch_size:
                    break
        del waiting[len(waiting) - taken:]
        del wkeys[len(wkeys) - taken:]
        if not batch:
            break
        batch.reverse()
        bkeys = [cum[i] + LOOKAHEAD * (length[i] - pos[i]) for i in batch]
        batch = [batch[k] for k in sorted(range(len(batch)), key=bkeys.__getitem__)]
        if fkeys and cum[batch[0]] >= fkeys[0] + FINISHED_MARGIN:
            break
        for k, i in enumerate(batch):
            if when is not None:
                when[step_off[i] + pos[i]] = number * 1024 + k
            cum[i] += step_cost[step_off[i] + pos[i]]
            pos[i] += 1
        for i in batch:
            if waiting and cum[i] >= cum[waiting[0]] + WAITING_MARGIN:
                continue
            key = cum[i] + LOOKAHEAD * (length[i] - pos[i])
            at = _bisect_left(wkeys, len(wkeys), key)
            wkeys.insert(at, key)
            waiting.insert(at, i)
        del waiting[cap:]
        del wkeys[cap:]
    return list(zip(frefs[:beam_width], fkeys[:beam_width])), pos


# ------------------------------------------------------------------------------------------------------------ E edges as arrays
class EdgeBatch(object):
    """The edges of one round as concatenated arrays.  desc[e] = (n_in, n_alt, n_pre, in_off, alt_off, trk_off, pre_off,
    max_batches); step_off is an offset into the round's cost array (one f64 per (track, step) pair, pairs in walk-row
    order); pair_alt[s] = index into the alt_* arrays of the alternative pair s belongs to."""
    FIELDS = (("cum_in", np.float64), ("alt_conf", np.float64), ("pre_cost", np.float64), ("desc", np.int32),
              ("slot_in", np.int32), ("alt_len", np.int32), ("alt_class", np.int32), ("step_off", np.int32),
              ("final_slot", np.int32), ("pre_class", np.int32), ("pre_slot", np.int32), ("pair_alt", np.int32))

    def __init__(self):
        self.lists = dict((name, []) for name, _ in self.FIELDS)
        self.n_edges = 0
        self.n_pairs = 0

    def add_edge(self, cum_in, slot_in, alt_len, alt_conf, alt_class, final_slot, pre_cost, pre_class, pre_slot, max_batches):
        """appends one edge; its tracks' step costs follow the pairs already there (track-major).  final_slot: per track,
        ignored for empty alternatives (their hypothesis' slot is stored in its place).  Returns the edge's number."""
        ls = self.lists
        n_in, n_alt, n_pre = len(cum_in), len(alt_len), len(pre_cost)
        ls["desc"].append((n_in, n_alt, n_pre, len(ls["cum_in"]), len(ls["alt_len"]), len(ls["step_off"]), len(ls["pre_cost"]),
                           int(max_batches)))
        alt0 = len(ls["alt_len"])
        ls["cum_in"].extend(cum_in)
        ls["slot_in"].extend(slot_in)
        ls["alt_len"].extend(alt_len)
        ls["alt_conf"].extend(alt_conf)
        ls["alt_class"].extend(alt_class)
        ls["pre_cost"].extend(pre_cost)
        ls["pre_class"].extend(pre_class)
        ls["pre_slot"].extend(pre_slot)
        # (a track with an empty alternative keeps its hypothesis' slot: the kernel reads it from final_slot)
        ls["final_slot"].extend(f if alt_len[t % n_alt] else slot_in[t // n_alt] for t, f in enumerate(final_slot))
        at = self.n_pairs
        step_off, pair_alt = ls["step_off"], ls["pair_alt"]
        for _ in range(n_in):
            for a, k in enumerate(alt_len):
                step_off.append(at)
                at += k
                if k:
                    pair_alt.extend([alt0 + a] * k)
        self.n_pairs = at
        self.n_edges += 1
        return self.n_edges - 1

    def arrays(self):
        out = {}
        for name, dtype in self.FIELDS:
            a = np.asarray(self.lists[name], dtype=dtype)
            out[name] = a.reshape(-1, 8) if name == "desc" else a.reshape(-1)
        return out


def decode_batch_host(arrays, cost, batch_size, beam_width, close=None):
    """`edge_decode_host` over the edges of an EdgeBatch (arrays: EdgeBatch.arrays(), cost: the round's f64 cost array);
    the shape of the kernel's outputs: (count [E], status [E], ref [E][beam_width], cost [E][beam_width], consumed [tracks],
    when [pairs])"""
    desc = arrays["desc"]
    n_edges = len(desc)
    count = np.zeros(n_edges, dtype=np.int32)
    status = np.zeros(n_edges, dtype=np.int32)
    ref = np.zeros((n_edges, beam_width), dtype=np.int32)
    out_cost = np.zeros((n_edges, beam_width), dtype=np.float64)
    consumed = np.zeros(len(arrays["step_off"]), dtype=np.int32)
    cost = cost if isinstance(cost, list) else np.asarray(cost, dtype=np.float64).tolist()
    when = [-1] * len(cost)
    lists = dict((name, arrays[name].tolist()) for name in arrays if name != "desc")
    for e, (n_in, n_alt, n_pre, in_off, alt_off, trk_off, pre_off, max_batches) in enumerate(desc.tolist()):
        n = n_in * n_alt
        survivors, pos = edge_decode_host(
            lists["cum_in"][in_off:in_off + n_in], lists["slot_in"][in_off:in_off + n_in], lists["alt_len"][alt_off:alt_off + n_alt],
            lists["alt_class"][alt_off:alt_off + n_alt], lists["step_off"][trk_off:trk_off + n], cost,
            lists["final_slot"][trk_off:trk_off + n], lists["pre_cost"][pre_off:pre_off + n_pre],
            lists["pre_class"][pre_off:pre_off + n_pre], lists["pre_slot"][pre_off:pre_off + n_pre], batch_size, max_batches,
            beam_width, close, when)
        count[e] = len(survivors)
        for k, (r, c) in enumerate(survivors):
            ref[e, k], out_cost[e, k] = r, c
        consumed[trk_off:trk_off + n] = pos
    return count, status, ref, out_cost, consumed, np.asarray(when, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------ the driver
class _Edge(object):
    __slots__ = ("tracks", "target", "pre", "rows", "finals", "number", "max_batches", "ctx", "fallback")


def _classes(tracks, pre):
    """text-class ids: alternatives of equal text share one; an entry already at the destination gets the class of its
    `value`, or one no alternative has"""
    ids = {}
    alt_class = [ids.setdefault(t, len(ids)) for t in tracks.text]
    pre_class = [ids.get(node.value, -1) for node in pre]
    return alt_class, pre_class


def _report_unmapped(tracks, consumed, step_off, when):
    """the unmapped-character report of one edge (module docstring): consumed [tracks], step_off [tracks] into `when`"""
    if not any(any(u) for u in tracks.unmapped):
        return
    n_alt = len(tracks.alternatives)
    events = []
    for i, reach in enumerate(consumed):
        a = i % n_alt
        flags = tracks.unmapped[a]
        for p in range(reach):
            if flags[p]:
                events.append((when[step_off[i] + p], a, tracks.text[a][p]))
    events.sort()
    for stamp, a, char in events:
        if char not in tracks.reported[a]:
            tracks.reported[a].add(char)
            tracks.logger.error('unmapped character "%s" at input alternative %d of element %s', char,
                                tracks.alternatives[a].index or stamp % 1024, tracks.element.id if tracks.element else "space")


def decode_lattices(rater, graphs, start_nodes, end_nodes, start_tracebacks=None, contexts=None, lm_weight=0.5, beam_width=10,
                    beam_clustering_dist=0, slot_budget_bytes=None, timings=None):
    """What `Rater.rate_best_batch` does (its docstring has the interface).  timings: a dict that receives the seconds spent in
    'build' (host arrays), 'walk', 'decode' (launch to results on the host) and 'nodes' per call, summed over the rounds."""
    from time import perf_counter
    from . import windows
    from .node import Node
    n_lat = len(graphs)
    if len(start_nodes) != n_lat or len(end_nodes) != n_lat:
        raise ValueError("rate_best_batch: one start and one end node per lattice, please")
    if start_tracebacks is None:
        start_tracebacks = [None] * n_lat
    if contexts is None or not len(contexts):
        ctxs = [rater.underspecify_contexts()] * n_lat
    elif isinstance(contexts[0], (list, tuple, np.ndarray)):
        if len(contexts) != n_lat:
            raise ValueError("rate_best_batch: one context list per lattice (or one for all), please")
        ctxs = [c if len(c) else rater.underspecify_contexts() for c in contexts]
    else:
        ctxs = [contexts] * n_lat
    ctxs = [np.asarray(windows.clamp_context(c), dtype=np.int32).reshape(-1) for c in ctxs]
    rater._ensure_precision()
    lm = rater.model
    walk = getattr(lm, "walk_host", None)
    device = walk is not None and hasattr(lm, "edge_round")
    clustering = bool(beam_clustering_dist)
    depth = rater.depth
    batch_size = rater.batch_size
    c_i = rater.mapping[0]
    tbs, plans = [], []
    for g, s, tb in zip(graphs, start_nodes, start_tracebacks):
        if not tb:
            root = Node(state=None, value='\n', cost=0.0)
            tb = ([root], root)
        g.nodes[s]['traceback'] = tb[0]
        tbs.append(tb)
        plans.append(list(lattice_beam.lattice_edges(g, s)))
    pool = rater._state_pool() if walk is not None else None
    budget = batch_slot_budget(pool.slot_bytes, slot_budget_bytes) if pool is not None else None
    clock = dict(build=0.0, walk=0.0, decode=0.0, nodes=0.0)

    def predict(chars, states, targets=None, context=None):
        return rater._predict_refs(chars, states, context, heads=clustering, targets=targets)

    def close_refs(a, b):
        return all(rater._state_distance_below(a, b, k, beam_clustering_dist) for k in range(depth))

    for r in range(max((len(p) for p in plans), default=0)):
        t0 = perf_counter()
        edges = []
        for g, plan, ctx in zip(graphs, plans, ctxs):
            if r >= len(plan):
                continue
            source, reached = plan[r]
            data = g.edges[source, reached]
            assert 'traceback' in g.nodes[source], "breadth-first search should have visited %d first" % source
            e = _Edge()
            e.tracks = lattice_beam.EdgeTracks(g.nodes[source]['traceback'], data['alternatives'], data['element'], c_i, lm_weight,
                                               rater.logger)
            e.target = g.nodes[reached]
            e.pre = e.target.get('traceback', [])
            e.max_batches = max(len(a.Unicode) for a in data['alternatives']) * 3
            e.rows = [i for i in range(len(e.tracks)) if e.tracks.length[e.tracks.alt[i]] > 0]
            e.finals = [None] * len(e.tracks)
            e.ctx = ctx
            e.fallback = (len(e.tracks) > MAX_TRACKS or len(e.pre) > MAX_PRE
                          or any(n.pro_cost() != n.cum_cost for n in e.pre))
            edges.append(e)
        if walk is None:
            # ---- an engine without walk_host: chained steps per edge, the statement on their table
            tables = []
            for e in edges:
                table = lattice_beam.EdgeTable(len(e.tracks))
                if e.rows:
                    lattice_beam._chain_edge(e.tracks, e.rows, table,
                                             lambda ch, st, tg, ctx=e.ctx.tolist(): predict(ch, st, tg, context=ctx))
                tables.append(table)
            clock["walk"] += perf_counter() - t0
            t0 = perf_counter()
            for e, table in zip(edges, tables):
                _decode_table_host(e, table, batch_size, beam_width, close_refs if clustering else None)
            clock["decode"] += perf_counter() - t0
        else:
            _round_with_walk(rater, lm, pool, edges, budget, device, clustering, depth, beam_clustering_dist, lm_weight,
                             batch_size, beam_width, close_refs, clock, t0)
    # ---- the paths
    out = []
    for g, plan, e_node, tb in zip(graphs, plans, end_nodes, tbs):
        reached = plan[-1][1] if plan else None
        assert reached == e_node, 'breadth-first search failed to reach true end node (%s instead of %s)' % (reached, e_node)
        assert 'traceback' in g.nodes[reached], "breadth-first search failed to reach end node with any result"
        out.append(rater.next_path(g.nodes[reached]['traceback'], tb))
    if timings is not None:
        for k, v in clock.items():
            timings[k] = timings.get(k, 0.0) + v
    return out


def _decode_table_host(e, table, batch_size, beam_width, close):
    """an edge through `decode_edge(table=...)` itself: engines without walk_host, and edges beyond the kernel's capacity"""
    tracks = e.tracks
    finished = lattice_beam.FinishedBeam(e.pre)
    lattice_beam.decode_edge(tracks, finished, None, batch_size, e.max_batches, close, table=table)
    e.target['traceback'] = [ref if kind == "node" else tracks.node(ref) for kind, ref in finished.items[:beam_width]]


def _round_with_walk(rater, lm, pool, edges, budget, device, clustering, depth, dist, lm_weight, batch_size, beam_width,
                     close_refs, clock, t0):
    """one round on an engine with walk_host: all edges' rows in one walk (chunks of at most `budget` pairs), then ONE decode
    -- on the device where the engine has `edge_round`, else the statement on the host"""
    from time import perf_counter
    zero = pool.zero_slot
    # ---- walk rows of all edges, in edge and track order
    lens, fed, target, ctx_rows, slot_in, owners = [], [], [], [], [], []
    for e in edges:
        tr = e.tracks
        first = tr.first_ids()
        ctx = e.ctx
        for i in e.rows:
            own = tr.ids[tr.alt[i]]
            lens.append(len(own))
            fed.append(first[tr.parent[i]])
            fed.extend(own[:-1])
            target.extend(own)
            ctx_rows.append(ctx)
            slot_in.append(tr.state[i].slot if tr.state[i] is not None else zero)
            owners.append((e, i))
    n_rows = len(lens)
    # ---- chunks of rows whose pairs fit the budget (a single row always goes)
    chunks, c0, pairs = [], 0, 0
    for j, k in enumerate(lens):
        if j > c0 and pairs + k > budget:
            chunks.append((c0, j))
            c0, pairs = j, 0
        pairs += k
    if n_rows:
        chunks.append((c0, n_rows))
    finals, final_slots = pool.refs(n_rows)
    for (e, i), ref in zip(owners, finals):
        e.finals[i] = ref
    # ---- the edges as arrays (the pairs of an edge's tracks are contiguous and in walk-row order)
    eb = EdgeBatch()
    at = 0
    for e in edges:
        tr = e.tracks
        if e.fallback:
            e.number = -1
            at += len(e.rows)
            continue
        alt_class, pre_class = _classes(tr, e.pre)
        fs = [zero] * len(tr)
        for i in e.rows:
            fs[i] = final_slots[at]
            at += 1
        e.number = eb.add_edge(
            [h.cum_cost for h in tr.incoming], [h.state.slot if h.state is not None else zero for h in tr.incoming],
            tr.length, tr.conf_term, alt_class, fs,
            [n.cum_cost for n in e.pre], pre_class, [n.state.slot if n.state is not None else zero for n in e.pre], e.max_batches)
    arrays = eb.arrays()
    # (fallback edges' pairs are walked too but belong to no EdgeBatch edge: pair numbering of the walk vs the batch)
    walk_pair_of_batch = None
    if any(e.fallback for e in edges):
        keep, s = [], 0
        row = 0
        for e in edges:
            for i in e.rows:
                if not e.fallback:
                    keep.extend(range(s, s + lens[row]))
                s += lens[row]
                row += 1
        walk_pair_of_batch = np.asarray(keep, dtype=np.int64)
    clock["build"] += perf_counter() - t0
    t0 = perf_counter()
    use_device = device and eb.n_edges > 0 and walk_pair_of_batch is None
    head_k = depth if clustering and not use_device else 0      # (the host's predicate compares head vectors; the kernel reads the pool)
    tprob_all = None
    result = None
    round_ = lm.edge_round(arrays, lm_weight, batch_size, beam_width, depth if clustering else 0, float(dist)) if use_device else None
    probs_parts = []
    taken = []
    try:
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) if n_rows else np.zeros(1, dtype=np.int64)
        for c0, c1 in chunks:
            p0, p1 = int(off[c0]), int(off[c1])
            slot_step = []
            scratch = pool.take_slots((p1 - p0) - (c1 - c0))
            taken.append(scratch)
            s_at = 0
            for j in range(c0, c1):
                k = lens[j]
                slot_step.extend(scratch[s_at:s_at + k - 1])
                slot_step.append(final_slots[j])
                s_at += k - 1
            args = (lens[c0:c1], fed[p0:p1], target[p0:p1], np.asarray(ctx_rows[c0:c1], dtype=np.int32).reshape(c1 - c0, -1),
                    slot_in[c0:c1], slot_step)
            if use_device:
                round_.walk(args, p0, p1 - p0)
            else:
                tprob, heads = lm.walk_host(*args, head_k=head_k)
                probs_parts.append(np.asarray(tprob))
                if head_k:
                    for j in range(c0, c1):
                        finals[j].head = heads[j - c0]
        clock["walk"] += perf_counter() - t0
        t0 = perf_counter()
        if use_device:
            result = round_.finish()
            tprob_all = result.get("tprob")
    finally:
        for scratch in taken:
            pool.release_slots(scratch)
    if not use_device:
        tprob_all = np.concatenate(probs_parts) if probs_parts else np.zeros(0)
        if eb.n_edges:
            tp = tprob_all if walk_pair_of_batch is None else tprob_all[walk_pair_of_batch]
            cost = edge_costs_host(tp, arrays["pair_alt"].tolist(), arrays["alt_conf"].tolist(), lm_weight)
            close = None
            if clustering:
                by_slot = {}      # slot -> handle, for the predicate (heads travel with the handles)
                for e in edges:
                    for h in list(e.tracks.incoming) + list(e.pre):
                        if h.state is not None:
                            by_slot[h.state.slot] = h.state
                for ref in finals:
                    by_slot[ref.slot] = ref
                by_slot.setdefault(zero, [np.zeros((1, rater.width))] * (2 * depth))

                def close(a, b):
                    return close_refs(by_slot[a], by_slot[b])
            result = dict(zip(("count", "status", "ref", "cost", "consumed", "when"),
                              decode_batch_host(arrays, cost, batch_size, beam_width, close)))
    clock["decode"] += perf_counter() - t0
    t0 = perf_counter()
    # ---- per edge: Nodes for the survivors
    desc = arrays["desc"]
    row = 0
    pair = 0
    for e in edges:
        tr = e.tracks
        n_rows_e = len(e.rows)
        on_host = e.fallback or (result is not None and int(result["status"][e.number]) != 0)
        if on_host:
            if tprob_all is None:
                raise RuntimeError("edge beyond the decode kernel's capacity, and the round's probabilities were not kept")
            table = lattice_beam.EdgeTable(len(tr))
            q = pair
            for j, i in enumerate(e.rows):
                k = lens[row + j]
                table.prob[i] = np.asarray(tprob_all[q:q + k], dtype=np.float64).tolist()
                table.final[i] = e.finals[i]
                q += k
            _decode_table_host(e, table, batch_size, beam_width, close_refs if clustering else None)
        else:
            trk_off = int(desc[e.number][5])
            if any(any(u) for u in tr.unmapped):
                _report_unmapped(tr, result["consumed"][trk_off:trk_off + len(tr)].tolist(),
                                 arrays["step_off"][trk_off:trk_off + len(tr)].tolist(), result["when"])
            beam = []
            for k in range(int(result["count"][e.number])):
                ref = int(result["ref"][e.number][k])
                if ref < 0:
                    beam.append(e.pre[-1 - ref])
                    continue
                tr.cum[ref] = float(result["cost"][e.number][k])
                if tr.length[tr.alt[ref]]:
                    tr.state[ref] = e.finals[ref]
                beam.append(tr.node(ref))
            e.target['traceback'] = beam
        pair += sum(lens[row:row + n_rows_e])
        row += n_rows_e
    clock["nodes"] += perf_counter() - t0
