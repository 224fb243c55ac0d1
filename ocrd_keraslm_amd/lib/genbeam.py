"""Host side of the device beam of `Rater.generate` (rating.py:685-709).

`expand_host` is one expansion and pruning step of the search in numpy float32 -- the same total order kl_beam_expand
(csrc/beam.hip) implements, so it is that kernel's checker, and it lets an engine without the kernel offer `beam_expand`;
`run_steps` chains steps and expansions for such an engine; `backtrack` spells the strings from the log of back-pointers.

The order (include/keraslm_hip.h, kl_beam_expand):
  * candidates of a live row (cum < +inf): its `fan` largest probabilities, equal values by SMALLER ID FIRST (our definition:
    the reference leaves such ties to numpy's unstable argsort); of those the ones with p >= floor (float32 comparison); of
    those the valid ids -- an invalid id among the `fan` largest still occupies its place;
  * cost = -log(p) in float32, cum = cum_in[row] + cost as one float32 addition (what Node.cum_cost does on the host path);
  * insertion sequence = row * fan + k, k counting a row's candidates from the least to the most probable: the order in
    which the host loop insorts them;
  * survivors: the first `rows` candidates by (cum ascending, insertion sequence DESCENDING) -- insort_left puts a later
    equal key in front, and truncating the running list to `rows` after every insertion leaves the head of that order.
"""
from __future__ import annotations

import numpy as np


def candidates_host(probs, cum, valid=None, rows=None, fan=10, floor=0.004):
    """ALL candidates of one step, in no particular order: (row, id, cum, sequence) arrays -- what `expand_host` orders and
    truncates (and what a test looks at to see how far apart the costs are)."""
    probs = np.asarray(probs, dtype=np.float32)
    if rows is None:
        rows = probs.shape[0]
    probs = probs[:rows]
    V = probs.shape[1]
    fan_eff = min(int(fan), V)
    cum = np.asarray(cum, dtype=np.float32).reshape(-1)[:rows]
    floor = np.float32(floor)
    ok = (np.arange(V) != 0) if valid is None else (np.asarray(valid).reshape(-1)[:V] != 0)
    ids = np.broadcast_to(np.arange(V), probs.shape)
    order = np.lexsort((ids, -probs), axis=-1)[:, :fan_eff]      # p descending, equal values by id ascending
    p_top = np.take_along_axis(probs, order, axis=1)
    keep = (p_top >= floor) & ok[order] & (cum < np.inf)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        cost = -np.log(p_top)                                      # float32
        cand_cum = cum[:, None] + cost                             # float32 + float32
    seq = np.arange(rows)[:, None] * int(fan) + (int(fan) - 1 - np.arange(fan_eff))[None, :]
    r_at, j_at = np.nonzero(keep)
    return r_at, order[r_at, j_at], cand_cum[r_at, j_at], seq[r_at, j_at]


def expand_host(probs, cum, valid=None, rows=None, fan=10, floor=0.004, slot_new=None, zero_slot=0):
    """One step: probs [rows][V], cum [rows] (+inf: dead row), valid [V] (None: every id except 0), slot_new [rows] (None: the
    row numbers).  Returns (idx [rows] int32, slot_in_next [rows] int32, cum_next [rows] float32, parent [rows] int32,
    n_live): survivor i in entry i; beyond the survivors id 0, zero_slot, +inf and parent -1."""
    if rows is None:
        rows = np.shape(probs)[0]
    slot_new = np.arange(rows, dtype=np.int32) if slot_new is None else np.asarray(slot_new, dtype=np.int32).reshape(-1)
    row, cid, c, s = candidates_host(probs, cum, valid, rows, fan, floor)
    first = np.lexsort((-s, c))[:rows]                             # cum ascending, sequence descending
    n_live = len(first)
    idx = np.zeros(rows, dtype=np.int32)
    slot_in = np.full(rows, zero_slot, dtype=np.int32)
    cum_next = np.full(rows, np.inf, dtype=np.float32)
    parent = np.full(rows, -1, dtype=np.int32)
    idx[:n_live] = cid[first]
    parent[:n_live] = row[first]
    slot_in[:n_live] = slot_new[row[first]]
    cum_next[:n_live] = c[first]
    return idx, slot_in, cum_next, parent, n_live


def run_steps(engine, idx0, slot0, ctx, length, rows, fan, floor, valid, slots_a, slots_b, zero_slot):
    """`length` steps of the search on an engine with numpy `step_slots` and `beam_expand` (HipLM.beam_generate is the same
    loop on device tensors): step s feeds the fringe to the model, writing the new states to slot set s & 1, and expands.
    Returns the log (parent [length][rows], idx, cum, n_live [length])."""
    sets = (np.asarray(slots_a, dtype=np.int32), np.asarray(slots_b, dtype=np.int32))
    ctx_rows = np.tile(np.asarray(ctx, dtype=np.int32).reshape(1, -1), (rows, 1))
    idx = np.zeros(rows, dtype=np.int32)
    slot_in = np.full(rows, zero_slot, dtype=np.int32)
    cum = np.full(rows, np.inf, dtype=np.float32)
    idx[0], slot_in[0], cum[0] = idx0, slot0, 0.0                 # the first step has one live row
    parent_log = np.full((length, rows), -1, dtype=np.int32)
    idx_log = np.zeros((length, rows), dtype=np.int32)
    cum_log = np.full((length, rows), np.inf, dtype=np.float32)
    live_log = np.zeros(length, dtype=np.int32)
    for s in range(length):
        out = sets[s & 1]
        probs = engine.step_slots(idx, ctx_rows, slot_in, out)
        idx, slot_in, cum, parent, n_live = engine.beam_expand(probs, cum, out, zero_slot, fan, floor, valid)
        parent_log[s], idx_log[s], cum_log[s], live_log[s] = parent, idx, cum, n_live
    return parent_log, idx_log, cum_log, live_log


def backtrack(log, variants, i_c, first_char):
    """The `variants` cheapest final hypotheses as strings, each starting with `first_char` (the last character of the
    prefix, as the host path's Node chain does).  log = (parent [length][rows], idx [length][rows], ...): entry i of step s
    is survivor i of that step, parent its row in step s (= survivor number in step s - 1)."""
    parent, idx = np.asarray(log[0]), np.asarray(log[1])
    length = parent.shape[0]
    if length == 0:
        return [first_char]
    out = []
    for v in range(min(int(variants), parent.shape[1])):
        if parent[length - 1, v] < 0:
            break
        chars, at = [], v
        for s in range(length - 1, -1, -1):
            chars.append(i_c[int(idx[s, at])])
            at = int(parent[s, at])
        chars.append(first_char)
        out.append(''.join(reversed(chars)))
    return out
