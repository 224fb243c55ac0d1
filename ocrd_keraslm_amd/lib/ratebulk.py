"""Scheduler of bulk rating (`Rater.rate_batch(precision="bf16")`): many independent texts as plan rows over one id corpus.

`ratebatch.plan` builds the `[B][T]` index arrays of every call on the host.  Here the ids of all texts lie end to end in ONE
vector that is uploaded once (text i at offset o_i), and a call is described by what `kl_assemble_windows` reads: one int64
row `[start, vlen, zero_col, zero_ctx, ctx_0 ..]` per stream.  The way back is `kl_rate_scatter` (a call's `[B][T]` target
probabilities to the positions of their characters in a vector shaped like the corpus) and `kl_rate_text_bits` (one f64 sum
per text over that vector).

Rules of the plan:
  * text i of n_i characters has n_i - 1 predictions; window w of a call of length T has start = o_i + done and
    vlen = min(T, n_i - 1 - done), `done` being the predictions of the text's earlier windows;
  * the windows of a text are consecutive calls of one row, and a row takes a new text only at a call boundary (its state is
    zeroed there) -- as in `ratebatch.plan`; a row with nothing to do has vlen 0: idx 0, tgt -1, no target, no bits;
  * texts of more than `length` predictions run at T = length, dealt longest first to the row that is free first;
  * texts that fit one window are sorted by length and taken in groups of `streams`; a group runs at T = its longest text's
    prediction count rounded up to a multiple of 32 (at least 3, at most `length`): few distinct (B, T) shapes, and a corpus
    of 50-character lines does not run 256-step windows.

`windows_host`, `scatter_host` and `text_bits_host` state in numpy what kl_assemble_windows, kl_rate_scatter and
kl_rate_text_bits compute; `scatter_alts_host` and `select_host` what kl_rate_scatter_alts and kl_rate_select do for rating
with alternatives (`Rater.rate_alternatives(precision="bf16")`, `Rater.suspects`); `variant_windows_host` what
kl_variant_windows / kl_edit_windows make of the suspects for `Rater.corrections`, and `variant_pick_host` is the choice among a suspect's
variants (numpy on every path: S * R doubles); `prefix_windows_host` and `fan_states_host` state kl_prefix_windows and
kl_state_fanout, which read a suspect's left context once for all its variants (`Rater.corrections(share_left=True)`);
`span_windows_host` and `span_pick_host` what kl_span_windows and kl_span_pick
make of spans with caller-supplied replacements for `Rater.rescore`.  `plan_candidates` is the plan of `Rater.rate_contexts`
-- every text under every one of C candidate contexts, the pairs as plan rows over the one corpus --, and
`scatter_planes_host` and `context_mix_host` state what kl_rate_scatter_planes and kl_context_mix make of its calls.
`word_bounds_host`, `segments_host` and `segment_select_host` state kl_word_bounds, kl_rate_segments and kl_segment_select: the
words of the texts, a rating per segment and the ordered selection among them (`Rater.suspect_words`, `Rater.rate_segments`).
`lexicon_layout_host` builds the device layout of a word list and `lexicon_neighbours_host` states kl_lexicon_neighbours: the
entries within a few edits of every query word (`Rater.lexicon_neighbours`, `Rater.correct_words`); `lexicon_splits_host` states
kl_lexicon_splits: the places at which a query word falls into two entries (`Rater.lexicon_splits`); `lexicon_chains_host` states
kl_lexicon_chains: a query word as a chain of up to 8 exact entries, links between them allowed (`Rater.lexicon_chains`).
numpy only: the plan is built and tested without an engine.
"""
from __future__ import annotations

import numpy as np

CTX_CAND_MAX = 256          # candidate contexts of `plan_candidates` at most (KL_CTX_CAND_MAX of the C ABI)
PLANE_BYTES = 1 << 30       # `Rater.rate_contexts`: device bytes of the [C][characters] f32 planes of one chunk of texts
MIN_T = 3          # shorter windows fall off the persistent scans (engine.HipLM._padded_streams)
ROUND_T = 32       # short-text groups: T is rounded up to a multiple of this


class Call(object):
    """One window call: T, the int64 plan rows [B, 4 + n_ctx] and reset [B] bool -- the rows whose state is zeroed before it."""

    def __init__(self, T, rows, reset):
        self.T, self.rows, self.reset = int(T), rows, reset

    @property
    def B(self):
        return int(self.rows.shape[0])


class Plan(object):
    """What `plan` returns: calls (in order), offsets int64 [n + 1] (text i is corpus[offsets[i]:offsets[i + 1]]), sizes,
    n_ctx, and per text (input order) its row, first call and number of windows (0: no prediction, row -1)."""

    def __init__(self, calls, offsets, sizes, n_ctx, row, first, count):
        self.calls, self.offsets, self.sizes, self.n_ctx = calls, offsets, sizes, n_ctx
        self.row, self.first, self.count = row, first, count

    @property
    def n_calls(self):
        return len(self.calls)

    @property
    def total(self):
        return int(self.offsets[-1])


def _rows(B, n_ctx):
    rows = np.zeros((B, 4 + n_ctx), dtype=np.int64)
    rows[:, 2:4] = -1          # (zero_col, zero_ctx: rating degrades nothing)
    return rows


def plan(sizes, contexts, length, streams):
    """sizes: characters per text; contexts: one (clamped) context list per text; length: the longest window; streams: upper
    limit of rows per call.  Returns a Plan (without calls if no text has a prediction)."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    n = len(sizes)
    length = int(length)
    streams = max(1, int(streams))
    n_ctx = len(contexts[0]) if n else 0
    ctx = np.asarray(contexts, dtype=np.int64).reshape(n, n_ctx)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    preds = np.maximum(sizes - 1, 0)
    row = np.full(n, -1, dtype=np.int64)
    first = np.zeros(n, dtype=np.int64)
    count = -(-preds // length)
    calls = []
    # texts of several windows: list scheduling at T = length, longest first
    long_ = [int(i) for i in np.argsort(-count, kind="stable") if preds[i] > length]
    if long_:
        B = min(streams, len(long_))
        free = np.zeros(B, dtype=np.int64)
        for i in long_:
            r = int(np.argmin(free))
            row[i], first[i] = r, free[r]
            free[r] += count[i]
        for s in range(int(free.max())):
            calls.append(Call(length, _rows(B, n_ctx), np.zeros(B, dtype=bool)))
        for i in long_:
            for w in range(int(count[i])):
                c = calls[int(first[i]) + w]
                done = w * length
                c.rows[row[i], 0] = offsets[i] + done
                c.rows[row[i], 1] = min(length, int(preds[i]) - done)
                c.rows[row[i], 4:] = ctx[i]
                c.reset[row[i]] = w == 0
    # texts of one window: sorted by length, in groups of `streams`, each group as short as its longest text allows
    short = [int(i) for i in np.argsort(preds, kind="stable") if 0 < preds[i] <= length]
    for a in range(0, len(short), streams):
        group = np.array(short[a:a + streams], dtype=np.int64)
        T = -(-int(preds[group].max()) // ROUND_T) * ROUND_T
        T = min(max(T, MIN_T), length)
        rows = _rows(len(group), n_ctx)
        rows[:, 0] = offsets[group]
        rows[:, 1] = preds[group]
        rows[:, 4:] = ctx[group]
        row[group] = np.arange(len(group))
        first[group] = len(calls)
        calls.append(Call(T, rows, np.ones(len(group), dtype=bool)))
    return Plan(calls, offsets, sizes, n_ctx, row, first, count)


def windows_host(corpus, rows, T):
    """what kl_assemble_windows makes of plan rows: (idx [B,T], ctx [B,T,n_ctx], tgt [B,T]) int32; positions outside the
    corpus read as 0"""
    corpus = np.asarray(corpus, dtype=np.int32)
    rows = np.asarray(rows, dtype=np.int64)
    B, n_ctx = rows.shape[0], rows.shape[1] - 4
    t = np.arange(T, dtype=np.int64)[None, :]
    start = rows[:, 0:1]
    vlen = np.clip(rows[:, 1:2], 0, T)
    live = t < vlen

    def read(at):
        ok = (at >= 0) & (at < len(corpus))
        return np.where(ok, corpus[np.where(ok, at, 0)] if len(corpus) else 0, 0)

    zero_col = np.where((rows[:, 2:3] >= 0) & (rows[:, 2:3] < T), rows[:, 2:3], -1)
    idx = np.where(live & (t != zero_col), read(start + t), 0).astype(np.int32)
    tgt = np.where(live, read(start + t + 1), -1).astype(np.int32)
    keep = np.arange(n_ctx)[None, :] != rows[:, 3:4]
    ctx = (live[:, :, None] * (rows[:, 4:] * keep)[:, None, :]).astype(np.int32)
    return idx, ctx, tgt


def scatter_host(tprob, rows, out):
    """what kl_rate_scatter does: out[start + 1 + t] = tprob[b][t] for t < min(vlen, T), inside out; in place, returns out"""
    tprob = np.asarray(tprob)
    B, T = tprob.shape
    n = len(out)
    for b in range(B):
        start, vlen = int(rows[b, 0]), int(min(max(rows[b, 1], 0), T))
        for t in range(vlen):
            g = start + 1 + t
            if 0 <= g < n:
                out[g] = tprob[b, t]
    return out


def scatter_alts_host(tprob, rank, alt_id, alt_p, rows, out_prob, out_rank, out_alt_id, out_alt_p):
    """what kl_rate_scatter_alts does: `scatter_host` for the four results of a call with alternatives -- position
    g = start + 1 + t takes tprob[b][t], rank[b][t] and the K-wide rows alt_id[b][t], alt_p[b][t] for t < min(vlen, T), inside
    the outputs ([n], [n], [n, K], [n, K]); in place, returns the four outputs"""
    tprob = np.asarray(tprob)
    B, T = tprob.shape
    n = len(out_prob)
    for b in range(B):
        start, vlen = int(rows[b, 0]), int(min(max(rows[b, 1], 0), T))
        for t in range(vlen):
            g = start + 1 + t
            if 0 <= g < n:
                out_prob[g] = tprob[b, t]
                out_rank[g] = rank[b, t]
                out_alt_id[g] = alt_id[b, t]
                out_alt_p[g] = alt_p[b, t]
    return out_prob, out_rank, out_alt_id, out_alt_p


def select_host(probs, rank, alt_id, alt_p, max_prob, min_rank):
    """what kl_rate_select computes: the positions j with rank[j] >= min_rank and probs[j] <= float32(max_prob), ascending --
    an f32 comparison: a NaN probability is never selected, and min_rank >= 0 keeps rank -1 (no prediction) out.  Returns
    (pos int64 [m], prob [m], rank [m], alt_id [m, K], alt_p [m, K]), copies of the selected rows."""
    min_rank = int(min_rank)
    limit = np.float32(max_prob)
    if min_rank < 0 or np.isnan(limit):
        raise ValueError("min_rank >= 0 and max_prob not NaN")
    probs, rank, alt_id, alt_p = np.asarray(probs), np.asarray(rank), np.asarray(alt_id), np.asarray(alt_p)
    with np.errstate(invalid="ignore"):
        keep = (rank >= min_rank) & (probs.astype(np.float32, copy=False) <= limit)
    pos = np.nonzero(keep)[0].astype(np.int64)
    return pos, probs[pos], rank[pos], alt_id[pos], alt_p[pos]


def text_bits_host(probs, offsets):
    """what kl_rate_text_bits computes: per text -sum log2(max(p, 1e-99)) over all but its first character, f64"""
    probs = np.asarray(probs)
    out = np.zeros(len(offsets) - 1, dtype=np.float64)
    for i in range(len(out)):
        p = probs[int(offsets[i]) + 1:int(offsets[i + 1])].astype(np.float64)
        if len(p):
            out[i] = -np.log2(np.maximum(p, 1e-99)).sum()
    return out


def variant_windows_host(corpus, offsets, text_ctx, sel_pos, sel_alt_id, left, ahead, deletions, T, insertions=0):
    """what kl_variant_windows (kl_edit_windows with insertions) makes of S suspects (sel_pos [S] corpus positions, sel_alt_id
    [S, K] their alternatives): the R = K + 1 + deletions + K * insertions hypothesis rows of each, row b = s * R + v.  For g = sel_pos[s] in text i (offsets[i] <= g <
    offsets[i + 1]), w = corpus[g], L = min(left, g - offsets[i]), A = min(ahead, offsets[i + 1] - 1 - g):
      v = 0       q = x[g-L .. g-1], w, x[g+1 .. g+A]           invalid if L == 0 or g is in no text or beyond the corpus
      v = 1 .. K  the same with a = sel_alt_id[s][v-1] for w    invalid if v = 0 is, or a < 0, or a == w
      v = K + 1   q = x[g-L .. g-1], x[g+1 .. g+A]              (deletions only) invalid if v = 0 is, or A == 0
      v = K + 1 + deletions + j, j = 0 .. K-1  (insertions only: a character the text has lost in front of the suspect)
                  q = x[g-L .. g-1], a, w, x[g+1 .. g+A]        with a = sel_alt_id[s][j], len = L + 2 + A; invalid if v = 0
                                                                is, or a < 0 -- a == w (a doubled character that lost its
                                                                twin) and the unmapped id 0 are valid
    A valid row: idx[t] = q[t] for t < len - 1, else 0; tgt[t] = q[t+1] for L - 1 <= t < len - 1, else -1; ctx[t] =
    text_ctx[i] for t < len - 1, else 0 -- a window from a zero state over an insertion row predicts a, then w, then the A
    characters after it.  An invalid row is a dummy stream (idx 0, ctx 0, tgt -1).  text_ctx: [n_texts, n_ctx] (None: no
    contexts).  Positions outside [0, min(len(corpus), offsets[-1])) read as 0.  A fed row is up to left + ahead + insertions
    long: left + ahead + insertions <= T <= 1024.  The rows v <= K + deletions do not depend on `insertions`.
    Returns (idx [S*R, T], ctx [S*R, T, n_ctx], tgt [S*R, T], valid [S*R]) int32."""
    corpus = np.asarray(corpus, dtype=np.int32).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    g = np.asarray(sel_pos, dtype=np.int64).reshape(-1)
    alts = np.asarray(sel_alt_id, dtype=np.int32)
    S, K = alts.shape
    left, ahead, deletions, T, insertions = int(left), int(ahead), int(deletions), int(T), int(insertions)
    n_texts = len(offsets) - 1
    if (S != len(g) or S < 1 or n_texts < 1 or K < 1 or left < 1 or ahead < 0 or deletions not in (0, 1)
            or insertions not in (0, 1) or not left + ahead + insertions <= T <= 1024):
        raise ValueError("variant_windows_host: S, n_texts, K, left >= 1, ahead >= 0, deletions and insertions in {0, 1}, "
                         "left + ahead + insertions <= T <= 1024")
    text_ctx = np.zeros((n_texts, 0), dtype=np.int32) if text_ctx is None else np.asarray(text_ctx, dtype=np.int32)
    text_ctx = text_ctx.reshape(n_texts, -1)
    R = K + 1 + deletions + K * insertions
    limit = min(len(corpus), int(offsets[-1]))

    def read(at):
        ok = (at >= 0) & (at < limit)
        return np.where(ok, corpus[np.where(ok, at, 0)] if len(corpus) else 0, 0).astype(np.int32)

    # the text of g: the last i with offsets[i] <= g (repeated offsets -- empty texts -- lie in front of it)
    i = np.searchsorted(offsets, g, side="right") - 1
    found = (g >= 0) & (g < limit) & (i >= 0)
    i = np.clip(i, 0, n_texts - 1)
    L = np.where(found, np.minimum(left, g - offsets[i]), 0)
    A = np.where(found, np.minimum(ahead, offsets[i + 1] - 1 - g), 0)
    base = found & (L >= 1)
    w = read(g)
    # per variant [S, R]: the character at q[L] (if the variant has one of its own), how many characters stand for the
    # suspect (0 dropped, 1, 2 with one inserted in front of it) and whether the row is valid
    char = np.concatenate([w[:, None], alts] + ([np.zeros((S, 1), dtype=np.int32)] if deletions else [])
                          + ([alts] if insertions else []), axis=1)
    has = np.ones(R, dtype=np.int64)
    valid = np.empty((S, R), dtype=bool)
    valid[:, 0] = base
    valid[:, 1:K + 1] = base[:, None] & (alts >= 0) & (alts != w[:, None])
    if deletions:
        has[K + 1] = 0
        valid[:, K + 1] = base & (A > 0)
    if insertions:
        has[K + 1 + deletions:] = 2
        valid[:, K + 1 + deletions:] = base[:, None] & (alts >= 0)
    t = np.arange(T + 1, dtype=np.int64)[None, None, :]
    L3, g3 = L[:, None, None], g[:, None, None]
    has3 = has[None, :, None]
    length = L3 + has3 + A[:, None, None]
    # from t = L on the corpus is read one ahead (the character dropped) or one behind (one inserted in front of it)
    q = read(g3 - L3 + t + (1 - has3) * (t >= L3))
    q = np.where((has3 >= 1) & (t == L3), char[:, :, None], q)
    fed = valid[:, :, None] & (t[:, :, :T] < length - 1)
    idx = np.where(fed, q[:, :, :T], 0).astype(np.int32)
    tgt = np.where(fed & (t[:, :, :T] >= L3 - 1), q[:, :, 1:], -1).astype(np.int32)
    ctx = (fed[:, :, :, None] * text_ctx[i][:, None, None, :]).astype(np.int32)
    return (idx.reshape(S * R, T), ctx.reshape(S * R, T, text_ctx.shape[1]), tgt.reshape(S * R, T),
            valid.reshape(S * R).astype(np.int32))


def prefix_windows_host(corpus, offsets, text_ctx, sel_pos, left, T):
    """what kl_prefix_windows makes of S suspects (sel_pos [S] corpus positions): the left context of each as a row of its own,
    read once for all its variants.  For g = sel_pos[s] in text i (offsets[i] <= g < offsets[i + 1]) the row is valid iff g lies
    in a text, inside [0, min(len(corpus), offsets[-1])), and g - offsets[i] >= left -- the suspects whose
    `variant_windows_host` rows have L == left.  A valid row: idx[t] = x[g - left + t] for t < left - 1, else 0; ctx[t] =
    text_ctx[i] for t < left - 1, else 0; tgt[t] = -1 everywhere -- a window from a zero state over it predicts nothing and
    leaves the state after x[g-left .. g-2]; the rows of `variant_windows_host(left=1)`, which feed x[g-1] first, continue from
    it (`fan_states_host`).  An invalid row is a dummy stream (idx 0, ctx 0, tgt -1).  text_ctx: [n_texts, n_ctx] (None: no
    contexts).  left >= 2, left - 1 <= T <= 1024.
    Returns (idx [S, T], ctx [S, T, n_ctx], tgt [S, T], valid [S]) int32."""
    corpus = np.asarray(corpus, dtype=np.int32).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    g = np.asarray(sel_pos, dtype=np.int64).reshape(-1)
    S, left, T = len(g), int(left), int(T)
    n_texts = len(offsets) - 1
    if S < 1 or n_texts < 1 or left < 2 or not left - 1 <= T <= 1024:
        raise ValueError("prefix_windows_host: S, n_texts >= 1, left >= 2, left - 1 <= T <= 1024")
    text_ctx = np.zeros((n_texts, 0), dtype=np.int32) if text_ctx is None else np.asarray(text_ctx, dtype=np.int32)
    text_ctx = text_ctx.reshape(n_texts, -1)
    limit = min(len(corpus), int(offsets[-1]))
    # the text of g: the last i with offsets[i] <= g (repeated offsets -- empty texts -- lie in front of it)
    i = np.searchsorted(offsets, g, side="right") - 1
    found = (g >= 0) & (g < limit) & (i >= 0)
    i = np.clip(i, 0, n_texts - 1)
    valid = found & (g - offsets[i] >= left)
    t = np.arange(T, dtype=np.int64)[None, :]
    fed = valid[:, None] & (t < left - 1)
    at = g[:, None] - left + t      # (inside the text wherever the row is fed)
    idx = np.where(fed, corpus[np.where(fed, at, 0)] if len(corpus) else 0, 0).astype(np.int32)
    ctx = (fed[:, :, None] * text_ctx[i][:, None, :]).astype(np.int32)
    return idx, ctx, np.full((S, T), -1, dtype=np.int32), valid.astype(np.int32)


def fan_states_host(states, parent):
    """what kl_state_fanout does: row b of the result is row parent[b] of `states`, a row of zeros where parent[b] is outside
    [0, number of rows).  states: one array with the streams on axis 0 (the HIP engine's [B, 2 depth, width]), or a list of
    such arrays (an engine that keeps h and c per layer apart: [B, width] each) -- the result has the same form, copies."""
    parent = np.asarray(parent, dtype=np.int64).reshape(-1)

    def fan(a):
        a = np.asarray(a)
        inside = (parent >= 0) & (parent < a.shape[0])
        out = np.zeros((len(parent),) + a.shape[1:], dtype=a.dtype)
        out[inside] = a[parent[inside]]
        return out

    return [fan(a) for a in states] if isinstance(states, (list, tuple)) else fan(states)


def left_groups(sel_pos, offsets, left):
    """the suspects of `Rater.corrections(share_left=True)` in two groups: (full, short), ascending int64 indices into sel_pos
    [S] -- full where the whole of `left` characters stands in front of the suspect in its text (L == left: the rows
    `prefix_windows_host` calls valid), short all the others (L < left, and what lies in no text)."""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    g = np.asarray(sel_pos, dtype=np.int64).reshape(-1)
    i = np.searchsorted(offsets, g, side="right") - 1
    inside = (g >= 0) & (g < offsets[-1]) & (i >= 0)
    whole = inside & (g - offsets[np.clip(i, 0, len(offsets) - 2)] >= int(left))
    return np.nonzero(whole)[0].astype(np.int64), np.nonzero(~whole)[0].astype(np.int64)


def prefix_batches(n_full, streams, R):
    """the full group of `left_groups` (n_full suspects of R variants each) cut for windows of at most `streams` rows: suffix
    chunks of chunk = max(1, streams // R) suspects -- chunk * R hypothesis rows --, and prefix batches of
    Pc = max(1, streams // chunk) * chunk suspects, one prefix row each, so that a batch is a whole number of chunks (but for
    the last).  Returns [(a, b, [(c, d), ..])]: batch [a, b) and its chunks [c, d), a <= c < d <= b."""
    chunk = max(1, int(streams) // int(R))
    Pc = max(1, int(streams) // chunk) * chunk
    return [(a, min(a + Pc, n_full), [(c, min(c + chunk, a + Pc, n_full)) for c in range(a, min(a + Pc, n_full), chunk)])
            for a in range(0, int(n_full), Pc)]


def variant_pick_host(cost, valid):
    """the choice among a suspect's variants: cost [S, R] f64 (bits of the text around the suspect under variant v; v = 0 is
    the text as written), valid [S, R].  Returns (cost with +inf where invalid, best [S] int32, gain [S] f64): best is the
    valid v >= 1 of least cost, the smallest such v among equal costs, 0 if there is none; gain = cost[0] - cost[best] in bits
    (negative where every variant reads worse than what was written), 0.0 where best is 0.  Generic in R: with the rows of
    `variant_windows_host` the tie rule orders substitution < deletion < insertion, and within a kind by alternative rank."""
    cost = np.array(cost, dtype=np.float64, copy=True)
    valid = np.asarray(valid).astype(bool)
    S, R = cost.shape
    assert valid.shape == (S, R)
    cost[~valid] = np.inf
    best = np.zeros(S, dtype=np.int32)
    gain = np.zeros(S, dtype=np.float64)
    if S and R > 1:
        rest = cost[:, 1:]
        first = np.argmin(rest, axis=1)                 # (argmin: the first of equal minima)
        any_valid = valid[:, 0] & valid[:, 1:].any(axis=1)
        best[any_valid] = first[any_valid] + 1
        rows = np.nonzero(any_valid)[0]
        gain[rows] = cost[rows, 0] - cost[rows, best[rows]]
    return cost, best, gain


SPAN_LEN_MAX = 64      # ids of a span and of a candidate at most (KL_SPAN_LEN_MAX of the C ABI)


def span_windows_host(corpus, offsets, text_ctx, span_text, span_start, span_len, span_first, pool, cand_off, row0, rows, left,
                      ahead, max_len, T):
    """what kl_span_windows makes of S spans with caller-supplied replacements: span s replaces the D = span_len[s] >= 0 written
    characters at corpus position g = span_start[s] of text i = span_text[s] (D = 0: an insertion in front of g) and owns the
    candidates span_first[s] .. span_first[s+1]-1 (span_first [S + 1] ascending from 0 to C; a span may own none); candidate c
    is the id string r = pool[cand_off[c] .. cand_off[c+1]-1] (cand_off [C + 1] ascending) of any length m >= 0 (0: the span
    dropped).  Rows are numbered over all spans, N = S + C: span s has rows span_first[s] + s .. span_first[s+1] + s, the first
    the text as written (r = w = x[g .. g+D-1]), then its candidates in order; the call builds rows row0 .. row0 + rows - 1.
    With n_read = min(len(corpus), offsets[-1]), M = max_len, L = min(left, g - offsets[i]), A = min(ahead, offsets[i+1] - g - D):
      span base      0 <= i < n_texts, 0 <= D <= M, offsets[i] <= g, g + D <= min(offsets[i+1], n_read), L >= 1
      written row    valid iff the base holds and D + A >= 1
      candidate row  valid iff the written row is, 0 <= m <= M, every id of r is >= 0, m + A >= 1 and r != w as id strings (two
                     different unmapped characters are both id 0 and count as equal); a candidate whose range does not lie
                     inside the pool, or whose index is not in [0, C), is invalid
    A valid row has q = x[g-L .. g-1], r, x[g+D .. g+D+A-1], len = L + m + A, and `variant_windows_host`'s rule per word:
    idx[t] = q[t] for t < len - 1, else 0; tgt[t] = q[t+1] for L - 1 <= t < len - 1, else -1; ctx[t] = text_ctx[i] for
    t < len - 1, else 0.  An invalid row is a dummy stream (idx 0, ctx 0, tgt -1).  text_ctx: [n_texts, n_ctx] (None: no
    contexts).  Positions outside [0, n_read) read as 0.  1 <= M <= 64, left + ahead + M - 1 <= T <= 1024.
    Returns (idx [rows, T], ctx [rows, T, n_ctx], tgt [rows, T], valid [rows]) int32."""
    corpus = np.asarray(corpus, dtype=np.int32).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    span_text = np.asarray(span_text, dtype=np.int64).reshape(-1)
    span_start = np.asarray(span_start, dtype=np.int64).reshape(-1)
    span_len = np.asarray(span_len, dtype=np.int64).reshape(-1)
    span_first = np.asarray(span_first, dtype=np.int64).reshape(-1)
    pool = np.asarray(pool, dtype=np.int32).reshape(-1)
    cand_off = np.asarray(cand_off, dtype=np.int64).reshape(-1)
    S, C = len(span_first) - 1, len(cand_off) - 1
    row0, rows, left, ahead, M, T = int(row0), int(rows), int(left), int(ahead), int(max_len), int(T)
    n_texts = len(offsets) - 1
    if (S < 1 or C < 0 or n_texts < 1 or not len(span_text) == len(span_start) == len(span_len) == S or rows < 1 or row0 < 0
            or row0 + rows > S + C or left < 1 or ahead < 0 or not 1 <= M <= SPAN_LEN_MAX
            or not left + ahead + M - 1 <= T <= 1024):
        raise ValueError("span_windows_host: S, n_texts, rows >= 1, 0 <= row0, row0 + rows <= S + C, left >= 1, ahead >= 0, "
                         "1 <= max_len <= 64, left + ahead + max_len - 1 <= T <= 1024")
    text_ctx = np.zeros((n_texts, 0), dtype=np.int32) if text_ctx is None else np.asarray(text_ctx, dtype=np.int32)
    text_ctx = text_ctx.reshape(n_texts, -1)
    n_read = min(len(corpus), int(offsets[-1]))

    def read(at):
        ok = (at >= 0) & (at < n_read)
        return np.where(ok, corpus[np.where(ok, at, 0)] if len(corpus) else 0, 0).astype(np.int32)

    # the span of row b: the last s with span_first[s] + s <= b; v = 0 is the text as written, else candidate v - 1 of the span
    b = row0 + np.arange(rows, dtype=np.int64)
    keys = span_first[:S] + np.arange(S, dtype=np.int64)
    s = np.searchsorted(keys, b, side="right") - 1
    found = s >= 0
    s = np.maximum(s, 0)
    v = b - keys[s]
    written = v == 0
    i, g, D = span_text[s], span_start[s], span_len[s]
    ok = found & (i >= 0) & (i < n_texts) & (D >= 0) & (D <= M)
    i = np.clip(i, 0, n_texts - 1)
    o0, o1 = offsets[i], offsets[i + 1]
    lim = np.minimum(o1, n_read)
    ok &= (o0 <= g) & (g <= lim)
    ok &= D <= np.where(ok, lim - g, -1)
    L = np.where(ok, np.minimum(left, g - o0), 0)
    A = np.where(ok, np.minimum(ahead, o1 - g - D), 0)
    ok &= (L >= 1) & (D + A >= 1)
    # the candidate's range in the pool
    c = span_first[s] + v - 1
    known = ~written & (c >= 0) & (c < C)
    c = np.clip(c, 0, max(C - 1, 0))
    ends = np.concatenate([cand_off, cand_off[-1:]])
    lo, hi = ends[c], ends[c + 1]
    known &= (lo >= 0) & (hi >= lo) & (hi - lo <= M) & (hi <= len(pool))
    m = np.where(written, D, np.where(known, hi - lo, 0))
    ok &= written | (known & (m + A >= 1))
    m = np.where(ok, m, 0)
    # r [rows, M]: the written characters, or the candidate's ids
    k = np.arange(M, dtype=np.int64)[None, :]
    w = read(g[:, None] + k)
    at = np.clip(lo[:, None] + k, 0, max(len(pool) - 1, 0))
    own = pool[at] if len(pool) else np.zeros((rows, M), dtype=np.int32)
    r = np.where(written[:, None], w, own)
    inside = k < m[:, None]
    negative = (inside & (r < 0)).any(axis=1)
    differs = (m != D) | (inside & (r != w)).any(axis=1)
    ok &= written | (~negative & differs)
    m = np.where(ok, m, 0)
    # q [rows, T + 1]
    t = np.arange(T + 1, dtype=np.int64)[None, :]
    L2, m2, g2, D2 = L[:, None], m[:, None], g[:, None], D[:, None]
    length = np.where(ok, L + m + A, 0)[:, None]
    q = np.where(t < L2, read(g2 - L2 + t), read(g2 + D2 + t - L2 - m2))
    q = np.where((t >= L2) & (t < L2 + m2), np.take_along_axis(r, np.clip(t - L2, 0, M - 1), axis=1), q)
    fed = ok[:, None] & (t[:, :T] < length - 1)
    idx = np.where(fed, q[:, :T], 0).astype(np.int32)
    tgt = np.where(fed & (t[:, :T] >= L2 - 1), q[:, 1:], -1).astype(np.int32)
    ctx = (fed[:, :, None] * text_ctx[i][:, None, :]).astype(np.int32)
    return idx, ctx, tgt, ok.astype(np.int32)


def span_pick_host(cost, valid, span_first, min_gain):
    """what kl_span_pick computes: cost [S + C] f64 and valid [S + C] per row of `span_windows_host`'s numbering, span_first
    [S + 1].  Returns (best [S] int32, gain [S] f64, cost with +inf where invalid): best is the index j within the span's
    candidates of the valid candidate of least cost, the smallest j among equal costs (a NaN cost is never chosen);
    gain = cost[written] - cost[best]; best = -1 and gain = 0.0 where the written row is invalid, where no candidate is valid,
    or where not gain >= min_gain -- `variant_pick_host`'s rule plus `Rater.corrections`' drop rule, generic in the count."""
    cost = np.array(cost, dtype=np.float64, copy=True).reshape(-1)
    valid = np.asarray(valid).reshape(-1) != 0
    span_first = np.asarray(span_first, dtype=np.int64).reshape(-1)
    S = len(span_first) - 1
    C = int(span_first[-1]) if S >= 0 else 0
    if S < 1 or span_first[0] != 0 or (np.diff(span_first) < 0).any() or len(cost) != S + C or len(valid) != S + C:
        raise ValueError("span_pick_host: span_first [S + 1] ascending from 0 to C, cost and valid [S + C]")
    count = np.diff(span_first)
    written = span_first[:S] + np.arange(S, dtype=np.int64)
    best = np.full(S, -1, dtype=np.int32)
    gain = np.zeros(S, dtype=np.float64)
    if C:
        sid = np.repeat(np.arange(S, dtype=np.int64), count)
        j = np.arange(C, dtype=np.int64) - span_first[sid]
        row = written[sid] + 1 + j
        out = ~(valid[row] & ~np.isnan(cost[row]))
        key = np.where(out, 0.0, cost[row])
        order = np.lexsort((j, key, out, sid))      # per span: the candidates that may be chosen first, by (cost, j)
        has = np.nonzero(count > 0)[0]
        first = order[span_first[has]]
        some = ~out[first] & valid[written[has]]
        has, first = has[some], first[some]
        with np.errstate(invalid="ignore"):
            saved = cost[written[has]] - cost[row[first]]
            keep = saved >= float(min_gain)
        best[has[keep]] = j[first[keep]]
        gain[has[keep]] = saved[keep]
    cost[~valid] = np.inf
    return best, gain, cost


def span_chunks(span_first, streams):
    """the row space of S spans (`span_windows_host`'s numbering) cut for `Rater.rescore`: consecutive whole spans while the
    chunk has at most `streams` rows, a span with more rows than that a chunk of its own.  Returns [(row0, row1)]."""
    span_first = np.asarray(span_first, dtype=np.int64).reshape(-1)
    S = len(span_first) - 1
    keys = span_first + np.arange(S + 1, dtype=np.int64)      # the first row of every span, and the number of rows
    streams = max(1, int(streams))
    out = []
    a = 0
    while a < S:
        b = max(a + 1, int(np.searchsorted(keys, keys[a] + streams, side="right")) - 1)
        out.append((int(keys[a]), int(keys[b])))
        a = b
    return out


def plan_candidates(sizes, candidates, length, streams):
    """`plan` for every text under every one of C candidate contexts: its rules over the n * C virtual texts v = i * C + c, a
    virtual text having the size and the corpus start of text i and the (clamped) context candidates[c].  The rows point into
    the shared corpus of the n texts -- kl_assemble_windows serves unchanged --, so a row's start does not tell its candidate:
    that is `plane`.  Returns (Plan, planes): the Plan has offsets and sizes of the n texts, and row, first and count per
    virtual text [n * C]; planes[s] is int32 [B] for call s, the candidate of every row, -1 for a row with nothing to do.
    With C = 1 the calls are `plan`'s, row for row."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    n, C = len(sizes), len(candidates)
    if not 1 <= C <= CTX_CAND_MAX:
        raise ValueError("1 .. %d candidate contexts (got %d)" % (CTX_CAND_MAX, C))
    cand = np.asarray(candidates, dtype=np.int64).reshape(C, -1)
    virtual = plan(np.repeat(sizes, C), np.tile(cand, (n, 1)), length, streams)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    shift = np.repeat(offsets[:-1], C) - virtual.offsets[:-1]      # (from a virtual text's own start to its text's)
    planes = [np.full(c.B, -1, dtype=np.int32) for c in virtual.calls]
    # every window of every virtual text: (call, row), grouped by call
    count = np.where(virtual.row >= 0, virtual.count, 0)
    v = np.repeat(np.arange(n * C, dtype=np.int64), count)
    w = np.arange(len(v), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    call = virtual.first[v] + w
    order = np.argsort(call, kind="stable")
    cut = np.searchsorted(call[order], np.arange(len(virtual.calls) + 1), side="left")
    for s, one in enumerate(virtual.calls):
        mine = v[order[cut[s]:cut[s + 1]]]
        rows = virtual.row[mine]
        one.rows[rows, 0] += shift[mine]
        planes[s][rows] = mine % C
    return Plan(virtual.calls, offsets, sizes, virtual.n_ctx, virtual.row, virtual.first, virtual.count), planes


def text_chunks(sizes, limit):
    """texts in input order cut for `Rater.rate_contexts`: consecutive whole texts while the chunk has at most `limit`
    characters, a single larger text a chunk of its own.  Returns [(first text, end)], covering every text; [] for no text."""
    ends = np.cumsum(np.asarray(sizes, dtype=np.int64).reshape(-1))
    limit = max(1, int(limit))
    out = []
    a = 0
    while a < len(ends):
        done = int(ends[a - 1]) if a else 0
        b = max(a + 1, int(np.searchsorted(ends, done + limit, side="right")))
        out.append((a, b))
        a = b
    return out


def scatter_planes_host(tprob, rows, plane, out, n_out=None):
    """what kl_rate_scatter_planes does: `scatter_host` with a destination plane per row -- out [C, ld]:
    out[plane[b], start + 1 + t] = tprob[b][t] for t < min(vlen, T), inside [0, n_out) (n_out <= ld; None: ld); a row whose
    plane is outside [0, C) writes nothing; in place, returns out"""
    tprob = np.asarray(tprob)
    B, T = tprob.shape
    C, ld = out.shape
    n = ld if n_out is None else int(n_out)
    assert n <= ld
    for b in range(B):
        c = int(plane[b])
        if not 0 <= c < C:
            continue
        start, vlen = int(rows[b, 0]), int(min(max(rows[b, 1], 0), T))
        for t in range(vlen):
            g = start + 1 + t
            if 0 <= g < n:
                out[c, g] = tprob[b, t]
    return out


def context_mix_host(planes, offsets, log2prior=None, mix=None):
    """what kl_context_mix computes from planes [C, ld] f32 (candidate c's probabilities in corpus order), offsets [n + 1] and
    log2prior [C] f64 (None: uniform, every entry 0; finite entries or -inf, one finite).  For text i and its predicted
    positions j = max(offsets[i] + 1, 1) .. min(offsets[i + 1], ld) - 1, ascending, sequential f64:
      q_c[j] = np.fmax(planes[c, j], 1e-99) (a NaN counts as 1e-99);  lw_c(j) = log2prior[c] + sum_{j' < j} log2 q_c[j'];
      w_c = exp2(lw_c(j) - max_c lw_c(j)), 0 where lw_c(j) is -inf;  r[j] = sum_c w_c q_c[j] / sum_c w_c.
    mix (f32 [ld] or None) takes float32(r[j]) at these positions, in place; nothing else of it is written.  Returns
    (cand_bits [n, C] = -sum_j log2 q_c[j], mix_bits [n] = -sum_j log2 r[j], post [n, C], best [n] int32, margin [n]) -- with
    the final lw_c (the prior for a text without predictions): post = w_c / sum w, best the smallest c of maximal lw_c, margin
    lw_best minus the largest lw of the others, +inf where none of them is finite.  Without a finite prior entry: mix, mix_bits
    and post are NaN, best 0, margin +inf."""
    planes = np.asarray(planes)
    C, ld = planes.shape
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    n = len(offsets) - 1
    prior = np.zeros(C, dtype=np.float64) if log2prior is None else np.asarray(log2prior, dtype=np.float64).reshape(C)
    cand_bits = np.zeros((n, C), dtype=np.float64)
    mix_bits = np.zeros(n, dtype=np.float64)
    post = np.zeros((n, C), dtype=np.float64)
    best = np.zeros(n, dtype=np.int32)
    margin = np.zeros(n, dtype=np.float64)

    def weights(lw):      # [C, m] -> the weights and their sequential sum over c
        with np.errstate(invalid="ignore"):
            w = np.where(np.isneginf(lw), 0.0, np.exp2(lw - lw.max(axis=0)))
        return w, np.add.accumulate(w, axis=0)[-1]

    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            a, b = max(int(offsets[i]) + 1, 1), min(int(offsets[i + 1]), ld)
            sums = np.zeros(C, dtype=np.float64)
            if b > a:
                q = np.fmax(planes[:, a:b].astype(np.float64), 1e-99)
                run = np.add.accumulate(np.log2(q), axis=1)      # (sequential along the text)
                sums = run[:, -1]
                lw = prior[:, None] + np.concatenate([np.zeros((C, 1)), run[:, :-1]], axis=1)
                w, total = weights(lw)
                r = np.add.accumulate(w * q, axis=0)[-1] / total
                if mix is not None:
                    mix[a:b] = r.astype(np.float32)
                mix_bits[i] = -np.add.accumulate(np.log2(r))[-1]
            cand_bits[i] = 0.0 - sums
            lw = prior + sums
            w, total = weights(lw[:, None])
            post[i] = w[:, 0] / total[0]
            best[i] = int(np.argmax(lw))      # (the first of equal maxima)
            rest = np.delete(lw, best[i])
            second = rest.max() if len(rest) else -np.inf
            margin[i] = np.inf if np.isneginf(second) else lw[best[i]] - second
    return cand_bits, mix_bits, post, best, margin


def word_bounds_host(corpus, offsets, delim):
    """what kl_word_bounds computes: the words of the texts as (seg_start, seg_end) int64, ascending, [start, end) in corpus
    positions.  corpus [n] ids, offsets [n_texts + 1] ascending (repeated values: empty texts), delim [V] nonzero for the ids that
    separate words.  With lo = max(offsets[0], 0) and hi = min(n, offsets[n_texts]): position j is a character iff
    lo <= j < hi and not (0 <= corpus[j] < V and delim[corpus[j]] != 0) -- an id outside the table is a character --, it is a
    text's first iff j == offsets[i] for some i; a word starts at a character that is a first or follows no character, and ends
    behind a character that is the last below hi, or is followed by a first or by no character.  A word never crosses a text
    boundary."""
    corpus = np.asarray(corpus).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    delim = np.asarray(delim).reshape(-1)
    n, V = len(corpus), len(delim)
    if len(offsets) < 2 or V < 1:
        raise ValueError("word_bounds_host: one text and one table entry at least")
    lo, hi = max(int(offsets[0]), 0), min(n, int(offsets[-1]))
    char = np.zeros(n + 2, dtype=bool)           # (char[j + 1] is position j: one position of no character on either side)
    first = np.zeros(n + 2, dtype=bool)
    if hi > lo:
        ids = corpus[lo:hi].astype(np.int64)
        known = (ids >= 0) & (ids < V)
        char[lo + 1:hi + 1] = ~(known & (delim[np.where(known, ids, 0)] != 0))
    inside = offsets[(offsets >= 0) & (offsets <= n)]
    first[inside + 1] = True
    here, before, after = char[1:n + 1], char[0:n], char[2:n + 2]
    start = here & (first[1:n + 1] | ~before)
    end = here & (first[2:n + 2] | ~after)        # (hi itself is no character: the last one below it ends a word)
    return np.nonzero(start)[0].astype(np.int64), np.nonzero(end)[0].astype(np.int64) + 1


def segments_host(probs, rank, offsets, seg_start, seg_end, max_prob=0.0, min_rank=0):
    """what kl_rate_segments computes over probs [n] f32 and rank [n] int32 (or None) in corpus order: per segment s =
    [seg_start[s], seg_end[s]) -- any order, overlap allowed -- of the text i with offsets[i] <= seg_start[s] < offsets[i + 1]
    (empty texts are skipped), over its counted positions j in [max(a, offsets[i] + 1), min(b, offsets[i + 1], n)) (none where
    a < 0, b < a, a lies in no text or a >= n), sequentially in f64:
      seg_n int32, seg_bits = -sum log2(np.fmax(probs[j], 1e-99)) (a NaN counts as 1e-99), seg_psum = sum probs[j] (a NaN as it
      is), seg_min f32 the least probs[j] under `<` (a bit copy; a NaN is never it) and seg_worst int64 its j, the smallest among
      equal values -- +inf and -1 where nothing is counted or nothing counted lies below +inf --, seg_bad int32 the counted j
      with rank[j] >= min_rank and probs[j] <= float32(max_prob) (0 without rank).
    Returns (seg_n, seg_bits, seg_psum, seg_min, seg_worst, seg_bad)."""
    min_rank = int(min_rank)
    limit = np.float32(max_prob)
    if min_rank < 0 or np.isnan(limit):
        raise ValueError("min_rank >= 0 and max_prob not NaN")
    probs = np.asarray(probs, dtype=np.float32).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    seg_start = np.asarray(seg_start, dtype=np.int64).reshape(-1)
    seg_end = np.asarray(seg_end, dtype=np.int64).reshape(-1)
    n, n_texts, S = len(probs), len(offsets) - 1, len(seg_start)
    if n_texts < 1 or len(seg_end) != S:
        raise ValueError("segments_host: one text at least, and one end per start")
    with np.errstate(invalid="ignore", divide="ignore"):
        logs = -np.log2(np.fmax(probs.astype(np.float64), 1e-99))
        bad = np.zeros(n, dtype=bool) if rank is None else (np.asarray(rank).reshape(-1) >= min_rank) & (probs <= limit)
    text = np.searchsorted(offsets, seg_start, side="right") - 1      # (the largest i with offsets[i] <= a)
    seg_n = np.zeros(S, dtype=np.int32)
    seg_bits = np.zeros(S, dtype=np.float64)
    seg_psum = np.zeros(S, dtype=np.float64)
    seg_min = np.full(S, np.inf, dtype=np.float32)
    seg_worst = np.full(S, -1, dtype=np.int64)
    seg_bad = np.zeros(S, dtype=np.int32)
    for s in range(S):
        a, b, i = int(seg_start[s]), int(seg_end[s]), int(text[s])
        if a < 0 or b < a or a >= n or not 0 <= i < n_texts:
            continue
        lo, hi = max(a, int(offsets[i]) + 1), min(b, int(offsets[i + 1]), n)
        if hi <= lo:
            continue
        p = probs[lo:hi]
        seg_n[s] = hi - lo
        seg_bits[s] = np.add.accumulate(logs[lo:hi])[-1]
        seg_psum[s] = np.add.accumulate(p.astype(np.float64))[-1]
        seg_bad[s] = int(bad[lo:hi].sum())
        least = np.fmin.reduce(p)                 # (np.fmin passes a NaN over)
        if least < np.inf:
            at = int(np.argmax(p == least))       # (the first of equal values)
            seg_min[s], seg_worst[s] = p[at], lo + at
    return seg_n, seg_bits, seg_psum, seg_min, seg_worst, seg_bad


def segment_select_host(seg_start, seg_end, seg_n, seg_bits, seg_psum, seg_min, seg_worst, seg_bad, min_n=1, min_bad=1,
                        min_bpc=0.0):
    """what kl_segment_select computes: the segments s with seg_n[s] >= min_n, seg_bad[s] >= min_bad and
    seg_bits[s] >= min_bpc * float64(seg_n[s]), ascending -- equality selects, NaN bits never do.  Returns (index int64 [m],
    start, end, n, bits, psum, min, worst, bad): copies of the selected records."""
    min_n, min_bad, min_bpc = int(min_n), int(min_bad), float(min_bpc)
    if min_n < 1 or min_bad < 0 or not min_bpc >= 0.0:
        raise ValueError("min_n >= 1, min_bad >= 0 and min_bpc >= 0, not NaN")
    records = [np.asarray(a).reshape(-1) for a in (seg_start, seg_end, seg_n, seg_bits, seg_psum, seg_min, seg_worst, seg_bad)]
    n, bits, bad = records[2], records[3], records[7]
    with np.errstate(invalid="ignore"):
        keep = (n >= min_n) & (bad >= min_bad) & (bits.astype(np.float64) >= min_bpc * n.astype(np.float64))
    index = np.nonzero(keep)[0].astype(np.int64)
    return (index,) + tuple(a[index] for a in records)


LEXICON_V_MAX, LEXICON_DIST_MAX, LEXICON_K_MAX = 4096, 8, 16      # (KL_LEXICON_* of the C ABI)


def lexicon_layout_host(pool, off):
    """the device layout of a lexicon for kl_lexicon_neighbours: pool int32 ids and off int64 [N + 1] are the N entries in the
    caller's order -- the priority order, the most frequent entry first.  Returns (chars, order, class_first):
      order        int32 [N']  the original indices of the entries of 1 .. SPAN_LEN_MAX ids, sorted by (length, original
                               index); entries of no ids or of more are left out -- they are neighbours of nothing;
      class_first  int64 [66]  the entries of length L are the sorted positions [class_first[L], class_first[L + 1]);
                               class_first[0] = class_first[1] = 0, class_first[65] = N';
      chars        int32       column-major within a length class: with n_L entries in class L and base[L] = sum over l < L of
                               l * n_l, id j of sorted position p of class L is chars[base[L] + j * n_L + (p - class_first[L])]
                               -- consecutive lanes read consecutive addresses."""
    pool = np.asarray(pool, dtype=np.int32).reshape(-1)
    off = np.asarray(off, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > len(pool):
        raise ValueError("lexicon_layout_host: off [N + 1] ascending within the pool")
    length = np.diff(off)
    kept = np.nonzero((length >= 1) & (length <= SPAN_LEN_MAX))[0]
    order = kept[np.argsort(length[kept], kind="stable")].astype(np.int32)      # (stable: ascending index within a class)
    class_first = np.zeros(SPAN_LEN_MAX + 2, dtype=np.int64)
    class_first[1:] = np.searchsorted(length[order], np.arange(1, SPAN_LEN_MAX + 2), side="left")
    parts = []
    for L in range(1, SPAN_LEN_MAX + 1):
        a, b = int(class_first[L]), int(class_first[L + 1])
        if b > a:
            rows = pool[off[order[a:b]][:, None] + np.arange(L)[None, :]]      # [n_L, L]
            parts.append(np.ascontiguousarray(rows.T).reshape(-1))
    chars = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return chars, order, class_first


def lexicon_neighbours_host(q_pool, q_off, chars, order, class_first, V, max_dist, K):
    """what kl_lexicon_neighbours computes: for the Q queries q_pool[q_off[q]:q_off[q + 1]] and the lexicon (chars, order,
    class_first) of `lexicon_layout_host`, (exact int32 [Q], found int32 [Q], cand int32 [Q, K], dist int32 [Q, K]).  Two ids
    are equal iff they are the same number AND that number lies in [0, V): an id outside the range equals nothing, itself
    included.  lev is the Levenshtein distance with unit costs under that equality.  For a query of 1 .. 64 ids, over the
    entries e of `order` with lev(q, e) <= max_dist: exact[q] the smallest original index with lev == 0, or -1; found[q] the
    number with lev >= 1, whatever K is; cand[q] the original indices of the first K of these ordered by (lev, original index),
    dist[q] their distances, unused places -1 in both.  A query of no ids or of more than 64 gets -1, 0 and -1 everywhere.
    Duplicate entries are separate entries.  A plain DP, row by row of the query, over all entries of a length class at once
    -- only the classes max(1, m - max_dist) .. min(64, m + max_dist) can hold a neighbour."""
    q_pool = np.asarray(q_pool, dtype=np.int64).reshape(-1)
    q_off = np.asarray(q_off, dtype=np.int64).reshape(-1)
    chars = np.asarray(chars, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    class_first = np.asarray(class_first, dtype=np.int64).reshape(-1)
    V, max_dist, K = int(V), int(max_dist), int(K)
    if not (1 <= V <= LEXICON_V_MAX and 0 <= max_dist <= LEXICON_DIST_MAX and 1 <= K <= LEXICON_K_MAX):
        raise ValueError("lexicon_neighbours_host: V in 1 .. %d, max_dist in 0 .. %d, K in 1 .. %d"
                         % (LEXICON_V_MAX, LEXICON_DIST_MAX, LEXICON_K_MAX))
    n_class = np.diff(class_first)
    base = np.concatenate([[0], np.cumsum(np.arange(SPAN_LEN_MAX + 1) * n_class)])
    if (len(class_first) != SPAN_LEN_MAX + 2 or class_first[0] != 0 or class_first[1] != 0 or (n_class < 0).any()
            or class_first[-1] != len(order) or base[-1] != len(chars)):
        raise ValueError("lexicon_neighbours_host: class_first [66] ascending from 0, 0 to len(order), chars of sum L * n_L ids")
    if len(q_off) < 1 or q_off[0] < 0 or (np.diff(q_off) < 0).any() or q_off[-1] > len(q_pool):
        raise ValueError("lexicon_neighbours_host: q_off [Q + 1] ascending within the pool")
    Q = len(q_off) - 1
    exact = np.full(Q, -1, dtype=np.int32)
    found = np.zeros(Q, dtype=np.int32)
    cand = np.full((Q, K), -1, dtype=np.int32)
    dist = np.full((Q, K), -1, dtype=np.int32)
    known = (chars >= 0) & (chars < V)
    for q in range(Q):
        word = q_pool[q_off[q]:q_off[q + 1]]
        m = len(word)
        if not 1 <= m <= SPAN_LEN_MAX:
            continue
        hits, levs = [], []
        for L in range(max(1, m - max_dist), min(SPAN_LEN_MAX, m + max_dist) + 1):
            n = int(n_class[L])
            if n == 0:
                continue
            entry = chars[base[L]:base[L + 1]].reshape(L, n)             # [L, n]: id j of every entry of the class
            valid = known[base[L]:base[L + 1]].reshape(L, n)
            prev = np.repeat(np.arange(L + 1, dtype=np.int32)[:, None], n, axis=1)      # row 0: j edits
            for i in range(1, m + 1):
                differ = ~((entry == word[i - 1]) & valid)      # (a query id outside [0, V) is never among the valid ones)
                cur = np.empty_like(prev)
                cur[0] = i
                for j in range(1, L + 1):
                    cur[j] = np.minimum(np.minimum(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + differ[j - 1])
                prev = cur
            lev = prev[L]
            near = np.nonzero(lev <= max_dist)[0]
            hits.append(order[class_first[L] + near])
            levs.append(lev[near].astype(np.int64))
        if not hits:
            continue
        hits, levs = np.concatenate(hits), np.concatenate(levs)
        same = hits[levs == 0]
        if len(same):
            exact[q] = same.min()
        hits, levs = hits[levs > 0], levs[levs > 0]
        found[q] = len(hits)
        first = np.lexsort((hits, levs))[:K]
        cand[q, :len(first)] = hits[first]
        dist[q, :len(first)] = levs[first]
    return exact, found, cand, dist


LEXICON_MIN_PART_MAX = 32      # (kl_lexicon_splits: min_part at most)


def lexicon_splits_host(q_pool, q_off, chars, order, class_first, V, max_dist, min_part, K):
    """what kl_lexicon_splits computes: for the Q queries and the lexicon of `lexicon_neighbours_host`, under its id equality,
    (found int32 [Q], split, left, right, dist int32 [Q, K]).  The missing delimiter costs one edit, so the halves share
    d = max_dist - 1.  For a query q of m ids, 1 <= m <= 64, and every split point s with min_part <= s <= m - min_part:
    best(h) of a half h is the entry minimising (lev(h, e), original index) among the entries with lev(h, e) <= d -- entries
    at distance 0 count, duplicate entries are separate entries --, and s is valid iff best(q[:s]) and best(q[s:]) both exist
    and total = 1 + lev_left + lev_right <= max_dist.  found[q] is the number of valid split points, whatever K is;
    split, left, right, dist[q] hold s, the two original indices and total of the first K valid split points ordered by
    (total, max(left index, right index), s), unused places -1 in all four.  A query with no split point, of no ids or of
    more than 64 gets 0 and -1 everywhere.  A plain DP per half and length class, row by row of the half, over all entries of
    the class at once -- only the classes within d of the half's length can hold its entry."""
    q_pool = np.asarray(q_pool, dtype=np.int64).reshape(-1)
    q_off = np.asarray(q_off, dtype=np.int64).reshape(-1)
    chars = np.asarray(chars, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    class_first = np.asarray(class_first, dtype=np.int64).reshape(-1)
    V, max_dist, min_part, K = int(V), int(max_dist), int(min_part), int(K)
    if not (1 <= V <= LEXICON_V_MAX and 1 <= max_dist <= LEXICON_DIST_MAX and 1 <= min_part <= LEXICON_MIN_PART_MAX
            and 1 <= K <= LEXICON_K_MAX):
        raise ValueError("lexicon_splits_host: V in 1 .. %d, max_dist in 1 .. %d, min_part in 1 .. %d, K in 1 .. %d"
                         % (LEXICON_V_MAX, LEXICON_DIST_MAX, LEXICON_MIN_PART_MAX, LEXICON_K_MAX))
    n_class = np.diff(class_first)
    base = np.concatenate([[0], np.cumsum(np.arange(SPAN_LEN_MAX + 1) * n_class)])
    if (len(class_first) != SPAN_LEN_MAX + 2 or class_first[0] != 0 or class_first[1] != 0 or (n_class < 0).any()
            or class_first[-1] != len(order) or base[-1] != len(chars)):
        raise ValueError("lexicon_splits_host: class_first [66] ascending from 0, 0 to len(order), chars of sum L * n_L ids")
    if len(q_off) < 1 or q_off[0] < 0 or (np.diff(q_off) < 0).any() or q_off[-1] > len(q_pool):
        raise ValueError("lexicon_splits_host: q_off [Q + 1] ascending within the pool")
    d = max_dist - 1
    known = (chars >= 0) & (chars < V)
    seen = {}      # (halves recur within a call: a half is looked up once)

    def best(half):
        """(lev, original index) of the half's nearest entry within d, None: there is none"""
        if half.tobytes() in seen:
            return seen[half.tobytes()]
        n_half, least = len(half), None
        for L in range(max(1, n_half - d), min(SPAN_LEN_MAX, n_half + d) + 1):
            n = int(n_class[L])
            if n == 0:
                continue
            entry = chars[base[L]:base[L + 1]].reshape(L, n)
            valid = known[base[L]:base[L + 1]].reshape(L, n)
            along = np.arange(L + 1, dtype=np.int32)[:, None]
            prev = np.repeat(along, n, axis=1)                         # row 0: j edits
            for i in range(1, n_half + 1):
                differ = ~((entry == half[i - 1]) & valid)
                # cur[j] = min(prev[j] + 1, prev[j - 1] + differ, cur[j - 1] + 1), cur[0] = i: the third term is a running
                # minimum along j of the first two, each j behind costing one more
                cur = np.full_like(prev, i)
                cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + differ)
                prev = np.minimum.accumulate(cur - along, axis=0) + along
            lev = prev[L]
            near = np.nonzero(lev <= d)[0]
            if len(near):
                one = min(zip(lev[near].tolist(), order[class_first[L] + near].tolist()))
                least = one if least is None or one < least else least
        seen[half.tobytes()] = least
        return least

    Q = len(q_off) - 1
    found = np.zeros(Q, dtype=np.int32)
    out = np.full((4, Q, K), -1, dtype=np.int32)
    for q in range(Q):
        word = q_pool[q_off[q]:q_off[q + 1]]
        m = len(word)
        if not 1 <= m <= SPAN_LEN_MAX:
            continue
        valid = []
        for s in range(min_part, m - min_part + 1):
            a = best(word[:s])
            b = best(word[s:]) if a is not None else None
            if a is not None and b is not None and 1 + a[0] + b[0] <= max_dist:
                valid.append((1 + a[0] + b[0], max(a[1], b[1]), s, a[1], b[1]))
        found[q] = len(valid)
        for place, (total, _, s, a, b) in enumerate(sorted(valid)[:K]):
            out[:, q, place] = s, a, b, total
    return found, out[0], out[1], out[2], out[3]


LEXICON_PARTS_MAX, LEXICON_LINKS_MAX, LEXICON_LINK_LEN_MAX = 8, 8, 3      # (kl_lexicon_chains: parts, links, ids of a link)


def lexicon_links_host(links, V):
    """the links of `lexicon_chains_host` as kl_lexicon_chains takes them: int32 [n_links, 4] -- len, ids[3], unused ids 0 --
    from a sequence of id sequences (or from such an array).  ValueError for more than 8 links, a link of no ids or of more
    than 3, an id outside [0, V)."""
    if isinstance(links, np.ndarray) and links.ndim == 2 and links.shape[1] == 1 + LEXICON_LINK_LEN_MAX:
        rows = np.asarray(links, dtype=np.int64)
        if ((rows[:, 0] < 1) | (rows[:, 0] > LEXICON_LINK_LEN_MAX)).any():
            raise ValueError("lexicon_chains: a link has 1 .. %d ids" % LEXICON_LINK_LEN_MAX)
        links = [row[1:1 + row[0]].tolist() for row in rows]
    links = [[int(c) for c in one] for one in links]
    if len(links) > LEXICON_LINKS_MAX:
        raise ValueError("lexicon_chains: at most %d links (got %d)" % (LEXICON_LINKS_MAX, len(links)))
    out = np.zeros((len(links), 1 + LEXICON_LINK_LEN_MAX), dtype=np.int32)
    for l, one in enumerate(links):
        if not 1 <= len(one) <= LEXICON_LINK_LEN_MAX or any(not 0 <= c < V for c in one):
            raise ValueError("lexicon_chains: a link has 1 .. %d ids, each in [0, V)" % LEXICON_LINK_LEN_MAX)
        out[l, 0] = len(one)
        out[l, 1:1 + len(one)] = one
    return out


def lexicon_chains_host(q_pool, q_off, chars, order, class_first, V, links, max_parts, min_part):
    """what kl_lexicon_chains computes: for the Q queries and the lexicon of `lexicon_neighbours_host`, under its id equality,
    (found int32 [Q], worst int32 [Q, P], entry, start, link int32 [Q, P, P]) with P = max_parts.  links is a sequence of id
    sequences (1 .. 3 ids in [0, V) each, at most 8), or the int32 [n, 4] of `lexicon_links_host`.  For a query q of m ids,
    1 <= m <= 64: piece(a, b), b - a >= min_part, is the smallest original index of an entry identical to q[a:b] (duplicate
    entries are separate entries), or none.  A chain of p parts is a sequence of pieces from 0 to m, neighbours adjacent or
    with one of the links between them; its key is the largest piece index.  E[1][b] = piece(0, b); for p >= 2, E[p][b] is
    the least of max(E[p-1][b'], piece(a, b)), the candidates visited with a ascending and per a first b' = a, then the links
    in index order that are identical to q[a-len:a] with b' = a - len >= 1; the first candidate of least key is kept.  The
    chain of p parts is the walk back from E[p][m].  found[q] has bit p-1 set iff a chain of p parts exists, worst[q, p-1]
    is its key, entry[q, p-1, :p] the pieces' indices, start[q, p-1, :p] where they begin, link[q, p-1, :p-1] the link
    between piece k and k + 1 (-1: none); -1 in every unused place.  A query of no ids, of more than 64 or shorter than
    min_part gets 0 and -1 everywhere."""
    q_pool = np.asarray(q_pool, dtype=np.int64).reshape(-1)
    q_off = np.asarray(q_off, dtype=np.int64).reshape(-1)
    chars = np.asarray(chars, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    class_first = np.asarray(class_first, dtype=np.int64).reshape(-1)
    V, P, min_part = int(V), int(max_parts), int(min_part)
    if not (1 <= V <= LEXICON_V_MAX and 2 <= P <= LEXICON_PARTS_MAX and 1 <= min_part <= LEXICON_MIN_PART_MAX):
        raise ValueError("lexicon_chains_host: V in 1 .. %d, max_parts in 2 .. %d, min_part in 1 .. %d"
                         % (LEXICON_V_MAX, LEXICON_PARTS_MAX, LEXICON_MIN_PART_MAX))
    links = lexicon_links_host(links, V)
    links = [tuple(row[1:1 + row[0]].tolist()) for row in links]
    n_class = np.diff(class_first)
    base = np.concatenate([[0], np.cumsum(np.arange(SPAN_LEN_MAX + 1) * n_class)])
    if (len(class_first) != SPAN_LEN_MAX + 2 or class_first[0] != 0 or class_first[1] != 0 or (n_class < 0).any()
            or class_first[-1] != len(order) or base[-1] != len(chars)):
        raise ValueError("lexicon_chains_host: class_first [66] ascending from 0, 0 to len(order), chars of sum L * n_L ids")
    if len(q_off) < 1 or q_off[0] < 0 or (np.diff(q_off) < 0).any() or q_off[-1] > len(q_pool):
        raise ValueError("lexicon_chains_host: q_off [Q + 1] ascending within the pool")
    by_class = {}      # L -> {the entry's ids: its smallest original index}, made when a query first asks for the class

    def entries_of(L):
        if L not in by_class:
            n = int(n_class[L])
            rows = np.ascontiguousarray(chars[base[L]:base[L + 1]].reshape(L, n).T)      # [n, L]
            usable = ((rows >= 0) & (rows < V)).all(axis=1)
            index = order[class_first[L]:class_first[L + 1]]
            table = {}
            for e in np.nonzero(usable)[0].tolist():
                key = rows[e].tobytes()
                if key not in table or index[e] < table[key]:
                    table[key] = int(index[e])
            by_class[L] = table
        return by_class[L]

    Q = len(q_off) - 1
    found = np.zeros(Q, dtype=np.int32)
    worst = np.full((Q, P), -1, dtype=np.int32)
    entry = np.full((Q, P, P), -1, dtype=np.int32)
    start = np.full((Q, P, P), -1, dtype=np.int32)
    link = np.full((Q, P, P), -1, dtype=np.int32)
    for q in range(Q):
        word = np.ascontiguousarray(q_pool[q_off[q]:q_off[q + 1]])
        m = len(word)
        if not max(1, min_part) <= m <= SPAN_LEN_MAX:
            continue
        usable = (word >= 0) & (word < V)
        bad_before = np.concatenate([[0], np.cumsum(~usable)])
        piece = {}
        for a in range(m):
            for b in range(a + min_part, m + 1):
                if bad_before[b] == bad_before[a]:
                    index = entries_of(b - a).get(word[a:b].tobytes())
                    if index is not None:
                        piece[a, b] = index
        ids = word.tolist()
        ends = [[l for l, one in enumerate(links) if a - len(one) >= 1 and tuple(ids[a - len(one):a]) == one] for a in range(m + 1)]
        E = [None, dict((b, (piece[0, b], 0, -1)) for b in range(1, m + 1) if (0, b) in piece)]      # b -> (key, a, link)
        for p in range(2, P + 1):
            row = {}
            for b in range(1, m + 1):
                best = None
                for a in range(1, b - min_part + 1):
                    if (a, b) not in piece:
                        continue
                    for l, before in [(-1, a)] + [(l, a - len(links[l])) for l in ends[a]]:
                        if before in E[p - 1]:
                            key = max(E[p - 1][before][0], piece[a, b])
                            if best is None or key < best[0]:
                                best = (key, a, l)
                if best is not None:
                    row[b] = best
            E.append(row)
        for p in range(1, P + 1):
            if m not in E[p]:
                continue
            found[q] |= 1 << (p - 1)
            worst[q, p - 1] = E[p][m][0]
            b = m
            for k in range(p, 0, -1):
                _, a, l = E[k][b]
                entry[q, p - 1, k - 1] = piece[a, b]
                start[q, p - 1, k - 1] = a
                if k >= 2:
                    link[q, p - 1, k - 2] = l
                b = a - len(links[l]) if l >= 0 else a
    return found, worst, entry, start, link


CHANNEL_RULES_MAX, CHANNEL_COST_MAX = 1024, 4095      # (KL_CHANNEL_* of the C ABI)
CHANNEL_SCALE = 16                                    # the Python layer counts in sixteenths of a bit


def channel_rules_kept(rules, rule_cost, V):
    """the rules kl_lexicon_channel does not ignore, as [(src tuple, tgt tuple, cost)] in the order given: src_len in 1 .. 4,
    tgt_len in 0 .. 4, every used id in [0, V), the cost in 0 .. CHANNEL_COST_MAX.  rules is int32 [R, 10] in the record
    layout of `confusion_counts_host` (src_len, tgt_len, src[4], tgt[4]), rule_cost int32 [R]."""
    rules = np.asarray(rules, dtype=np.int64).reshape(-1, 2 + 2 * CONFUSION_CHARS_MAX)
    rule_cost = np.asarray(rule_cost, dtype=np.int64).reshape(-1)
    if len(rules) != len(rule_cost):
        raise ValueError("channel_rules_kept: one cost per rule")
    kept = []
    for rec, cost in zip(rules.tolist(), rule_cost.tolist()):
        s, t = rec[0], rec[1]
        if not (1 <= s <= CONFUSION_CHARS_MAX and 0 <= t <= CONFUSION_CHARS_MAX and 0 <= cost <= CHANNEL_COST_MAX):
            continue
        src, tgt = tuple(rec[2:2 + s]), tuple(rec[2 + CONFUSION_CHARS_MAX:2 + CONFUSION_CHARS_MAX + t])
        if all(0 <= c < V for c in src + tgt):
            kept.append((src, tgt, cost))
    return kept


def lexicon_channel_host(q_pool, q_off, chars, order, class_first, V, rules, rule_cost, unit, max_cost, K):
    """what kl_lexicon_channel computes: `lexicon_neighbours_host` under a weighted distance.  The lexicon, the queries, the
    id equality (an id outside [0, V) equals nothing, itself included) and the outputs' conventions are the same; rules and
    rule_cost are those of `channel_rules_kept` (None or empty: no rules), the SOURCE of a rule is what stands in the query,
    the TARGET what stands in the entry.  With m, n the lengths of query q and entry e: W[0][0] = 0 and otherwise W[i][j] is
    the least of W[i-1][j-1] + (q[i-1] == e[j-1] ? 0 : unit), W[i-1][j] + unit, W[i][j-1] + unit and W[i-s][j-t] + cost for
    every kept rule (src, tgt, cost) with s = len(src) <= i, t = len(tgt) <= j, q[i-s:i] == src, e[j-t:j] == tgt;
    w(q, e) = W[m][n].  Returns (exact int32 [Q], found int32 [Q], cand int32 [Q, K], cost int32 [Q, K]): exact[q] the smallest
    original index of an entry IDENTICAL to the query, or -1; found[q] the number of entries that are not identical with
    w <= max_cost; cand[q] the first K of these ordered by (w, original index), cost[q] their w, unused places -1.  A query of
    no ids or of more than 64 gets -1, 0 and -1 everywhere.

    A plain DP over all entries of a length class at once.  Only the classes m + d with |d| * price <= max_cost can hold
    such an entry, price being the least cost per id of lengthening (unit, or cost / (t - s) over the rules with t > s) for
    d > 0 and of shortening (s > t) for d < 0 -- compared as exact fractions."""
    q_pool = np.asarray(q_pool, dtype=np.int64).reshape(-1)
    q_off = np.asarray(q_off, dtype=np.int64).reshape(-1)
    chars = np.asarray(chars, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    class_first = np.asarray(class_first, dtype=np.int64).reshape(-1)
    V, unit, max_cost, K = int(V), int(unit), int(max_cost), int(K)
    if not (1 <= V <= LEXICON_V_MAX and 1 <= unit <= CHANNEL_COST_MAX and 0 <= max_cost <= CHANNEL_COST_MAX
            and 1 <= K <= LEXICON_K_MAX):
        raise ValueError("lexicon_channel_host: V in 1 .. %d, unit in 1 .. %d, max_cost in 0 .. %d, K in 1 .. %d"
                         % (LEXICON_V_MAX, CHANNEL_COST_MAX, CHANNEL_COST_MAX, LEXICON_K_MAX))
    if rules is None or len(rules) == 0:
        rules, rule_cost = np.zeros((0, 2 + 2 * CONFUSION_CHARS_MAX), dtype=np.int32), np.zeros(0, dtype=np.int32)
    if len(rule_cost) > CHANNEL_RULES_MAX:
        raise ValueError("lexicon_channel_host: at most %d rules" % CHANNEL_RULES_MAX)
    kept = channel_rules_kept(rules, rule_cost, V)
    n_class = np.diff(class_first)
    base = np.concatenate([[0], np.cumsum(np.arange(SPAN_LEN_MAX + 1) * n_class)])
    if (len(class_first) != SPAN_LEN_MAX + 2 or class_first[0] != 0 or class_first[1] != 0 or (n_class < 0).any()
            or class_first[-1] != len(order) or base[-1] != len(chars)):
        raise ValueError("lexicon_channel_host: class_first [66] ascending from 0, 0 to len(order), chars of sum L * n_L ids")
    if len(q_off) < 1 or q_off[0] < 0 or (np.diff(q_off) < 0).any() or q_off[-1] > len(q_pool):
        raise ValueError("lexicon_channel_host: q_off [Q + 1] ascending within the pool")
    # how far a length may lie from the query's: d * (num / den) <= max_cost
    reach = []
    for longer in (True, False):
        num, den = unit, 1
        for src, tgt, cost in kept:
            by = len(tgt) - len(src) if longer else len(src) - len(tgt)
            if by > 0 and cost * den < num * by:
                num, den = cost, by
        reach.append(SPAN_LEN_MAX if num == 0 else min(SPAN_LEN_MAX, max_cost * den // num))
    Q = len(q_off) - 1
    exact = np.full(Q, -1, dtype=np.int32)
    found = np.zeros(Q, dtype=np.int32)
    cand = np.full((Q, K), -1, dtype=np.int32)
    cost_out = np.full((Q, K), -1, dtype=np.int32)
    known = (chars >= 0) & (chars < V)
    beyond = max_cost + 1      # (every larger value is as good as this one)
    tables = {}                # (class, rules of one shape) -> [L + 1, n]: the least cost of those whose target ends at column j
    for q in range(Q):
        word = q_pool[q_off[q]:q_off[q + 1]]
        m = len(word)
        if not 1 <= m <= SPAN_LEN_MAX:
            continue
        word = np.where((word >= 0) & (word < V), word, -1)
        # the rules whose source stands in front of row i, by shape (s, t)
        active = [{} for _ in range(m + 1)]
        for r, (src, tgt, cost) in enumerate(kept):
            s = len(src)
            for i in range(s, m + 1):
                if tuple(word[i - s:i].tolist()) == src:
                    active[i].setdefault((s, len(tgt)), []).append(r)
        active = [[(s, t, tuple(rows)) for (s, t), rows in sorted(one.items())] for one in active]
        hits, costs, sames = [], [], []
        for L in range(max(1, m - reach[1]), min(SPAN_LEN_MAX, m + reach[0]) + 1):
            n = int(n_class[L])
            if n == 0:
                continue
            entry = np.where(known[base[L]:base[L + 1]], chars[base[L]:base[L + 1]], -2).reshape(L, n)
            W = np.full((m + 1, L + 1, n), beyond, dtype=np.int64)
            W[0, 0] = 0
            for j in range(L + 1):
                for i in range(m + 1):
                    v = W[i, j]
                    if i > 0:
                        v = np.minimum(v, W[i - 1, j] + unit)
                    if j > 0:
                        v = np.minimum(v, W[i, j - 1] + unit)
                    if i > 0 and j > 0:
                        v = np.minimum(v, W[i - 1, j - 1] + np.where(entry[j - 1] == word[i - 1], 0, unit))
                    for s, t, rows in active[i]:
                        if j < t:
                            continue
                        if (L, rows) not in tables:
                            least = np.full((L + 1, n), beyond, dtype=np.int64)
                            for r in rows:
                                tgt, cost = kept[r][1], kept[r][2]
                                if t <= L:
                                    ends = np.ones((L - t + 1, n), dtype=bool)
                                    for k in range(t):
                                        ends &= entry[k:L - t + 1 + k] == tgt[k]
                                    least[t:] = np.where(ends, np.minimum(least[t:], cost), least[t:])
                            tables[L, rows] = least
                        v = np.minimum(v, W[i - s, j - t] + tables[L, rows][j])
                    W[i, j] = np.minimum(v, beyond)
            w = W[m, L]
            near = np.nonzero(w <= max_cost)[0]
            hits.append(order[class_first[L] + near])
            costs.append(w[near])
            sames.append((entry[:, near] == word[:, None]).all(axis=0) if L == m else np.zeros(len(near), dtype=bool))
        if len(tables) > 1024:      # (the tables of one call, bounded)
            tables.clear()
        if not hits:
            continue
        hits, costs, sames = np.concatenate(hits), np.concatenate(costs), np.concatenate(sames)
        if sames.any():
            exact[q] = hits[sames].min()
        hits, costs = hits[~sames], costs[~sames]
        found[q] = len(hits)
        first = np.lexsort((hits, costs))[:K]
        cand[q, :len(first)] = hits[first]
        cost_out[q, :len(first)] = costs[first]
    return exact, found, cand, cost_out


ALIGN_DIST_MAX, ALIGN_LEN_MAX = 255, 4096      # (KL_ALIGN_* of the C ABI)
_BEYOND = 1 << 20                              # a value outside the band


def align_pairs_host(a_pool, a_off, b_pool, b_off, max_len, max_dist, join):
    """what kl_align_pairs computes: for the P pairs a = a_pool[a_off[p]:a_off[p + 1]], b = b_pool[b_off[p]:b_off[p + 1]] of
    int32 symbols (equal iff the same number), (dist int32 [P], n_spans int32 [P], spans int32 [P, max_dist, 4]).

    With n, m the lengths: D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1,
    D[i][j-1] + 1), d = D[n][m].  dist[p] is d if d <= max_dist, -1 if d > max_dist, -2 if n > max_len or m > max_len or the
    offsets are descending or reach outside their pool; n_spans is 0 for -1 and -2.  The walk back from (n, m) takes the first
    that applies at (i, j): a match (i, j > 0, a[i-1] == b[j-1], D[i-1][j-1] == D[i][j]), a substitution (i, j > 0,
    D[i-1][j-1] + 1 == D[i][j]), a deletion of a[i-1] (i > 0, D[i-1][j] + 1 == D[i][j]), else an insertion of b[j-1].  Read
    forwards, a maximal run of non-matches is a difference; two with at most `join` matches between them become one, the
    matches included.  spans[p, s] = (a_start, a_end, b_start, b_end), ascending, -1 in every place from n_spans[p] on.

    A plain DP, row by row, over the band |i - j| <= max_dist (row i holds j = i - max_dist .. i + max_dist at index
    j - i + max_dist, `_BEYOND` outside the matrix): a cell worth at most max_dist is exact under the band and every other only
    larger, so nothing above changes for d <= max_dist, and d > max_dist is seen as such."""
    a_pool = np.asarray(a_pool, dtype=np.int32).reshape(-1)
    b_pool = np.asarray(b_pool, dtype=np.int32).reshape(-1)
    a_off = np.asarray(a_off, dtype=np.int64).reshape(-1)
    b_off = np.asarray(b_off, dtype=np.int64).reshape(-1)
    max_len, K, join = int(max_len), int(max_dist), int(join)
    if not (0 <= max_len <= ALIGN_LEN_MAX and 1 <= K <= ALIGN_DIST_MAX and join >= 0):
        raise ValueError("align_pairs_host: max_len in 0 .. %d, max_dist in 1 .. %d, join >= 0" % (ALIGN_LEN_MAX, ALIGN_DIST_MAX))
    if len(a_off) < 2 or len(a_off) != len(b_off):
        raise ValueError("align_pairs_host: a_off and b_off [P + 1], P >= 1")
    P = len(a_off) - 1
    dist = np.zeros(P, dtype=np.int32)
    n_spans = np.zeros(P, dtype=np.int32)
    spans = np.full((P, K, 4), -1, dtype=np.int32)
    L = 2 * K + 1
    lane = np.arange(L)
    for p in range(P):
        a0, a1, b0, b1 = int(a_off[p]), int(a_off[p + 1]), int(b_off[p]), int(b_off[p + 1])
        n, m = a1 - a0, b1 - b0
        if a0 < 0 or n < 0 or a1 > len(a_pool) or b0 < 0 or m < 0 or b1 > len(b_pool) or n > max_len or m > max_len:
            dist[p] = -2
            continue
        if abs(n - m) > K:
            dist[p] = -1
            continue
        a, b = a_pool[a0:a1], b_pool[b0:b1]
        padded = np.concatenate([np.zeros(K + 1, dtype=np.int32), b, np.zeros(2 * K, dtype=np.int32)])      # b[j - 1] at [j + K]
        D = np.full((n + 1, L + 1), _BEYOND, dtype=np.int64)      # (one column more: D[i - 1][j] of the last diagonal)
        j = lane - K
        D[0, :L][(j >= 0) & (j <= m)] = j[(j >= 0) & (j <= m)]
        for i in range(1, n + 1):
            j = i + lane - K
            inside = (j >= 0) & (j <= m)
            differ = (padded[i:i + L] != a[i - 1]).astype(np.int64)
            cell = np.minimum(D[i - 1, :L] + differ, D[i - 1, 1:] + 1)      # from (i - 1, j - 1) and from (i - 1, j)
            cell[j == 0] = i
            cell[~inside] = _BEYOND
            cell = np.minimum.accumulate(cell - lane) + lane                 # from (i, j - 1), all the way along the row
            cell[~inside] = _BEYOND
            D[i, :L] = np.minimum(cell, _BEYOND)
        d = int(D[n, m - n + K])
        if d > K:
            dist[p] = -1
            continue
        dist[p] = d
        at = lambda i, j: int(D[i, j - i + K]) if i >= 0 and 0 <= j <= m and abs(i - j) <= K else _BEYOND
        ops = []                                  # backwards: (is a match, i, j) with (i, j) the cell the operation ends in
        i, j = n, m
        while i > 0 or j > 0:
            here = at(i, j)
            if i > 0 and j > 0 and a[i - 1] == b[j - 1] and at(i - 1, j - 1) == here:
                ops.append((True, i, j))
                i, j = i - 1, j - 1
            elif i > 0 and j > 0 and at(i - 1, j - 1) + 1 == here:
                ops.append((False, i, j))
                i, j = i - 1, j - 1
            elif i > 0 and at(i - 1, j) + 1 == here:
                ops.append((False, i, j))
                i = i - 1
            else:
                ops.append((False, i, j))
                j = j - 1
        found = []                                # [a_start, a_end, b_start, b_end], ascending
        i = j = matches = 0
        for match, i_next, j_next in reversed(ops):
            if match:
                matches += 1
            else:
                if found and matches <= join:
                    found[-1][1], found[-1][3] = i_next, j_next
                else:
                    found.append([i, i_next, j, j_next])
                matches = 0
            i, j = i_next, j_next
        n_spans[p] = len(found)
        if found:
            spans[p, :len(found)] = found
    return dist, n_spans, spans


CONFUSION_CHARS_MAX = 4      # (KL_CONFUSION_CHARS_MAX of the C ABI)


def confusion_counts_host(a_pool, a_off, b_pool, b_off, dist, n_spans, spans, max_chars, room):
    """what kl_confusion_counts computes: from the pairs of `align_pairs_host` (a the OCR, b the truth) and what it returned --
    dist [P], n_spans [P], spans [P, max_dist, 4] --, (rules int32 [room, 10], count int64 [room], occ int64 [room], stats
    int64 [4]).

    A pair is accepted if dist[p] >= 0 and its offsets ascend and lie inside their pools; nothing of another pair is read.  The
    record of a span (a0, a1, b0, b1) -- the slots s < n_spans[p] -- of an accepted pair with the texts a, b of n, m symbols:
    fields outside the texts (not 0 <= a0 <= a1 <= n and 0 <= b0 <= b1 <= m) give none and count as `long`; for a1 > a0 source
    a[a0:a1] and target b[b0:b1]; for a1 == a0 > 0 (the OCR lost characters, a rule needs a source: anchored in front) source
    a[a0-1:a0] and target b[b0-1:b1], `long` for b0 == 0; for a1 == a0 == 0 and n > 0 (anchored behind) source a[0:1] and target
    b[0:b1+1], `long` for b1 == m; for a1 == a0 == 0 and n == 0 none, counted as `empty`; more than max_chars symbols on either
    side after anchoring give none and count as `long`.

    The table holds the distinct records (src_len, tgt_len, src[4], tgt[4]; unused places 0) in order of first occurrence, by
    pair and then by span, with count -- the spans that gave the record -- and occ -- the positions i of the a-texts of all
    accepted pairs with a[i:i+src_len] == source, overlapping ones included, none across a text's end.  The outputs hold the
    first min(R, room) records, behind them -1 in rules and 0 in count and occ; stats = (R, spans that gave a record, long,
    empty).  Plain Python over the spans and a dictionary: the reference, not fast."""
    a_pool = np.asarray(a_pool, dtype=np.int32).reshape(-1)
    b_pool = np.asarray(b_pool, dtype=np.int32).reshape(-1)
    a_off = np.asarray(a_off, dtype=np.int64).reshape(-1)
    b_off = np.asarray(b_off, dtype=np.int64).reshape(-1)
    dist = np.asarray(dist, dtype=np.int32).reshape(-1)
    n_spans = np.asarray(n_spans, dtype=np.int32).reshape(-1)
    spans = np.asarray(spans, dtype=np.int32)
    max_chars, room = int(max_chars), int(room)
    P = len(a_off) - 1
    if P < 1 or len(b_off) != P + 1 or len(dist) != P or len(n_spans) != P or spans.ndim != 3 or spans.shape[0] != P or spans.shape[2] != 4:
        raise ValueError("confusion_counts_host: a_off and b_off [P + 1], dist and n_spans [P], spans [P, max_dist, 4], P >= 1")
    if not (1 <= spans.shape[1] <= ALIGN_DIST_MAX and 1 <= max_chars <= CONFUSION_CHARS_MAX and room >= 1):
        raise ValueError("confusion_counts_host: max_dist in 1 .. %d, max_chars in 1 .. %d, room >= 1" % (ALIGN_DIST_MAX, CONFUSION_CHARS_MAX))
    table = {}            # record -> its row: insertion order is the order of first occurrence
    counts = []
    counted = too_long = empty = 0
    texts = []            # the a-texts of the accepted pairs
    for p in range(P):
        a0, a1, b0, b1 = int(a_off[p]), int(a_off[p + 1]), int(b_off[p]), int(b_off[p + 1])
        if dist[p] < 0 or a0 < 0 or a1 < a0 or a1 > len(a_pool) or b0 < 0 or b1 < b0 or b1 > len(b_pool):
            continue
        a, b = a_pool[a0:a1].tolist(), b_pool[b0:b1].tolist()
        n, m = len(a), len(b)
        texts.append(a)
        for a0, a1, b0, b1 in spans[p, :max(int(n_spans[p]), 0)].tolist():
            if not (0 <= a0 <= a1 <= n and 0 <= b0 <= b1 <= m):
                too_long += 1
                continue
            if a1 > a0:
                source, target = a[a0:a1], b[b0:b1]
            elif a0 > 0:
                if b0 == 0:
                    too_long += 1
                    continue
                source, target = a[a0 - 1:a0], b[b0 - 1:b1]
            elif n > 0:
                if b1 == m:
                    too_long += 1
                    continue
                source, target = a[0:1], b[0:b1 + 1]
            else:
                empty += 1
                continue
            if len(source) > max_chars or len(target) > max_chars:
                too_long += 1
                continue
            counted += 1
            pad = lambda word: word + [0] * (CONFUSION_CHARS_MAX - len(word))
            record = tuple([len(source), len(target)] + pad(source) + pad(target))
            if record not in table:
                table[record] = len(counts)
                counts.append(0)
            counts[table[record]] += 1
    stands = {}           # (length, symbols) -> occurrences, for the sources of the table only
    for record in table:
        stands[record[0], record[2:2 + record[0]]] = 0
    for a in texts:
        for i in range(len(a)):
            for size in range(1, min(max_chars, len(a) - i) + 1):
                key = (size, tuple(a[i:i + size]))
                if key in stands:
                    stands[key] += 1
    R = len(counts)
    rules = np.full((room, 2 + 2 * CONFUSION_CHARS_MAX), -1, dtype=np.int32)
    count = np.zeros(room, dtype=np.int64)
    occ = np.zeros(room, dtype=np.int64)
    for record, row in table.items():
        if row < room:
            rules[row] = record
            count[row] = counts[row]
            occ[row] = stands[record[0], record[2:2 + record[0]]]
    return rules, count, occ, np.array([R, counted, too_long, empty], dtype=np.int64)


WITNESS_MAX = 64      # witnesses of a text at most (KL_WITNESS_MAX of the C ABI)


def witness_clusters_host(b_pool, b_off, dist, n_spans, spans, pair_first, text_off, join):
    """what kl_witness_clusters computes: the differing spans of ALL witnesses of a text clustered, every witness read over a
    whole cluster, equal readings made one and counted.  b_pool [n_b] int32 and b_off [P + 1] are the witnesses as
    `align_pairs_host` read them (side b), dist [P], n_spans [P], spans [P, max_dist, 4] what it returned; pair_first
    [n_texts + 1] (ascending from 0 to P) gives text i the pairs pair_first[i] .. pair_first[i+1]-1, its witnesses w = 0, 1, ..
    in order, all with that text as side a; text_off [n_texts + 1] are the texts' offsets in `span_windows_host`'s corpus,
    n_i = text_off[i+1] - text_off[i].  With R = P * max_dist returns (span_text int32 [R], span_start int64 [R], span_len
    int32 [R], span_first int64 [R + 1], cand_src int64 [R], cand_off int64 [R + 1], votes int32 [2 R], stats int64 [8]).

    A text whose pair range does not lie in [0, P] in ascending order, or holds more than WITNESS_MAX pairs, is counted in
    stats[7] and nothing of it is read.  A pair q of any other text is ACCEPTED if dist[q] >= 0, b_off[q] <= b_off[q+1] lie in
    [0, n_b] (m_q their difference), 0 <= n_spans[q] <= max_dist, and every slot s < n_spans[q] has 0 <= a0 <= a1 <= n_i,
    0 <= b0 <= b1 <= m_q, a0 >= the previous slot's a1 and b0 >= its b1; every other pair counts as `different` and nothing
    more of it is read.

    Clusters of text i: the spans (a0, a1) of its accepted pairs in order of (a0, a1, witness, slot), swept with a running end
    E: a span opens a cluster iff a0 > E + join, else it joins the current one and E = max(E, a1); the cluster is [u0, u1) =
    [least a0, greatest a1).  The spans of witness w in a cluster are a run f .. l of its slots -- none: it agrees with the text
    as written --, and its reading of text[u0:u1] is b[bs:be) with bs = b0_f - (a0_f - u0), be = b1_l + (u1 - a1_l).  The
    candidates of a cluster are the distinct readings, compared as code points, in order of the first witness that gives one;
    the votes of a candidate are the accepted witnesses that read it, those of the text as written 1 plus the accepted
    witnesses without a span in the cluster.  A cluster with u0 == 0 is dropped and counted as `first`; otherwise one with
    u1 - u0 > SPAN_LEN_MAX, a reading longer than that or a reading range outside [0, m_q] as `long`.

    The S kept clusters, ordered by text and u0, are `span_windows_host`'s spans: span_text, span_start = text_off[i] + u0,
    span_len, span_first [S + 1]; candidate c is b_pool[cand_src[c] : cand_src[c] + cand_off[c+1] - cand_off[c]] (cand_src
    the first witness' position in the pool, cand_off [C + 1] the offsets `witness_pool_host` fills); votes in ROW numbering --
    row span_first[s] + s the text as written, then the span's candidates.  Behind the used places -1, in votes and the two
    offset arrays 0.  stats = (S, C, n_pool = cand_off[C], the longest kept span or reading, different, first, long, texts
    with a bad pair range).  Plain Python over the spans: the reference, not fast."""
    b_pool = np.asarray(b_pool, dtype=np.int32).reshape(-1)
    b_off = np.asarray(b_off, dtype=np.int64).reshape(-1)
    dist = np.asarray(dist, dtype=np.int32).reshape(-1)
    n_spans = np.asarray(n_spans, dtype=np.int32).reshape(-1)
    spans = np.asarray(spans, dtype=np.int32)
    pair_first = np.asarray(pair_first, dtype=np.int64).reshape(-1)
    text_off = np.asarray(text_off, dtype=np.int64).reshape(-1)
    join = int(join)
    P, n_texts = len(b_off) - 1, len(pair_first) - 1
    if P < 1 or len(dist) != P or len(n_spans) != P or spans.ndim != 3 or spans.shape[0] != P or spans.shape[2] != 4:
        raise ValueError("witness_clusters_host: b_off [P + 1], dist and n_spans [P], spans [P, max_dist, 4], P >= 1")
    if n_texts < 1 or len(text_off) != n_texts + 1 or not 1 <= spans.shape[1] <= ALIGN_DIST_MAX or join < 0:
        raise ValueError("witness_clusters_host: pair_first and text_off [n_texts + 1], n_texts >= 1, max_dist in 1 .. %d, join >= 0"
                         % ALIGN_DIST_MAX)
    K, n_b = spans.shape[1], len(b_pool)
    R = P * K
    span_text, span_len = np.full(R, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32)
    span_start, cand_src = np.full(R, -1, dtype=np.int64), np.full(R, -1, dtype=np.int64)
    span_first, cand_off = np.zeros(R + 1, dtype=np.int64), np.zeros(R + 1, dtype=np.int64)
    votes = np.zeros(2 * R, dtype=np.int32)
    S = C = n_pool = longest = different = first = too_long = bad = 0
    for i in range(n_texts):
        q0, q1 = int(pair_first[i]), int(pair_first[i + 1])
        if q0 < 0 or q1 < q0 or q1 > P or q1 - q0 > WITNESS_MAX:
            bad += 1
            continue
        n_i = int(text_off[i + 1]) - int(text_off[i])
        accepted, items = {}, []      # witness -> (where its text begins in the pool, m_q, its slots)
        for w, q in enumerate(range(q0, q1)):
            lo, hi = int(b_off[q]), int(b_off[q + 1])
            m = hi - lo
            slots = spans[q, :max(int(n_spans[q]), 0)].tolist() if 0 <= n_spans[q] <= K else None
            ok = dist[q] >= 0 and 0 <= lo <= hi <= n_b and slots is not None
            end_a = end_b = 0
            for a0, a1, b0, b1 in slots or []:
                ok = ok and end_a <= a0 <= a1 <= n_i and end_b <= b0 <= b1 <= m
                end_a, end_b = a1, b1
            if not ok:
                different += 1
                continue
            accepted[w] = (lo, m, slots)
            items += [(a0, a1, w, s) for s, (a0, a1, _, _) in enumerate(slots)]
        clusters = []      # [u0, u1, {witness: [f, l]}]
        for a0, a1, w, s in sorted(items):
            if not clusters or a0 > clusters[-1][1] + join:
                clusters.append([a0, a1, {}])
            one = clusters[-1]
            one[1] = max(one[1], a1)
            one[2].setdefault(w, [s, s])[1] = s
        for u0, u1, runs in clusters:
            if u0 == 0:
                first += 1
                continue
            readings = []      # (position in the pool, length, witness) of every witness with a run
            fits = u1 - u0 <= SPAN_LEN_MAX
            for w in sorted(runs):
                lo, m, slots = accepted[w]
                f, l = runs[w]
                bs, be = slots[f][2] - (slots[f][0] - u0), slots[l][3] + (u1 - slots[l][1])
                fits = fits and 0 <= bs and be <= m and be - bs <= SPAN_LEN_MAX
                readings.append((lo + bs, be - bs))
            if not fits:
                too_long += 1
                continue
            distinct = {}      # code points -> [position of the first, length, votes]: insertion order is the order of first witnesses
            for at, size in readings:
                distinct.setdefault(tuple(b_pool[at:at + size].tolist()), [at, size, 0])[2] += 1
            span_text[S], span_start[S], span_len[S], span_first[S] = i, int(text_off[i]) + u0, u1 - u0, C
            votes[C + S] = 1 + len(accepted) - len(runs)
            longest = max(longest, u1 - u0)
            for at, size, count in distinct.values():
                cand_src[C], cand_off[C] = at, n_pool
                votes[C + S + 1] = count
                n_pool += size
                longest = max(longest, size)
                C += 1
            S += 1
    span_first[S], cand_off[C] = C, n_pool
    return (span_text, span_start, span_len, span_first, cand_src, cand_off, votes,
            np.array([S, C, n_pool, longest, different, first, too_long, bad], dtype=np.int64))


def witness_pool_host(b_ids, cand_src, cand_off, C, n_pool):
    """what kl_witness_pool computes: pool int32 [n_pool] with pool[cand_off[c] + k] = b_ids[cand_src[c] + k] for the candidates
    c < C of `witness_clusters_host` (cand_off [C + 1] ascending from 0 to n_pool): the readings as ids of the rater's mapping,
    b_ids [n_b] parallel to the code points the readings were compared by.  A position outside [0, n_b) reads as 0."""
    b_ids = np.asarray(b_ids, dtype=np.int32).reshape(-1)
    cand_src = np.asarray(cand_src, dtype=np.int64).reshape(-1)
    cand_off = np.asarray(cand_off, dtype=np.int64).reshape(-1)
    C, n_pool = int(C), int(n_pool)
    if C < 1 or n_pool < 0 or len(cand_src) < C or len(cand_off) < C + 1:
        raise ValueError("witness_pool_host: C >= 1, n_pool >= 0, cand_src [C], cand_off [C + 1]")
    g = np.arange(n_pool, dtype=np.int64)
    c = np.clip(np.searchsorted(cand_off[:C + 1], g, side="right") - 1, 0, C - 1)      # the last c with cand_off[c] <= g
    at = cand_src[c] + g - cand_off[c]
    inside = (at >= 0) & (at < len(b_ids))
    return np.where(inside, b_ids[np.where(inside, at, 0)] if len(b_ids) else 0, 0).astype(np.int32)
