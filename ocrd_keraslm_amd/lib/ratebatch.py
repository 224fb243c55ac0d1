"""Scheduler of `Rater.rate_batch`: many independent texts as lockstep rows of stateful windows.

`Rater.rate` (rating.py:493-529) feeds ONE text as `1 x length` windows.  Texts that do not depend on each other
can share a window call instead: each of B rows carries one text at a time, the windows of a text are exactly those
of `windows.stateful_windows(text, context, length, c_i)` (`train=False`), in order and in one row, and a row whose
text is finished takes the next text at the next call with that row's state zeroed.  A row with nothing left carries
`idx 0 / tgt -1` (no target, no bits).

Texts are dealt longest first to the row that is free first (list scheduling), so the number of window calls is at
most ceil(sum N_i / B) + max N_i for texts of N_i windows (Graham's bound; it holds for any order of the list).

numpy only: the plan is built and tested without an engine.
"""
from __future__ import annotations

import numpy as np

from . import windows


class Plan(object):
    """What `plan` returns.

    B, T        rows and window length of every call
    n_calls     number of window calls
    row, first, count   per text (input order): its row, its first call and its number of windows (0: none, row -1)
    sizes       per text: its number of characters
    """

    def __init__(self, B, T, n_calls, row, first, count, sizes, X, Y, Z, slots):
        self.B, self.T, self.n_calls = B, T, n_calls
        self.row, self.first, self.count, self.sizes = row, first, count, sizes
        self._X, self._Y, self._Z, self._slots = X, Y, Z, slots
        starts = [[] for _ in range(n_calls)]
        ends = [[] for _ in range(n_calls)]
        for i in np.nonzero(count > 0)[0]:
            starts[first[i]].append(int(i))
            ends[first[i] + count[i] - 1].append(int(i))
        self._starts, self._ends = starts, ends

    def call(self, s):
        """(idx [B,T], ctx [B,T,C], tgt [B,T]) int32 of call s"""
        w = self._slots[s]
        return self._X[w], self._Z[w], self._Y[w]

    def starting(self, s):
        """texts whose first window is in call s: their rows start from a zero state"""
        return self._starts[s]

    def ending(self, s):
        """texts whose last window is in call s"""
        return self._ends[s]

    def reset_rows(self, s):
        return [int(self.row[i]) for i in self._starts[s]]

    def text_probs(self, i, picked):
        """the probabilities of text i as `Rater.rate` lists them (1.0 for the first character) from the
        target probabilities of all calls, picked [n_calls][B][T]"""
        size = int(self.sizes[i])
        out = np.ones(min(size, 1) if self.count[i] == 0 else size, dtype=np.float32)
        if self.count[i]:
            a = int(self.first[i])
            out[1:] = picked[a:a + int(self.count[i]), int(self.row[i])].reshape(-1)[:size - 1]
        return out


def plan(ids, contexts, length, streams):
    """ids: one int32 id vector per text (`windows.encode`); contexts: one (clamped) context list per text;
    length: window length T; streams: upper limit of rows.  Returns a Plan, or None if no text has a window."""
    n = len(ids)
    T = int(length)
    sizes = np.array([len(a) for a in ids], dtype=np.int64)
    count = np.array([windows.count_windows(int(s), T) for s in sizes], dtype=np.int64)
    n_ctx = len(contexts[0]) if n else 0
    total = int(count.sum())
    if total == 0:
        return None
    B = int(min(max(1, int(streams)), int((count > 0).sum())))
    # every window of every text, padded as stateful_windows pads the last one (x 0, ctx 0, y -1), plus one idle window
    X = np.zeros((total + 1) * T, dtype=np.int32)
    Y = np.full((total + 1) * T, -1, dtype=np.int32)
    C = np.zeros((total + 1, n_ctx), dtype=np.int32)
    offset = np.concatenate([[0], np.cumsum(count)])[:-1]
    for i in range(n):
        if count[i]:
            a, m = int(offset[i]) * T, int(sizes[i]) - 1
            X[a:a + m] = ids[i][:-1]
            Y[a:a + m] = ids[i][1:]
            C[offset[i]:offset[i] + count[i]] = np.asarray(contexts[i], dtype=np.int32)
    X, Y = X.reshape(total + 1, T), Y.reshape(total + 1, T)
    Z = (Y >= 0)[:, :, None].astype(np.int32) * C[:, None, :]
    # list scheduling, longest first: the next text goes to the row that is free first
    order = [int(i) for i in np.argsort(-count, kind="stable") if count[i] > 0]
    free = np.zeros(B, dtype=np.int64)
    row = np.full(n, -1, dtype=np.int64)
    first = np.zeros(n, dtype=np.int64)
    for i in order:
        r = int(np.argmin(free))
        row[i], first[i] = r, free[r]
        free[r] += count[i]
    n_calls = int(free.max())
    slots = np.full((n_calls, B), total, dtype=np.int64)       # (total: the idle window)
    for i in order:
        slots[first[i]:first[i] + count[i], row[i]] = np.arange(offset[i], offset[i] + count[i])
    return Plan(B, T, n_calls, row, first, count, sizes, X, Y, Z, slots)


def bits_of(probs):
    """-sum log2(max(p, 1e-99)) over all but the first character (the clamp of rating.py:531-576)"""
    p = np.asarray(probs, dtype=np.float64)[1:]
    return float(-np.log2(np.maximum(p, 1e-99)).sum()) if len(p) else 0.0
