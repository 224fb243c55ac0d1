"""Host side of `Rater.sample`: drawing continuations from the model's distribution.

The numpy statement of kl_sample_pick (csrc/sample.hip, include/keraslm_hip.h) -- so it is that kernel's checker, and it is
what `Rater.sample` draws with on an engine without `sample_pick`:

  * `philox_uniform`: the uniform number of (seed, step, row) -- Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter
    (step, row, 0, 0), of the first output word x0 the float (x0 >> 8) * 2^-24.  Integer arithmetic: the same bits as the kernel's.
  * `candidates_host`: the valid ids (None: every id except 0); with top_k > 0 the first min(top_k, valid ids) of them in the
    order (p descending, id ascending); of those the ids with p >= floor (float32 comparison); if none is left, the first
    valid id of that order alone; if no id is valid, none.
  * `pick_host`: temperature 0 takes the first candidate.  Otherwise weight p (temperature 1) or
    exp((log p - log p_max) / temperature), 0 for p == 0; the pick is the smallest candidate id whose running weight sum, ids
    ascending, exceeds u * S; if rounding leaves none, the last candidate of positive weight; if no candidate has a positive
    weight, the first candidate.  Without a valid id the pick is 0.  Weights and sums are float64 here (the kernel's are float32).
  * `spell`: the strings of a log of picks.

Probabilities are compared as float32 values on both sides, so the candidate sets are exactly the kernel's.
"""
from __future__ import annotations

import numpy as np

MAX_ROWS = 1024      # chains per kl_sample_pick call; `Rater.sample` draws more in groups that continue the row numbers
MAX_TOP_K = 64

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)


def philox4x32(counter, key, rounds=10):
    """Philox4x32: counter = four arrays (or ints) of 32-bit words, key = two; returns the four output words (uint64 arrays
    holding 32-bit values)"""
    c = [np.asarray(w, dtype=np.uint64) & _MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(rounds):
        p0 = np.uint64(_M0) * c[0]            # (32 x 32 bits: fits 64)
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xffffffff, (k1 + _W1) & 0xffffffff
    return c


def philox_uniform(seed, step, rows, row0=0):
    """float32 [rows]: the uniform numbers in [0, 1) of rows row0 .. row0 + rows - 1 at `step` under `seed`"""
    seed = int(seed) & 0xffffffffffffffff
    r = (np.arange(int(rows), dtype=np.uint64) + np.uint64(int(row0) & 0xffffffff)) & _MASK
    x0 = philox4x32((int(step) & 0xffffffff, r, 0, 0), (seed & 0xffffffff, seed >> 32))[0]
    return ((x0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def check_args(temperature, top_k, floor):
    """what kl_sample_pick refuses, refused here"""
    if not (temperature >= 0 and np.isfinite(temperature)):
        raise ValueError("temperature must be >= 0 and finite, not %r" % (temperature,))
    if int(top_k) != top_k or not 0 <= top_k <= MAX_TOP_K:
        raise ValueError("top_k must be 0 .. %d (0: off), not %r" % (MAX_TOP_K, top_k))
    if not floor >= 0:
        raise ValueError("floor must be >= 0, not %r" % (floor,))


def _valid(valid, V):
    return (np.arange(V) != 0) if valid is None else (np.asarray(valid).reshape(-1)[:V] != 0)


def candidate_mask(p, valid=None, top_k=0, floor=0.0):
    """p [rows][V] -> (mask [rows][V] bool: is a candidate; first [rows]: the first candidate in (p descending, id
    ascending) order, -1 where no id is valid)"""
    p = np.asarray(p, dtype=np.float32)
    rows, V = p.shape
    ok = _valid(valid, V)
    ids = np.broadcast_to(np.arange(V), p.shape)
    order = np.lexsort((ids, -p), axis=-1)                          # p descending, equal values by id ascending
    ok_o = np.broadcast_to(ok, p.shape)[np.arange(rows)[:, None], order]
    keep = ok_o & (np.take_along_axis(p, order, axis=1) >= np.float32(floor))
    if top_k > 0:
        keep &= np.cumsum(ok_o, axis=1) <= int(top_k)                 # among the first top_k VALID ids
    has = ok_o.any(axis=1)
    first_at = ok_o.argmax(axis=1)
    none = has & ~keep.any(axis=1)
    keep[none, first_at[none]] = True                                # nothing reaches the floor: the first valid id alone
    mask = np.zeros(p.shape, dtype=bool)
    np.put_along_axis(mask, order, keep, axis=1)
    first = np.where(has, order[np.arange(rows), first_at], -1)
    return mask, first


def candidates_host(p, valid=None, top_k=0, floor=0.0):
    """the candidate ids of ONE row p [V], in (p descending, id ascending) order (so [0] is the greedy pick); empty if no id
    is valid"""
    p = np.asarray(p, dtype=np.float32).reshape(1, -1)
    mask, _first = candidate_mask(p, valid, top_k, floor)
    ids = np.flatnonzero(mask[0])
    return ids[np.lexsort((ids, -p[0, ids]))]


def weights_host(p, mask, first, temperature):
    """float64 [rows][V]: the weights of the candidates (0 elsewhere) at a temperature > 0"""
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64)
    if temperature == 1:
        w = p64.copy()
    else:
        p_max = p64[np.arange(len(p64)), np.maximum(first, 0)]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.exp((np.log(p64) - np.log(p_max)[:, None]) / float(temperature))
    w[~mask | ~(p64 > 0)] = 0.0
    return w


def pick_host(p, u, valid=None, temperature=1.0, top_k=0, floor=0.0):
    """The pick of every row: p [rows][V] and u [rows] -> int32 [rows]; or of one row: p [V] and a number u -> int."""
    check_args(temperature, top_k, floor)
    p = np.asarray(p, dtype=np.float32)
    if p.ndim == 1:
        return int(pick_host(p[None, :], np.asarray([u]), valid, temperature, top_k, floor)[0])
    mask, first = candidate_mask(p, valid, top_k, floor)
    pick = np.maximum(first, 0)
    if temperature == 0:
        return pick.astype(np.int32)
    w = weights_host(p, mask, first, temperature)
    run = np.cumsum(w, axis=1)                                       # ids ascending
    target = np.asarray(u, dtype=np.float64).reshape(-1) * run[:, -1]
    positive = w > 0
    beyond = positive & (run > target[:, None])
    last = p.shape[1] - 1 - positive[:, ::-1].argmax(axis=1)
    pick = np.where(positive.any(axis=1), last, pick)                # rounding left none: the last of positive weight
    pick = np.where(beyond.any(axis=1), beyond.argmax(axis=1), pick)
    return pick.astype(np.int32)


def spell(log, i_c, first_char):
    """One string per chain from log = (idx [length][rows], ...): `first_char` (the last character of the prefix) and the
    characters of the chain's picks"""
    idx = np.asarray(log[0])
    return [first_char + ''.join(i_c[int(i)] for i in idx[:, r]) for r in range(idx.shape[1])]
