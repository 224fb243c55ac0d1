"""Segment streams: cut a few long files into as many contiguous pieces as there are stateful streams.

`Rater.train` trains `streams * world` independent stateful streams; without this module a stream is a list of FILES, so a
corpus of two texts trains at two streams.  With `Rater.segment_streams` a group of files (training, validation) that has
fewer files than streams is cut into **segments**, and a stream is a list of segments.

A file of `size` characters at window length T has F = len(range(T, size, T)) full windows and one tail window iff
F * T + 1 < size (`windows.stateful_windows`); number its windows 0 .. W - 1.  A segment is a run of windows [a, b) of ONE
file, i.e. the character slice [a * T, b * T + 1) -- one character of overlap: the last target -- or [a * T, size) when
b == W (the last segment keeps the tail).  Cuts lie on window boundaries only, so `stateful_windows` of the slice yields
exactly the windows a .. b - 1 of the file: an epoch sees the same (input, target) windows as file-wise training, only the
points where the carried state is reset move (and with them the order in which the augmentation numbers are drawn).

The plan is a pure function of (file sizes in their order, T, number of streams): every rank of a data-parallel run derives
the same one from the file order rank 0 broadcasts."""
from __future__ import annotations


def window_count(size, length):
    """number of windows of a file (== windows.count_windows): full ones, plus the tail"""
    full = len(range(length, size, length))
    return full + (1 if full * length + 1 < size else 0)


def char_slice(size, length, a, b):
    """the characters [lo, hi) of a file of `size` characters that hold its windows a .. b - 1"""
    assert 0 <= a < b <= window_count(size, length)
    return a * length, (size if b == window_count(size, length) else b * length + 1)


def _apportion(wins, n):
    """n segments over files with `wins` windows each (n <= sum(wins)): every file with a window gets one, the others go
    by window count (largest remainder), no file gets more segments than it has windows"""
    active = [k for k, w in enumerate(wins) if w > 0]
    rest = n - len(active)
    assert rest >= 0
    extra = dict.fromkeys(active, 0)
    capped = set()
    while True:
        open_ = [k for k in active if k not in capped]
        left = rest - sum(extra[k] for k in capped)
        if not open_:
            assert left == 0
            break
        total = sum(wins[k] for k in open_)
        for k in open_:
            extra[k] = left * wins[k] // total
        spare = left - sum(extra[k] for k in open_)
        for k in sorted(open_, key=lambda k: (-(left * wins[k] % total), k))[:spare]:
            extra[k] += 1
        over = [k for k in open_ if 1 + extra[k] > wins[k]]
        if not over:
            break
        for k in over:       # (a short file cannot take its share: it is cut into single windows, the others share the rest)
            extra[k] = wins[k] - 1
            capped.add(k)
    counts = [0] * len(wins)
    for k in active:
        counts[k] = 1 + extra[k]
    return counts


def plan(sizes, length, n_streams, strict=True):
    """The segments of a group of files: a list of (file index, a, b) -- windows [a, b) of that file --, file by file in order.

    Exactly `n_streams` segments when the group has that many windows: every file with a window gets at least one, the rest
    are apportioned by window count, and inside a file the segments' window counts differ by at most one.  Files without
    any window get no segment.  With fewer windows than streams: an AssertionError if `strict` (training), else one segment
    per window (validation: the caller's streams left over fall back to the first segment, as streams without a file of
    their own fall back to the first file)."""
    wins = [window_count(int(s), length) for s in sizes]
    total = sum(wins)
    n = int(n_streams)
    if total < n:
        assert not strict, \
            "segment_streams: the training files hold %d windows of %d characters, fewer than %d streams: lower `streams`" \
            % (total, length, n)
        n = total
    if len([w for w in wins if w > 0]) > n:       # (not reached from Rater.train: it segments groups with fewer files than streams)
        return [(k, 0, w) for k, w in enumerate(wins) if w > 0]
    out = []
    for k, c in enumerate(_apportion(wins, n)):
        a = 0
        for j in range(c):
            b = a + wins[k] // c + (1 if j < wins[k] % c else 0)
            out.append((k, a, b))
            a = b
    return out


def char_plan(sizes, length, n_streams, strict=True):
    """`plan` as character slices: a list of (file index, lo, hi)"""
    return [(k,) + char_slice(int(sizes[k]), length, a, b) for k, a, b in plan(sizes, length, n_streams, strict)]


def deal(items, rank, per_rank, n_streams):
    """what the `per_rank` streams of `rank` take: global stream gid = rank * per_rank + s takes items[gid::n_streams]
    (as files are dealt); a stream without an item of its own falls back to the first one"""
    return [items[rank * per_rank + s::n_streams] or items[:1] for s in range(per_rank)]
