"""HipLM._plan_512 (how a batch of stateful streams is cut into groups the width-512 scans take) as plain host logic: no GPU."""
import pytest

from ocrd_keraslm_amd.lib.engine import HipLM


class _Self(object):
    pad_streams = True
    plan_override = None


@pytest.mark.parametrize("B,limit,want", [
    (300, 3072, [(300, 300)]), (512, 3072, [(512, 512)]),
    (520, 3072, [(520, 1024)]), (1000, 3072, [(1000, 1024)]), (1280, 3072, [(1280, 1536)]),
    (2560, 3072, [(2560, 2560)]), (3000, 3072, [(3000, 3072)]), (3072, 3072, [(3072, 3072)]),
    (3073, 3072, [(2560, 2560), (513, 1024)]),                       # (never a single block of 512 at the end)
    (3584, 3072, [(2560, 2560), (1024, 1024)]), (4096, 3072, [(3072, 3072), (1024, 1024)]),
    (6144, 3072, [(3072, 3072), (3072, 3072)]),
    (10000, 3072, [(3072, 3072), (3072, 3072), (3072, 3072), (784, 1024)]),
    (4096, 16383, [(3072, 3072), (1024, 1024)]),                     # (short windows: still at most six row blocks per workgroup)
    (3000, 2047, [(1536, 1536), (1464, 1536)]),                      # (long windows: fewer streams per launch sequence)
])
def test_plan(B, limit, want):
    plan = HipLM._plan_512(_Self(), B, limit)
    assert plan == want
    assert sum(n for n, _ in plan) == B
    assert all(n <= run <= max(limit, 512) and (run % 512 == 0 or run == n) for n, run in plan)


def test_windows_too_long_for_1024_streams():
    """at T >= ~1024 fewer than 1024 streams fit the 32-bit offsets of a launch sequence -- no second-generation
    count applies, and the batch must still come back in groups the kernels address, not as one oversized group"""
    plan = HipLM._plan_512(_Self(), 2000, 700)
    assert sum(n for n, _ in plan) == 2000
    assert all(n == run and n <= 700 for n, run in plan), plan
    plan = HipLM._plan_512(_Self(), 2000, 1023)
    assert sum(n for n, _ in plan) == 2000 and all(run <= 1023 for _, run in plan), plan


def _engine_like(pwidth, pad_streams, max_streams):
    """what _stream_groups / _padded_streams / _plan_512 read of an engine, without one"""
    lm = HipLM.__new__(HipLM)
    lm.pwidth, lm.pad_streams, lm.plan_override, lm.max_streams_per_launch = pwidth, pad_streams, None, max_streams
    return lm


def _stream_counts(top=8200):
    """every multiple of 16 (so of 128 and of 512) up to `top` with both neighbours, and every count up to 130"""
    out = set(range(1, 131))
    for m in range(16, top + 1, 16):
        out.update((m - 1, m, m + 1))
    return sorted(b for b in out if 1 <= b <= top)


ADDRESSED = 0xfffffff0      # bytes of a layer's gate rows, Bp * T * 4W bf16, that the scans' 32-bit offsets reach (engine.py)


@pytest.mark.parametrize("pwidth", [128, 256, 512, 1024])
@pytest.mark.parametrize("pad_streams", [True, False])
def test_plan_invariants(pwidth, pad_streams):
    """What train_window / forward_window rely on, over every window length class and stream count around every multiple of
    16, 128 and 512 up to 8200, padding on and off, and three values of max_streams_per_launch (0 = what the kernels address,
    64, and 3000 -- more than long windows address): the groups are non-empty, ordered and partition [0, B); a padded count
    is at least the group and within the 32-bit offsets; at width 512 it is the `run` _plan_512 planned; the dummy streams of
    a group are at most as many as its real ones (train_window extends the keep-masks by m[:, :Bp - n], which silently yields
    too few rows otherwise); the weights n / B sum to 1."""
    counts = _stream_counts()
    for max_streams in (0, 64, 3000):
        lm = _engine_like(pwidth, pad_streams, max_streams)
        for T in (1, 2, 3, 5, 64, 256, 512, 800, 1024):
            limit = ADDRESSED // (T * 4 * pwidth * 2)
            for B in counts:
                where = (pwidth, pad_streams, max_streams, T, B)
                parts = lm._stream_groups(B, T)
                assert parts and parts[0][0] == 0 and parts[-1][1] == B, (where, parts)
                assert all(b0 < b1 for b0, b1 in parts), (where, parts)
                assert all(a[1] == b[0] for a, b in zip(parts, parts[1:])), (where, parts)
                padded = [lm._padded_streams(b1 - b0, T) for b0, b1 in parts]
                planned = None
                if pwidth == 512 and T >= 3 and not max_streams:
                    planned = lm._plan_512(B, limit)
                    assert [n for n, _run in planned] == [b1 - b0 for b0, b1 in parts], (where, parts, planned)
                total = 0.0
                for i, ((b0, b1), Bp) in enumerate(zip(parts, padded)):
                    n = b1 - b0
                    assert Bp >= n, (where, parts, padded)
                    assert Bp * T * 4 * pwidth * 2 <= ADDRESSED, (where, parts, padded)
                    if max_streams:
                        assert n <= max_streams and Bp == n, (where, parts, padded)
                    if planned is not None:
                        assert Bp == planned[i][1], (where, parts, padded, planned)
                    if Bp != n:
                        assert pad_streams and Bp - n <= n, (where, parts, padded)
                    total += n / B
                assert abs(total - 1.0) <= 4 * len(parts) * 2.0 ** -53, (where, total)


def test_plan_handed_in():
    """a plan handed in (tests do) reaches both the groups and the padded counts"""
    lm = _engine_like(512, True, 0)
    lm.plan_override = [(1024, 1024), (520, 1024)]
    assert lm._stream_groups(1544, 3) == [(0, 1024), (1024, 1544)]
    assert [lm._padded_streams(n, 3) for n in (1024, 520)] == [1024, 1024]


def test_no_padding_when_switched_off():
    s = _Self()
    s.pad_streams = False
    assert HipLM._plan_512(s, 3000, 3072) == [(3000, 3000)]
    assert HipLM._plan_512(s, 5000, 3072) == [(3072, 3072), (1928, 1928)]
