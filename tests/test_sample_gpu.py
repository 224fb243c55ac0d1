"""Sampling on the GPU (-m gpu), all through the C ABI:
  * kl_sample_pick's uniform numbers against gensample.philox_uniform, bit for bit;
  * its picks on synthetic probabilities against the numpy statement (gensample): the pick is in the exact candidate set (both
    sides compare float32 values), has a positive float64 weight, and sits where the float64 running sums put u * S, give or
    take m * S with m = 1e-4: |ln p| <= 14 here and temperature >= 0.5, so a weight's exponent is at most 28 in size, a few
    ulp of float32 on it are about 1e-5 relative on the weight, and m is ten times that; the cost within 2e-6 relative (the
    bar tests/test_device_beam_gpu.py uses for the same logf and one addition);
  * determinism, aliased cum_in / cum_next, the refusals with nothing launched;
  * `Rater.sample` on the HIP engine: every logged pick against the probabilities its step saw."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import gensample
from tests.test_device_beam_gpu import generate_rater, hip_factory

pytestmark = pytest.mark.gpu

M_SLACK = 1e-4
FLOOR = 0.004
KL_ERR_WORKSPACE, KL_ERR_ARG = 4, 5


@pytest.fixture(scope="module")
def sample_lib():
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    assert torch.cuda.is_available()
    lib = hipabi.load()
    handles = {}

    def handle(V):
        if V not in handles:
            cfg = hipabi.KlConfig(1, 64, V, 1, 200, 10)
            handles[V] = lib.kl_create(C.byref(cfg))
            assert handles[V]
        return handles[V]

    yield lib, handle
    torch.cuda.synchronize()
    for h in handles.values():
        lib.kl_destroy(h)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Call(object):
    """device copies of one case's inputs and pattern-filled outputs; `pick` is one kl_sample_pick on the current stream"""

    def __init__(self, lib, h, probs, cum_in, valid=None):
        import torch
        self.torch, self.lib, self.h = torch, lib, h
        dev = self.dev = torch.device("cuda:0")
        self.rows = probs.shape[0]
        self.p = torch.from_numpy(np.ascontiguousarray(probs)).to(dev)
        self.cum_in = torch.from_numpy(cum_in).to(dev)
        self.valid = torch.from_numpy(valid).to(dev) if valid is not None else None
        self.need = int(lib.kl_sample_workspace_bytes(h, self.rows))
        self.ws = torch.zeros(max(self.need, 1 << 16), dtype=torch.uint8, device=dev)

    def pick(self, temperature, top_k, floor, seed, step, rows=None, valid="own", ws_bytes=None, null=(), cum_out=None, want_u=True):
        torch = self.torch
        rows = self.rows if rows is None else rows
        n_out = max(self.rows, 1)
        idx = torch.full((n_out,), -77, dtype=torch.int32, device=self.dev)
        cum = torch.full((n_out,), -77.0, dtype=torch.float32, device=self.dev) if cum_out is None else cum_out
        u = torch.full((n_out,), -77.0, dtype=torch.float32, device=self.dev)
        args = dict(probs=self.p, cum_in=self.cum_in, idx_next=idx, cum_next=cum)
        for name in null:
            args[name] = None
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        code = self.lib.kl_sample_pick(self.h, rows, _ptr(args["probs"]), _ptr(self.valid if valid == "own" else valid),
                                       float(temperature), int(top_k), float(floor), int(seed), int(step), _ptr(args["cum_in"]),
                                       _ptr(args["idx_next"]), _ptr(args["cum_next"]), _ptr(u if want_u else None), _ptr(self.ws),
                                       self.need if ws_bytes is None else ws_bytes, stream)
        return code, idx, cum, u


def build_probs(V, rows, seed):
    """[rows][V] float32, every entry exactly 0 or >= 1e-6, rows normalised; by row number (shifted by V, so that one-row cases
    differ): plain; exact ties, also of the maximum; a peaked row (one entry 1 - 1e-6); zeros; nothing valid reaches the
    floor; id 0 and id 5 (which the mask removes) carrying large probabilities; all entries equal; entries at 0.004f and the
    float32 below"""
    rng = np.random.default_rng(seed)
    out = np.zeros((rows, V), dtype=np.float32)
    open_ids = np.array([v for v in range(1, V) if v != 5])      # valid with and without the mask
    below = np.nextafter(np.float32(FLOOR), np.float32(0))
    for r in range(rows):
        kind = (r + V) % 8
        p = rng.random(V) ** 4 + 1e-3 / V
        fixed = None
        if kind == 1:
            p[rng.choice(V, 3, replace=False)] = p.max()
            p[rng.choice(V, 2, replace=False)] = np.median(p)
        elif kind == 2:
            a, b = rng.choice(open_ids, 2, replace=False)
            p[:] = 0
            p[a], p[b] = 1 - 1e-6, 1.0000001e-6
            fixed = True
        elif kind == 3:
            p[rng.random(V) < 0.5] = 0
            p[rng.choice(open_ids)] = 0.5
        elif kind == 4:
            p[:] = rng.uniform(0.2, 1.0, V) * min(0.0039, 0.5 / V)      # every valid id below the floor, none below 1e-6
            p[0] = 1 - p[1:].sum()
        elif kind == 5:
            p *= 0.4 / p.sum()
            p[0] += 0.35
            p[5 % V] += 0.25
        elif kind == 6:
            p[:] = 1.0
        if not fixed:
            p = p / p.sum()
            p[p < 2e-6] = 0                                    # (what is left only grows when the row is normalised again)
            p = p / p.sum()
        if kind == 7 and V >= 64:
            a, b, c = rng.choice(open_ids, 3, replace=False)
            p[[a, b, c]] = 0
            p *= (1 - 3 * FLOOR) / p.sum()                     # (by 0.98 or more: what was 2e-6 stays above 1e-6)
            p = p.astype(np.float32)
            p[a], p[b], p[c] = FLOOR, FLOOR, below
        out[r] = p.astype(np.float32)
    assert ((out == 0) | (out >= np.float32(1e-6))).all() and np.abs(out.sum(axis=1, dtype=np.float64) - 1).max() < 1e-5
    return out


# ---------------------------------------------------------------------- the uniform numbers
def test_uniform_numbers_are_philox_bit_for_bit(sample_lib):
    lib, handle = sample_lib
    V = 7
    probs = build_probs(V, 1024, 1)
    cum = np.zeros(1024, dtype=np.float32)
    for rows in (1, 5, 256, 1024):
        call = Call(lib, handle(V), probs[:rows], cum[:rows])
        for step in (0, 1, 2 ** 31):
            for seed in (0, 12345, 2 ** 40 + 7):
                for temperature in (1.0, 0.0):      # (u is computed at every temperature)
                    code, _idx, _cum, u = call.pick(temperature, 0, 0.0, seed, step)
                    assert code == 0
                    assert np.array_equal(u.cpu().numpy().view(np.uint32), gensample.philox_uniform(seed, step, rows).view(np.uint32))
    # kl_sample_pick_from continues the row numbers: what `Rater.sample` draws its second group of 1024 chains with
    import torch
    call = Call(lib, handle(V), probs[:6], cum[:6])
    idx = torch.full((6,), -77, dtype=torch.int32, device=call.dev)
    out = torch.full((2, 6), -77.0, dtype=torch.float32, device=call.dev)
    stream = C.c_void_p(torch.cuda.current_stream(call.dev).cuda_stream)
    code = lib.kl_sample_pick_from(call.h, 6, 1024, _ptr(call.p), None, 1.0, 0, 0.0, 2 ** 40 + 7, 2, _ptr(call.cum_in), _ptr(idx),
                                   _ptr(out[0]), _ptr(out[1]), _ptr(call.ws), call.need, stream)
    assert code == 0
    assert np.array_equal(out[1].cpu().numpy(), gensample.philox_uniform(2 ** 40 + 7, 2, 1030)[1024:])


# ---------------------------------------------------------------------- pick parity
@pytest.mark.parametrize("rows", [1, 4, 5, 256])
@pytest.mark.parametrize("V", [7, 64, 200, 256, 257, 1000])
def test_picks_match_the_numpy_statement(sample_lib, V, rows):
    import torch
    lib, handle = sample_lib
    probs = build_probs(V, rows, seed=V * 1000 + rows)
    rng = np.random.default_rng(rows * 7 + V)
    cum_in = rng.uniform(0.5, 30.0, rows).astype(np.float32)
    mask = np.ones(V, dtype=np.uint8)
    mask[[0, 5]] = 0
    p64 = probs.astype(np.float64)
    at = np.arange(rows)
    used = 0.0
    step = 3
    for valid in (None, mask):
        call = Call(lib, handle(V), probs, cum_in, valid)
        for top_k in (0, 1, 3, 64):
            for floor in (0.0, FLOOR):
                cand, first = gensample.candidate_mask(probs, valid, top_k, floor)
                assert (first >= 0).all()
                for temperature in (0.0, 0.5, 1.0, 1.7):
                    seed = 1000 * top_k + int(temperature * 10) + (1 << 33)
                    code, idx, cum, u = call.pick(temperature, top_k, floor, seed, step)
                    torch.cuda.synchronize()
                    assert code == 0
                    idx, cum, u = idx.cpu().numpy(), cum.cpu().numpy(), u.cpu().numpy()
                    where = (V, rows, valid is not None, top_k, floor, temperature)
                    assert ((idx >= 0) & (idx < V)).all(), where
                    assert np.array_equal(u, gensample.philox_uniform(seed, step, rows)), where
                    assert cand[at, idx].all(), where                                                  # (a)
                    if temperature == 0:
                        assert np.array_equal(idx, first), where                                       # greedy: exact
                    else:
                        w = gensample.weights_host(probs, cand, first, temperature)
                        assert (w[at, idx] > 0).all(), where                                           # (b)
                        run = np.cumsum(w, axis=1)
                        S = run[:, -1]
                        target = u.astype(np.float64) * S
                        lo, hi = run[at, idx] - w[at, idx], run[at, idx]
                        assert (lo - M_SLACK * S <= target).all() and (target < hi + M_SLACK * S).all(), where      # (c)
                        if temperature == 1:
                            used = max(used, float((np.maximum(np.maximum(lo - target, target - hi), 0) / S).max()))
                    want = cum_in.astype(np.float64) - np.log(p64[at, idx])
                    assert (np.abs(cum - want) <= 2e-6 * np.abs(want)).all(), where                    # (d)
    print("V %d rows %d: at temperature 1 the device needed a slack of %.3g * S (allowed %.3g)" % (V, rows, used, M_SLACK))


def test_built_in_cases_are_there():
    """what build_probs promises, on the numpy side alone (it runs with the GPU tests it belongs to)"""
    V = 257
    probs = build_probs(V, 256, seed=V * 1000 + 256)
    mask = np.ones(V, dtype=np.uint8)
    mask[[0, 5]] = 0
    order = np.sort(probs, axis=1)[:, ::-1]
    assert (order[:, 0] == order[:, 2]).any()                                                   # ties of the maximum
    assert (probs >= np.float32(1 - 1e-6)).any() and (probs == 0).any()
    cand, first = gensample.candidate_mask(probs, mask, 0, FLOOR)
    nothing = ~(probs[np.arange(256), first] >= np.float32(FLOOR))
    assert nothing.any() and (cand[nothing].sum(axis=1) == 1).all()                             # nothing reaches the floor
    assert ((probs[:, 0] > 0.3) & (probs[:, 5] > 0.2)).any() and not cand[:, 0].any() and not cand[:, 5].any()
    assert (probs == np.float32(FLOOR)).any() and (probs == np.nextafter(np.float32(FLOOR), np.float32(0))).any()
    assert gensample.candidate_mask(build_probs(7, 5, 1), None, 64, 0.0)[0].sum(axis=1).max() <= 6      # V < top_k


# ---------------------------------------------------------------------- determinism, aliasing
@pytest.mark.parametrize("V", [64, 1000])
def test_same_call_twice_and_aliased_costs(sample_lib, V):
    import torch
    lib, handle = sample_lib
    rows = 256
    probs = build_probs(V, rows, seed=9)
    cum_in = np.random.default_rng(4).uniform(0.5, 30.0, rows).astype(np.float32)
    call = Call(lib, handle(V), probs, cum_in)
    for temperature, top_k in ((1.0, 0), (0.7, 20), (0.0, 0)):
        code, idx, cum, u = call.pick(temperature, top_k, 0.001, 77, 5)
        code2, idx2, cum2, u2 = call.pick(temperature, top_k, 0.001, 77, 5)
        separate = call.cum_in
        call.cum_in = own = separate.clone()
        code3, idx3, cum3, _u = call.pick(temperature, top_k, 0.001, 77, 5, cum_out=own, want_u=False)      # cum_next = cum_in, no u_log
        call.cum_in = separate
        torch.cuda.synchronize()
        assert code == code2 == code3 == 0
        assert torch.equal(idx, idx2) and torch.equal(cum.view(torch.int32), cum2.view(torch.int32)) and torch.equal(u, u2)
        assert torch.equal(idx, idx3) and torch.equal(cum.view(torch.int32), cum3.view(torch.int32))
        assert (_u == -77.0).all()
        other = call.pick(temperature, top_k, 0.001, 78, 5)[1]
        assert temperature == 0 or not torch.equal(idx, other)


# ---------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(sample_lib):
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib, handle = sample_lib
    V = 300
    probs = build_probs(V, 1025, seed=2)
    cum_in = np.ones(1025, dtype=np.float32)
    call = Call(lib, handle(V), probs, cum_in)
    call.need = int(lib.kl_sample_workspace_bytes(handle(V), 1024))
    call.ws = torch.zeros(call.need, dtype=torch.uint8, device=call.dev)
    assert call.need >= 1 and lib.kl_sample_workspace_bytes(handle(V), 0) == lib.kl_sample_workspace_bytes(handle(V), 1025) == 0
    good = dict(temperature=1.0, top_k=0, floor=0.0, seed=1, step=0, rows=1024)
    cases = [(dict(rows=0), KL_ERR_ARG), (dict(rows=1025), KL_ERR_ARG), (dict(top_k=-1), KL_ERR_ARG), (dict(top_k=65), KL_ERR_ARG),
             (dict(temperature=-0.5), KL_ERR_ARG), (dict(temperature=float("nan")), KL_ERR_ARG), (dict(floor=-1e-3), KL_ERR_ARG),
             (dict(null=("probs",)), KL_ERR_ARG), (dict(null=("idx_next",)), KL_ERR_ARG), (dict(null=("cum_in",)), KL_ERR_ARG),
             (dict(null=("cum_next",)), KL_ERR_ARG), (dict(ws_bytes=call.need - 1), KL_ERR_WORKSPACE)]
    for kw, want in cases:
        code, idx, cum, u = call.pick(**{**good, **kw})
        torch.cuda.synchronize()
        assert code == want, (kw, code)
        # nothing was launched: every output still holds its pattern
        assert (idx == -77).all() and (cum == -77.0).all() and (u == -77.0).all(), kw
    code, idx, _cum, _u = call.pick(**good)      # (the same call, arguments in range: it runs)
    torch.cuda.synchronize()
    assert code == 0 and (idx[:1024] > 0).all()
    with pytest.raises(hipabi.KlError):
        hipabi.check(KL_ERR_ARG, "kl_sample_pick")


# ---------------------------------------------------------------------- Rater.sample on the HIP engine
def check_log(r, log, seed, temperature, top_k, floor, row0=0):
    """every logged pick against the probabilities its step saw: (a) to (c), the costs, the uniform numbers"""
    idx, cum, u, probs = log
    length, rows = idx.shape
    valid = np.zeros(r.voc_size, dtype=np.uint8)
    valid[list(r.mapping[1])] = 1
    at = np.arange(rows)
    before = np.zeros(rows)
    for s in range(length):
        assert np.array_equal(u[s], gensample.philox_uniform(seed, s, rows, row0))
        cand, first = gensample.candidate_mask(probs[s], valid, top_k, floor)
        assert cand[at, idx[s]].all()
        if temperature == 0:
            assert np.array_equal(idx[s], first)
        else:
            w = gensample.weights_host(probs[s], cand, first, temperature)
            assert (w[at, idx[s]] > 0).all()
            run = np.cumsum(w, axis=1)
            S, target = run[:, -1], u[s].astype(np.float64) * run[:, -1]
            assert (run[at, idx[s]] - w[at, idx[s]] - M_SLACK * S <= target).all() and (target < run[at, idx[s]] + M_SLACK * S).all()
        want = before - np.log(probs[s][at, idx[s]].astype(np.float64))
        assert (np.abs(cum[s] - want) <= 2e-6 * np.abs(want)).all()
        before = cum[s].astype(np.float64)


@pytest.mark.parametrize("variants", [8, 300])
@pytest.mark.parametrize("width", [64, 128])
def test_rater_sample_on_the_hip_engine(width, variants):
    prefix, ctx = "HELLO", [17]
    r = generate_rater(hip_factory, 2, width, 1, 2.0)
    assert hasattr(r.model, "sample_pick")
    r.sample_keep_probs = True
    pool = r._state_pool()
    pool.release_slots(pool.take_slots(2 * variants + len(prefix)))      # (grown beforehand: the free list is then the same before and after)
    free = sorted(pool.free)
    kw = dict(temperature=0.8, top_k=20, floor=0.001)
    for length in (12, 1):
        got = r.sample(prefix, length, ctx, variants, seed=3, **kw)
        (log,) = r.sample_log
        costs = list(r.sample_costs)
        assert sorted(pool.free) == free
        assert log[0].shape == (length, variants) and log[3].shape == (length, variants, r.voc_size)
        assert len(got) == variants and all(len(s) == length + 1 and s[0] == prefix[-1] for s in got)
        assert got == gensample.spell(log, r.mapping[1], prefix[-1]) and costs == [float(c) for c in log[1][-1]]
        check_log(r, log, 3, **kw)
        again = r.sample(prefix, length, ctx, variants, seed=3, **kw)
        assert again == got and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(log[:3], r.sample_log[0][:3]))
        assert r.sample(prefix, length, ctx, variants, seed=4, **kw) != got
    print("width %d, %d chains: %r ..." % (width, variants, got[:3]))
    plain = r.sample(prefix, 12, ctx, variants, seed=3)                  # the distribution itself
    check_log(r, r.sample_log[0], 3, 1.0, 0, 0.0)
    assert len(set(plain)) > 1
    cold = r.sample(prefix, 12, ctx, variants, temperature=0.0, seed=3)
    check_log(r, r.sample_log[0], 3, 0.0, 0, 0.0)
    assert len(set(cold)) == 1 and len(cold) == variants
    assert r.sample(prefix, 0, ctx, 2) == [prefix[-1]] * 2
    assert sorted(pool.free) == free
    # the slots come back when the call raises: on a bad argument, and on an engine failure in the middle
    with pytest.raises(ValueError):
        r.sample(prefix, 12, ctx, variants, top_k=65)
    assert sorted(pool.free) == free
    real, calls = r.model.sample_pick, []

    def failing(*args, **kwargs):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("engine failure in the middle of the chains")
        return real(*args, **kwargs)
    r.model.sample_pick = failing
    try:
        with pytest.raises(RuntimeError, match="in the middle"):
            r.sample(prefix, 12, ctx, variants, seed=3)
    finally:
        del r.model.sample_pick
    assert sorted(pool.free) == free
    assert r.sample(prefix, 12, ctx, variants, seed=3) == plain
