"""Sampling on the CPU: `gensample` (the numpy statement of kl_sample_pick) against a brute-force statement of the same
rules and against the binomial law, the Philox numbers against the published known-answer vector, `Rater.sample` on the
CPU double -- through `_predict_refs` and, on a double that offers `sample_pick` / `sample_generate` through gensample,
through the device path's bookkeeping --, and the command line's `generate --sample`."""
import math
import os
import tempfile

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import Rater, gensample
from tests.oracle_engine import OracleLM


# ---------------------------------------------------------------------- Philox
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: zero counter and key; all-ones counter and key"""
    words = [int(w) for w in gensample.philox4x32((0, 0, 0, 0), (0, 0))]
    assert words == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = [int(w) for w in gensample.philox4x32((0xffffffff,) * 4, (0xffffffff,) * 2)]
    assert ones == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # the product's number: the first word's upper 24 bits
    assert gensample.philox_uniform(0, 0, 1)[0] == np.float32((0x6627e8d5 >> 8) * 2.0 ** -24)


def test_philox_uniform_is_a_pure_function_of_seed_step_and_row():
    u = gensample.philox_uniform(12345, 7, 1024)
    assert u.dtype == np.float32 and u.shape == (1024,) and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u, gensample.philox_uniform(12345, 7, 1024))
    assert np.array_equal(u[:5], gensample.philox_uniform(12345, 7, 5))                      # a row's number does not depend on the row count
    assert np.array_equal(u[100:], gensample.philox_uniform(12345, 7, 924, row0=100))        # ... nor on where the group starts
    far = gensample.philox_uniform(12345, 7, 3000)
    assert np.array_equal(far[2048:], gensample.philox_uniform(12345, 7, 952, row0=2048))
    assert len(set(far.tolist())) > 2990                                                      # (24 bits: a handful may coincide)
    seen = {}
    for seed in (0, 1, 12345, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7, 2 ** 63 + 1):               # seeds that differ only above bit 32 too
        for step in (0, 1, 2, 2 ** 31, 2 ** 32 - 1):
            seen[(seed, step)] = tuple(gensample.philox_uniform(seed, step, 8).tolist())
    assert len(set(seen.values())) == len(seen)
    assert all(len(set(v)) == 8 for v in seen.values())


# ---------------------------------------------------------------------- pick_host against a brute-force statement
def brute_candidates(p, valid, top_k, floor):
    V = len(p)
    ok = [v for v in range(V) if (valid[v] if valid is not None else v != 0)]
    if not ok:
        return []
    order = sorted(ok, key=lambda v: (-float(p[v]), v))
    cand = [v for v in (order[:top_k] if top_k > 0 else order) if p[v] >= np.float32(floor)]
    return cand or [order[0]]


def brute_weights(p, cand, temperature):
    p_max = max(float(p[v]) for v in cand)
    return {v: 0.0 if p[v] == 0 else (float(p[v]) if temperature == 1 else
                                      math.exp((math.log(float(p[v])) - math.log(p_max)) / temperature)) for v in cand}


def brute_pick(p, u, valid, temperature, top_k, floor):
    cand = brute_candidates(p, valid, top_k, floor)
    if not cand:
        return 0
    if temperature == 0:
        return cand[0]
    w = brute_weights(p, cand, temperature)
    total = 0.0
    for v in sorted(cand):
        total += w[v]
    run = 0.0
    for v in sorted(cand):
        run += w[v]
        if w[v] > 0 and run > float(u) * total:
            return v
    positive = [v for v in sorted(cand) if w[v] > 0]
    return positive[-1] if positive else cand[0]


def small_rows(V):
    """rows of V probabilities with what the rules turn on: ties (also of the maximum), zeros, a floor that keeps some, all
    or none, id 0 and a masked id in front"""
    rng = np.random.default_rng(V)
    rows = []
    for n in range(24):
        p = rng.random(V) ** 3
        if n % 3 == 0:
            p[rng.choice(V, 2, replace=False)] = 0.0
        if n % 4 == 1:
            p[rng.choice(V, 3, replace=False)] = p.max()                  # the maximum, three times
        if n % 4 == 2:
            p[0], p[2] = 5.0, 4.0                                         # id 0 and id 2 (masked below) in front
        if n % 6 == 5:
            p[1:] *= 1e-3                                                 # nothing but id 0 reaches the floor
            p[0] = 1.0
        rows.append((p / p.sum()).astype(np.float32))
    rows.append(np.full(V, 1.0 / V, dtype=np.float32))                    # all equal
    only = np.zeros(V, dtype=np.float32)
    only[0] = 1.0                                                         # every id that may be drawn has probability 0
    rows.append(only)
    return np.stack(rows)


@pytest.mark.parametrize("V", [5, 7])
def test_pick_host_equals_the_brute_force_statement(V):
    p = small_rows(V)
    mask = np.ones(V, dtype=np.uint8)
    mask[[0, 2]] = 0
    us = np.array([0.0, 1e-7, 0.25, 0.5, 0.75, 1 - 2.0 ** -24], dtype=np.float32)
    seen = set()
    for valid in (None, mask, np.zeros(V, dtype=np.uint8)):
        for top_k in range(0, V + 2):
            for floor in (0.0, 0.05):
                for r in range(len(p)):
                    want = brute_candidates(p[r], valid, top_k, floor)
                    assert gensample.candidates_host(p[r], valid, top_k, floor).tolist() == want
                    if want and not p[r][want[0]] >= np.float32(floor):
                        seen.add("below the floor")
                    if len(want) > 1 and p[r][want[0]] == p[r][want[1]]:
                        assert want[0] < want[1]
                        seen.add("tie")
                for temperature in (0.0, 0.5, 1.0, 1.7):
                    for u in us:
                        got = gensample.pick_host(p, np.full(len(p), u), valid, temperature, top_k, floor)
                        want = [brute_pick(p[r], u, valid, temperature, top_k, floor) for r in range(len(p))]
                        assert got.tolist() == want, (valid, top_k, floor, temperature, u)
                        assert gensample.pick_host(p[3], u, valid, temperature, top_k, floor) == want[3]      # the one-row form
                        for r, v in enumerate(want):
                            cand = brute_candidates(p[r], valid, top_k, floor)
                            if not cand:
                                assert v == 0
                                seen.add("no valid id")
                            elif temperature == 0:
                                assert v == cand[0]                                    # greedy
                            elif any(p[r][c] > 0 for c in cand):
                                assert p[r][v] > 0                                     # a candidate of weight 0 is never picked
                                if any(p[r][c] == 0 for c in cand):
                                    seen.add("zero among candidates")
                            else:
                                assert v == cand[0]
                                seen.add("only zeros")
    assert seen == {"below the floor", "tie", "no valid id", "zero among candidates", "only zeros"}


def test_pick_host_refuses_what_the_kernel_refuses():
    p = np.full(5, 0.2, dtype=np.float32)
    for kw in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1),
               dict(top_k=65), dict(floor=-0.1), dict(floor=float("nan"))):
        with pytest.raises(ValueError):
            gensample.pick_host(p, 0.5, **kw)


@pytest.mark.parametrize("temperature,top_k", [(1.0, 0), (0.7, 0), (1.0, 4)])
def test_pick_host_frequencies_follow_the_weights(temperature, top_k):
    """200 000 Philox draws on one fixed row: the count of entry v is binomial (N, q_v = w_v / S), so it stays within 5
    standard deviations sqrt(N q (1 - q)) of N q (a chance of 6e-7 per entry to fail by accident; the 2^-24 grid of u
    moves q by less than 1e-7, a thousandth of the smallest deviation allowed here)"""
    p = np.array([0.05, 0.3, 0.1, 0.25, 0.2, 0.1], dtype=np.float32)
    valid = np.ones(6, dtype=np.uint8)
    steps, rows = 200, 1000
    cand = brute_candidates(p, valid, top_k, 0.0)
    w = brute_weights(p, cand, temperature)
    q = np.array([w.get(v, 0.0) for v in range(6)]) / sum(w.values())
    counts = np.zeros(6)
    for step in range(steps):
        u = gensample.philox_uniform(2 ** 40 + 7, step, rows)
        picks = gensample.pick_host(np.tile(p, (rows, 1)), u, valid, temperature, top_k, 0.0)
        counts += np.bincount(picks, minlength=6)
    N = steps * rows
    sigma = np.sqrt(N * q * (1 - q))
    print("counts %s expected %s sigma %s" % (counts, N * q, sigma))
    assert (np.abs(counts - N * q) <= 5 * sigma).all()
    assert (counts[q == 0] == 0).all() and (len(cand) == 6 or (q == 0).sum() == 2)


def test_abi_refusals_need_no_device():
    """KL_ERR_ARG and KL_ERR_WORKSPACE come back before anything is launched, so no pointer is ever followed: made-up
    addresses do, and the test runs without a GPU (tests/test_sample_gpu.py repeats it on real buffers and looks at them)"""
    import ctypes as C
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    cfg = hipabi.KlConfig(1, 64, 300, 1, 200, 10)
    h = lib.kl_create(C.byref(cfg))
    assert h
    try:
        need = lib.kl_sample_workspace_bytes(h, 1024)
        assert need >= 1024 * 300 * 4 and lib.kl_sample_workspace_bytes(h, 1) >= 300 * 4
        assert lib.kl_sample_workspace_bytes(h, 0) == lib.kl_sample_workspace_bytes(h, 1025) == lib.kl_sample_workspace_bytes(None, 8) == 0
        fake = C.c_void_p(0x1000)
        good = dict(h=h, rows=1024, probs=fake, valid=None, temperature=1.0, top_k=0, floor=0.0, seed=1, step=0, cum_in=fake,
                    idx_next=fake, cum_next=fake, u_log=None, ws=fake, ws_bytes=need - 1, stream=None)
        order = ("h", "rows", "probs", "valid", "temperature", "top_k", "floor", "seed", "step", "cum_in", "idx_next", "cum_next",
                 "u_log", "ws", "ws_bytes", "stream")
        assert lib.kl_sample_pick(*[good[k] for k in order]) == 4                  # KL_ERR_WORKSPACE: one byte short
        assert lib.kl_sample_pick(*[dict(good, ws=None, ws_bytes=need)[k] for k in order]) == 4
        for kw in (dict(rows=0), dict(rows=1025), dict(top_k=-1), dict(top_k=65), dict(temperature=-0.5), dict(temperature=float("nan")),
                   dict(temperature=float("inf")), dict(floor=-1e-3), dict(floor=float("nan")), dict(probs=None), dict(idx_next=None),
                   dict(cum_in=None), dict(cum_next=None), dict(h=None)):
            args = dict(good, ws_bytes=need, **kw)
            assert lib.kl_sample_pick(*[args[k] for k in order]) == 5, kw        # KL_ERR_ARG
            assert lib.kl_sample_pick_from(*([args[k] for k in order[:2]] + [7] + [args[k] for k in order[2:]])) == 5, kw
    finally:
        lib.kl_destroy(h)


# ---------------------------------------------------------------------- Rater.sample on the CPU double
class SampleOracle(OracleLM):
    """OracleLM (float32, as the HIP engine delivers) that offers the device path's two calls through gensample"""

    def __init__(self, *args, **kwargs):
        kwargs.setdefault("dtype", np.float32)
        super().__init__(*args, **kwargs)
        self.sample_generates = []
        self.picks = 0
        self.fail_at = None

    def sample_pick(self, probs, cum_in, temperature, top_k, floor, seed, step, valid=None, out=None, row0=0):
        self.picks += 1
        if self.fail_at is not None and self.picks >= self.fail_at:
            raise RuntimeError("engine failure in the middle of the chains")
        rows = len(cum_in)
        u = gensample.philox_uniform(seed, step, rows, row0)
        idx = gensample.pick_host(probs, u, valid, temperature, top_k, floor)
        with np.errstate(divide="ignore"):
            cum = (np.asarray(cum_in, dtype=np.float32) - np.log(probs[np.arange(rows), idx].astype(np.float32))).astype(np.float32)
        return idx, cum, u

    def sample_generate(self, idx0, slot0, ctx, length, rows, temperature, top_k, floor, seed, valid, slots_a, slots_b, zero_slot,
                        keep_probs=False, row0=0):
        self.sample_generates.append((rows, row0))
        sets = (np.asarray(slots_a, dtype=np.int32), np.asarray(slots_b, dtype=np.int32))
        assert len(sets[0]) == len(sets[1]) == rows and slot0 not in set(sets[0]) | set(sets[1])
        ctx_rows = np.tile(np.asarray(ctx, dtype=np.int32).reshape(1, -1), (rows, 1))
        idx, slot_in, cum = np.full(rows, idx0, dtype=np.int32), np.full(rows, slot0, dtype=np.int32), np.zeros(rows, dtype=np.float32)
        log = ([], [], [], [])
        for s in range(length):
            probs = self.step_slots(idx, ctx_rows, slot_in, sets[s & 1])
            idx, cum, u = self.sample_pick(probs, cum, temperature, top_k, floor, seed, s, valid, row0=row0)
            slot_in = sets[s & 1]
            for part, value in zip(log, (idx, cum, u, probs)):
                part.append(value)
        return tuple(np.stack(part) for part in (log if keep_probs else log[:3]))


def make_rater(factory, seed=2, emb_std=1.0):
    chars = [chr(c) for c in range(0x41, 0x41 + 60)]          # (tests/test_device_beam.py's model)
    r = Rater(engine_factory=factory)
    r.width, r.depth, r.length = 16, 1, 8
    r.stateful, r.incremental = False, True
    r.mapping = ({c: i + 1 for i, c in enumerate(chars)}, {i + 1: c for i, c in enumerate(chars)})
    r.voc_size = len(chars) + 1
    r.configure()
    r.model.init_weights(seed=seed, emb_std=emb_std)
    r.status = 2
    return r


def chain_costs(r, prefix, text, ctx):
    """-log p of every character of `text` after the first, one step at a time with the states kept in the engine's pool (at
    its own precision; `predict` would hand them through float32), and the greedy character at each place"""
    state = None
    for char in prefix[:-1]:
        _, states = r._predict_refs([char], [state], ctx)
        state = states[0]
    costs, greedy = [], []
    for char, nxt in zip(text[:-1], text[1:]):
        preds, states = r._predict_refs([char], [state], ctx)
        state = states[0]
        costs.append(-math.log(preds[0][r.mapping[0][nxt]]))
        greedy.append(r.mapping[1][1 + int(np.argmax(preds[0][1:].astype(np.float32)))])
    return costs, greedy


def test_sample_on_the_oracle_engine():
    r = make_rater(OracleLM)
    ctx = [17]
    got = r.sample("ABC", 12, ctx, 3, seed=5)
    costs = list(r.sample_costs)
    assert len(got) == 3 and all(len(s) == 13 and s[0] == "C" for s in got) and len(set(got)) == 3
    assert r.sample("ABC", 12, ctx, 3, seed=5) == got and r.sample_costs == costs          # the same seed, the same strings
    assert r.sample("ABC", 12, ctx, 3, seed=6) != got
    assert r.sample("ABC", 12, ctx, 3, seed=5 + 2 ** 32) != got
    for text, cost in zip(got, costs):
        assert cost == pytest.approx(sum(chain_costs(r, "ABC", text, ctx)[0]), abs=1e-9)
    # the numbers the chains drew with, and what they made of them
    idx, _cum, u = r.sample("ABC", 12, ctx, 3, seed=5) and r.sample_log[0]
    assert all(np.array_equal(u[s], gensample.philox_uniform(5, s, 3)) for s in range(12))
    assert [''.join(r.mapping[1][int(i)] for i in idx[:, v]) for v in range(3)] == [s[1:] for s in got]
    # temperature 0: every chain is the greedy one
    cold = r.sample("ABC", 12, ctx, 3, temperature=0.0, seed=5)
    assert len(set(cold)) == 1 and list(cold[0][1:]) == chain_costs(r, "ABC", cold[0], ctx)[1]
    # top_k = 1 is greedy too, whatever the temperature
    assert r.sample("ABC", 12, ctx, 2, temperature=1.5, top_k=1, seed=9) == cold[:2]
    # a one-character prefix (no warm-up), length 0
    assert all(len(s) == 5 and s[0] == "Q" for s in r.sample("Q", 4, ctx, 2))
    assert r.sample("AB", 0, ctx, 3) == ["B"] * 3 and r.sample_costs == [0.0] * 3
    for kw in (dict(variants=0), dict(length=-1), dict(top_k=65), dict(temperature=-0.5), dict(floor=-1.0)):
        with pytest.raises(ValueError):
            r.sample("AB", **{"length": 4, "context": ctx, **kw})
    with pytest.raises(ValueError):
        r.sample("", 4, ctx)


def test_sample_more_than_1024_variants_runs_in_groups_that_continue_the_row_numbers():
    r = make_rater(OracleLM)
    ctx = [17]
    many = r.sample("AB", 3, ctx, 1030, seed=3)
    logs = r.sample_log
    assert len(many) == 1030 == len(r.sample_costs) and [log[0].shape for log in logs] == [(3, 1024), (3, 6)]
    for s in range(3):
        want = gensample.philox_uniform(3, s, 1030)
        assert np.array_equal(logs[0][2][s], want[:1024]) and np.array_equal(logs[1][2][s], want[1024:])
        assert not np.array_equal(logs[1][2][s], want[:6])
    assert r.sample("AB", 3, ctx, 1024, seed=3) == many[:1024]          # a chain does not depend on how many there are
    assert r.sample("AB", 3, ctx, 3, seed=3) == many[:3]
    assert len(set(many)) > 100


@pytest.mark.parametrize("variants", [3, 1030])
def test_sample_device_bookkeeping_equals_the_host_loop(variants):
    ctx = [17]
    host = make_rater(lambda *a: OracleLM(*a, dtype=np.float32))
    want = host.sample("ABCD", 5, ctx, variants, temperature=0.8, top_k=20, floor=0.001, seed=11)
    r = make_rater(SampleOracle)
    pool = r._state_pool()
    pool.release_slots(pool.take_slots(2 * min(variants, 1024) + 3))      # (grown beforehand: the free list is then the same before and after)
    before = sorted(pool.free)
    got = r.sample("ABCD", 5, ctx, variants, temperature=0.8, top_k=20, floor=0.001, seed=11)
    assert got == want
    assert r.sample_costs == pytest.approx(host.sample_costs, rel=1e-5)          # (float32 sums against float64 ones)
    assert r.model.sample_generates == ([(3, 0)] if variants == 3 else [(1024, 0), (6, 1024)])
    assert sorted(pool.free) == before and pool.capacity >= 2 * min(variants, 1024)
    r.sample_keep_probs = True
    assert r.sample("ABCD", 5, ctx, variants, seed=11) and r.sample_log[0][3].shape == (5, min(variants, 1024), r.voc_size)
    r.sample_keep_probs = False
    # an engine failure in the middle: the slots come back
    r.model.fail_at = r.model.picks + 3
    with pytest.raises(RuntimeError, match="in the middle"):
        r.sample("ABCD", 5, ctx, variants, seed=11)
    assert sorted(pool.free) == before
    r.model.fail_at = None
    with pytest.raises(ValueError):
        r.sample("ABCD", 5, ctx, variants, top_k=65)
    assert sorted(pool.free) == before


# ---------------------------------------------------------------------- the command line
def test_cli_generate_sample(monkeypatch):
    from click.testing import CliRunner
    from ocrd_keraslm_amd.scripts import run
    res = CliRunner().invoke(run.cli, ["generate", "--help"])
    assert res.exit_code == 0 and all(opt in res.output for opt in ("--sample", "--temperature", "--top-k", "--seed"))
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model.h5")
        make_rater(OracleLM).save(model)
        monkeypatch.setattr(run.lib, "Rater", lambda: Rater(engine_factory=OracleLM))
        runner = CliRunner()
        outs = {}
        for name, extra in (("a", ["--seed", "4"]), ("again", ["--seed", "4"]), ("b", ["--seed", "5"]),
                            ("cold", ["--temperature", "0"]), ("k", ["--top-k", "1", "--temperature", "2.5"])):
            res = runner.invoke(run.cli, ["generate", "-m", model, "-n", "6", "-v", "3", "-c", "170", "--sample"] + extra + ["AB"])
            assert res.exit_code == 0, res.output + repr(res.exception)
            outs[name] = res.output.strip("\n").splitlines()
            assert len(outs[name]) == 3 and all(o.startswith("AB") and len(o) == 8 for o in outs[name])
        assert outs["a"] == outs["again"] != outs["b"]
        assert len(set(outs["cold"])) == 1 and outs["k"] == outs["cold"]
        beam = runner.invoke(run.cli, ["generate", "-m", model, "-n", "6", "-v", "3", "-c", "170", "AB"])      # without --sample: the beam
        assert beam.exit_code == 0 and len(beam.output.strip("\n").splitlines()) == 3
        for bad in (["--top-k", "65"], ["--temperature", "-1"], ["--seed", "-3"]):
            assert runner.invoke(run.cli, ["generate", "-m", model, "--sample"] + bad + ["AB"]).exit_code == 2
