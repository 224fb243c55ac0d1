"""Rating under candidate contexts on the GPU (run with -m gpu on an MI355X): kl_rate_scatter_planes and kl_context_mix against
their numpy statements in lib/ratebulk.py, their argument errors, and `Rater.rate_contexts` on the HIP engine.

Bounds of the mix (derived, not tuned).  The kernel and the statement take the same f64 logs but sum them in another order --
a shuffle scan per tile of 64 positions against a sequential sum, an online fold over the candidates against a two-pass one.
For a text of n_i predictions under C candidates
    delta_i = 1e-12 * max(1, max_c |cand_bits[i][c]|) + n_i * C * 2**-50,
the project's bound for another order of an f64 sum of logs plus the operation count of the weight chain: cand_bits and
mix_bits within delta_i, the posterior within 4 delta_i (its exponent moves by at most 2 delta_i, its normalisation as much
again), the margin -- a difference of two such sums -- within 2 delta_i, the mixture's f32 probabilities within two ulps.  `best`
must be equal: the test first asserts, from the statement alone, that every margin exceeds 2 delta_i or is an exact tie (which
both sides break towards the smaller index), so a seed that does not decide fails loudly."""
import ctypes as C

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk, windows
from tests.test_rate_window_gpu import ptr

pytestmark = pytest.mark.gpu

KL_ERR_ARG = 5
SPLIT_BOUND = 2e-5      # the project's split-precision bound on a probability (test_rate_window_against_the_oracle)
MARK32 = np.uint32(0x7fc0beef)
MARK64 = np.uint64(0x7ff8beefbeefbeef)
GUARD = 64


def device():
    import torch
    return torch, torch.device("cuda:0")


def lib_and_stream():
    from ocrd_keraslm_amd.lib import hipabi
    torch, dev = device()
    return hipabi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---------------------------------------------------------------------------------------------- kl_rate_scatter_planes
@pytest.mark.parametrize("n_ctx", [0, 2])
@pytest.mark.parametrize("B,T", [(5, 7), (70, 33)])
def test_scatter_planes_is_scatter_planes_host(B, T, n_ctx):
    """bit for bit, any bit pattern (NaNs included); planes -1 and C among the rows; vlen 0, 1, T and T + 3 (clipped to T);
    ld > n_out; the last row ends beyond n_out; a guard band behind every plane and behind the array keeps its marker"""
    torch, dev = device()
    lib, stream = lib_and_stream()
    n_planes = 3
    rng = np.random.default_rng(B * 10 + n_ctx)
    tprob = rng.integers(0, 2 ** 32, (B, T), dtype=np.uint64).astype(np.uint32)
    rows = np.zeros((B, 4 + n_ctx), dtype=np.int64)
    rows[:, 0] = (np.arange(B) // n_planes) * (T + 2) + 3          # (the rows of a text's candidates share their positions)
    rows[:, 1] = np.array([0, 1, T, T + 3])[np.arange(B) % 4]
    rows[-1, 1] = T
    rows[:, 2:] = rng.integers(-1, 200, (B, 2 + n_ctx))      # (not read here)
    plane = (np.arange(B) % n_planes).astype(np.int32)
    plane[1], plane[2] = -1, n_planes                        # (vlen 1 and T: rows that would write)
    plane[-1] = (B - 1) % n_planes
    n_out = int(rows[-1, 0]) + 1 + T // 2                    # the last row's second half lies beyond the end
    ld = n_out + GUARD
    want = np.full((n_planes, ld), MARK32, dtype=np.uint32)
    ratebulk.scatter_planes_host(tprob, rows, plane, want, n_out)
    assert (want[plane[-1], int(rows[-1, 0]) + 1:n_out] != MARK32).all() and (want[:, n_out:] == MARK32).all()
    written = [(want[c] != MARK32).any() for c in range(n_planes)]
    assert sum(written) >= 2 and (B < 3 * n_planes or all(written))      # (five rows do not reach every plane)
    out_d = torch.from_numpy(np.full(n_planes * ld + GUARD, MARK32, dtype=np.uint32).view(np.float32)).to(dev)
    tprob_d, rows_d, plane_d = (torch.from_numpy(a).to(dev) for a in (tprob.view(np.float32), rows, plane))
    assert lib.kl_rate_scatter_planes(ptr(tprob_d), ptr(rows_d), ptr(plane_d), B, T, n_ctx, n_planes, ptr(out_d), ld, n_out,
                                      stream) == 0
    torch.cuda.synchronize()
    got = out_d.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n_planes * ld].reshape(n_planes, ld), want)
    assert (got[n_planes * ld:] == MARK32).all()


# ---------------------------------------------------------------------------------------------- kl_context_mix
SIZES = [0, 1, 2, 65, 1000, 0, 2, 130]


def mix_inputs(n_cand, with_prior):
    """planes [C, ld] with ld > n: rng**4 probabilities with a tilt per candidate, one 0.0 and one NaN, one plane duplicated;
    offsets; log2prior (None, or distinct weights with one -inf entry)"""
    rng = np.random.default_rng(100 + n_cand)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(offsets[-1])
    ld = n + 37
    planes = (rng.random((n_cand, ld)) ** 4 * np.linspace(0.6, 1.0, n_cand)[:, None]).astype(np.float32)
    planes[0, offsets[4] + 77] = 0.0
    planes[n_cand // 2, offsets[4] + 500] = np.nan
    if n_cand > 1:
        planes[n_cand - 1] = planes[n_cand // 3]
    prior = None
    if with_prior:
        weights = rng.random(n_cand) + 0.25
        if n_cand > 1:
            weights[n_cand // 3] = 0.0
        with np.errstate(divide="ignore"):
            prior = np.log2(weights / weights.sum())
    return planes, offsets, prior


def deltas(cand_bits, n_cand):
    preds = np.maximum(np.asarray(SIZES) - 1, 0)
    return 1e-12 * np.maximum(1.0, np.abs(cand_bits).max(axis=1)) + preds * n_cand * 2.0 ** -50


def run_mix(lib, stream, planes, offsets, prior, want_mix):
    """one kl_context_mix call into marked outputs with a guard band behind each: the raw arrays"""
    torch, dev = device()
    n_cand, ld = planes.shape
    n = len(offsets) - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    planes_d, off_d, prior_d = up(planes), up(offsets), (None if prior is None else up(prior))
    marked64 = lambda m: up(np.full(m + GUARD, MARK64, dtype=np.uint64).view(np.float64))
    mix_d = up(np.full(ld + GUARD, MARK32, dtype=np.uint32).view(np.float32)) if want_mix else None
    cand_d, bits_d, post_d, margin_d = marked64(n * n_cand), marked64(n), marked64(n * n_cand), marked64(n)
    best_d = up(np.full(n + GUARD, MARK32, dtype=np.uint32).view(np.int32))
    assert lib.kl_context_mix(ptr(planes_d), ld, ptr(off_d), n, n_cand, ptr(prior_d), ptr(mix_d), ptr(cand_d), ptr(bits_d),
                              ptr(post_d), ptr(best_d), ptr(margin_d), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(planes_d.cpu().numpy().view(np.uint32), planes.view(np.uint32))      # (the input is left alone)
    return [None if t is None else t.cpu().numpy() for t in (mix_d, cand_d, bits_d, post_d, best_d, margin_d)]


@pytest.mark.parametrize("with_prior", [False, True], ids=["uniform", "prior"])
@pytest.mark.parametrize("n_cand", [1, 2, 63, 64, 65, 200, 256])
def test_context_mix_is_context_mix_host(n_cand, with_prior):
    lib, stream = lib_and_stream()
    planes, offsets, prior = mix_inputs(n_cand, with_prior)
    n_texts, n, ld = len(SIZES), int(offsets[-1]), planes.shape[1]
    want_mix = np.full(ld, MARK32, dtype=np.uint32).view(np.float32)
    cand_bits, mix_bits, post, best, margin = ratebulk.context_mix_host(planes, offsets, prior, want_mix)
    delta = deltas(cand_bits, n_cand)
    # from the statement alone: every decision is clear, or an exact tie
    assert ((margin > 2 * delta) | (margin == 0.0)).all(), (margin, delta)
    assert cand_bits[4].max() > 328.0      # (the zero, or the NaN, at the floor)
    runs = [run_mix(lib, stream, planes, offsets, prior, True) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))      # two runs agree bit for bit
    got_mix, got_cand, got_bits, got_post, got_best, got_margin = runs[0]
    # guard bands, and everything of mix that is no predicted position
    assert (got_mix[ld:].view(np.uint32) == MARK32).all() and (got_best[n_texts:].view(np.uint32) == MARK32).all()
    for a, m in ((got_cand, n_texts * n_cand), (got_bits, n_texts), (got_post, n_texts * n_cand), (got_margin, n_texts)):
        assert (a[m:].view(np.uint64) == MARK64).all()
    untouched = want_mix.view(np.uint32) == MARK32
    assert untouched[offsets[:-1][np.asarray(SIZES) > 0]].all() and untouched[n:].all() and untouched.sum() == ld - n + 6
    assert (got_mix[:ld].view(np.uint32)[untouched] == MARK32).all()
    got_cand, got_post = got_cand[:n_texts * n_cand].reshape(n_texts, n_cand), got_post[:n_texts * n_cand].reshape(n_texts, n_cand)
    got_bits, got_best, got_margin = got_bits[:n_texts], got_best[:n_texts], got_margin[:n_texts]
    print("C = %d: max |cand_bits - host| / delta = %.3g, mix_bits %.3g, post / 4 delta %.3g"
          % (n_cand, (np.abs(got_cand - cand_bits) / delta[:, None]).max(), (np.abs(got_bits - mix_bits) / delta).max(),
             (np.abs(got_post - post) / (4 * delta[:, None])).max()))
    assert (np.abs(got_cand - cand_bits) <= delta[:, None]).all()
    assert (np.abs(got_bits - mix_bits) <= delta).all()
    assert (np.abs(got_post - post) <= 4 * delta[:, None]).all()
    assert np.array_equal(got_best, best)
    finite = np.isfinite(margin)
    assert np.array_equal(np.isposinf(got_margin), ~finite) and (np.abs(got_margin[finite] - margin[finite]) <= 2 * delta[finite]).all()
    live = ~untouched
    np.testing.assert_allclose(got_mix[:ld][live], want_mix[live], rtol=2.0 ** -22, atol=0)
    if n_cand == 1:
        # the plane itself, bit for bit -- but 0 for the NaN
        hole = np.isnan(planes[0])
        assert hole.sum() == 1 and (got_mix[:ld][live & hole] == 0.0).all() and got_mix[offsets[4] + 77] == 0.0
        assert np.array_equal(got_mix[:ld][live & ~hole].view(np.uint32), planes[0][live & ~hole].view(np.uint32))
    # the mixture telescopes: mix_bits = -log2 sum_c pi_c 2**-bits_c, on the device's own outputs, as a log-sum-exp
    lp = (np.zeros(n_cand) if prior is None else prior)[None, :] - got_cand
    lp = lp - (np.log2(n_cand) if prior is None else 0.0)
    top = lp.max(axis=1, keepdims=True)
    lse = top[:, 0] + np.log2(np.exp2(lp - top).sum(axis=1))
    assert (np.abs(got_bits + lse) <= 2 * delta).all(), np.abs(got_bits + lse) / delta
    # without mix: the same six other outputs
    bare = run_mix(lib, stream, planes, offsets, prior, False)
    assert bare[0] is None and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(bare[1:], runs[0][1:]))


def test_context_mix_without_a_finite_prior_stays_inside_its_outputs():
    """the caller's promise broken: what the header says is delivered, and nothing outside the outputs is touched"""
    lib, stream = lib_and_stream()
    planes, offsets, _ = mix_inputs(3, False)
    prior = np.full(3, -np.inf)
    n_texts, ld = len(SIZES), planes.shape[1]
    want = ratebulk.context_mix_host(planes, offsets, prior)
    mix, cand, bits, post, best, margin = run_mix(lib, stream, planes, offsets, prior, True)
    assert (mix[ld:].view(np.uint32) == MARK32).all() and (best[n_texts:].view(np.uint32) == MARK32).all()
    for a, m in ((cand, n_texts * 3), (bits, n_texts), (post, n_texts * 3), (margin, n_texts)):
        assert (a[m:].view(np.uint64) == MARK64).all()
    assert (best[:n_texts] == 0).all() and np.isposinf(margin[:n_texts]).all() and np.isnan(post[:n_texts * 3]).all()
    predicted = np.asarray(SIZES) > 1
    assert np.isnan(bits[:n_texts][predicted]).all() and (bits[:n_texts][~predicted] == 0.0).all()
    assert np.array_equal(np.isnan(bits[:n_texts]), np.isnan(want[1]))
    np.testing.assert_allclose(cand[:n_texts * 3].reshape(n_texts, 3), want[0], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_write_nothing():
    torch, dev = device()
    lib, stream = lib_and_stream()
    marked = lambda m, dt: torch.from_numpy(np.full(m, 0x55, dtype=np.uint8).view(dt)).to(dev)
    f, out = torch.zeros(64, dtype=torch.float32, device=dev), marked(4 * 3 * 64, np.float32)
    rows = torch.zeros((2, 5), dtype=torch.int64, device=dev)
    rows[:, 1] = 4
    plane = torch.zeros(64, dtype=torch.int32, device=dev)
    sp = lambda **k: lib.kl_rate_scatter_planes(k.get("tprob", ptr(f)), k.get("plan", ptr(rows)), k.get("plane", ptr(plane)),
                                                k.get("B", 2), k.get("T", 4), k.get("n_ctx", 1), k.get("C", 3),
                                                k.get("out", ptr(out)), k.get("ld", 64), k.get("n_out", 60), stream)
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    for bad in (dict(tprob=None), dict(plan=None), dict(plane=None), dict(out=None), dict(B=0), dict(T=0), dict(C=0), dict(C=257),
                dict(n_ctx=-1), dict(n_ctx=9), dict(ld=59), dict(tprob=off(f, 2)), dict(plan=off(rows, 4)), dict(plane=off(plane, 2)),
                dict(out=off(out, 1))):
        assert sp(**bad) == KL_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint8) == 0x55).all()
    assert sp() == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint8) != 0x55).any()
    offsets = torch.tensor([0, 3, 8], dtype=torch.int64, device=dev)
    prior = torch.zeros(4, dtype=torch.float64, device=dev)
    outs = dict(mix=marked(4 * 64, np.float32), cand_bits=marked(8 * 8, np.float64), mix_bits=marked(8 * 8, np.float64),
                post=marked(8 * 8, np.float64), best=marked(4 * 8, np.int32), margin=marked(8 * 8, np.float64))
    planes = torch.full((3, 64), 0.5, dtype=torch.float32, device=dev)
    cm = lambda **k: lib.kl_context_mix(k.get("planes", ptr(planes)), k.get("ld", 64), k.get("offsets", ptr(offsets)), k.get("n", 2),
                                        k.get("C", 3), k.get("prior", ptr(prior)), k.get("mix", ptr(outs["mix"])),
                                        k.get("cand_bits", ptr(outs["cand_bits"])), k.get("mix_bits", ptr(outs["mix_bits"])),
                                        k.get("post", ptr(outs["post"])), k.get("best", ptr(outs["best"])),
                                        k.get("margin", ptr(outs["margin"])), stream)
    for bad in (dict(planes=None), dict(offsets=None), dict(cand_bits=None), dict(mix_bits=None), dict(post=None), dict(best=None),
                dict(margin=None), dict(n=0), dict(C=0), dict(C=257), dict(ld=0), dict(planes=off(planes, 2)),
                dict(offsets=off(offsets, 4)), dict(prior=off(prior, 4)), dict(mix=off(outs["mix"], 2)),
                dict(cand_bits=off(outs["cand_bits"], 4)), dict(mix_bits=off(outs["mix_bits"], 4)), dict(post=off(outs["post"], 4)),
                dict(best=off(outs["best"], 2)), dict(margin=off(outs["margin"], 4))):
        assert cm(**bad) == KL_ERR_ARG, bad
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) == 0x55).all() for t in outs.values())
    assert cm() == 0 and cm(mix=None, prior=None) == 0      # (the two optional pointers)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) != 0x55).any() for t in outs.values())


# ---------------------------------------------------------------------------------------------- Rater.rate_contexts
CANDIDATES = [[171], [185], [0]]
STREAMS = 4


def raters():
    from tests.test_rate_bulk_gpu import small_rater
    from tests.test_rate_corrections import wide_rater
    from tests.test_rate_suspects import LENGTH
    return {"small": lambda factory: small_rater(factory, length=LENGTH), "wide": lambda factory: wide_rater(factory, length=LENGTH)}


@pytest.mark.parametrize("which", ["small", "wide"])
def test_one_candidate_is_rate_batch_bf16(which):
    """the same plan and the same launches: probabilities bit for bit, bits within 1e-12"""
    from tests.test_rate_suspects import contract_texts
    from tests.test_rater_golden import hip_factory
    texts, _ = contract_texts()
    r = raters()[which](hip_factory)
    probs, bits = r.rate_batch(texts, [185], streams=STREAMS, precision="bf16")
    found = r.rate_contexts(texts, [[185]], streams=STREAMS, precision="bf16")
    for one, p, b in zip(found, probs, bits):
        assert one.probs.dtype == np.float32 and np.array_equal(one.probs.view(np.uint32), p.view(np.uint32))
        assert abs(one.bits[0] - b) <= 1e-12 * max(1.0, b) and abs(one.mix_bits - b) <= 1e-12 * max(1.0, b)
        assert one.best == 0 and one.margin == np.inf and one.posterior.tolist() == [1.0]
    bare = r.rate_contexts(texts, [[185]], streams=STREAMS, precision="bf16", want_probs=False)
    assert all(x.probs is None and np.array_equal(x.bits, y.bits) for x, y in zip(bare, found))


@pytest.mark.parametrize("which", ["small", "wide"])
def test_three_candidates_are_the_replayed_plan_mixed_by_the_statement(which):
    """the test replays the plan's calls itself -- assemble_windows and rate_window_bulk at the same (B, T) -- and applies the
    two numpy statements; the Rater's result is held to that by the bounds of the mix"""
    from tests.test_rate_suspects import contract_texts
    from tests.test_rater_golden import hip_factory
    texts, _ = contract_texts()
    r = raters()[which](hip_factory)
    found = r.rate_contexts(texts, CANDIDATES, streams=STREAMS, precision="bf16")
    lm = r.model
    torch = lm.torch
    ids = [windows.encode(windows.normalize(t), r.mapping[0]) for t in texts]
    plan, plane = ratebulk.plan_candidates([len(a) for a in ids], CANDIDATES, r.length, STREAMS)
    corpus = torch.from_numpy(np.concatenate(ids).astype(np.int32)).to(lm.device)
    planes = np.ones((len(CANDIDATES), plan.total), dtype=np.float32)
    B = None
    for call, where in zip(plan.calls, plane):
        if call.B != B:
            B = call.B
            lm.reset_states(B)
        elif call.reset.any():
            lm.reset_states_where(torch.from_numpy(call.reset).to(lm.device))
        rows = torch.from_numpy(call.rows).to(lm.device)
        x, z, y = lm.assemble_windows(corpus, rows, call.T, plan.n_ctx)
        ratebulk.scatter_planes_host(lm.rate_window_bulk(x, z, y).cpu().numpy(), call.rows, where, planes)
    lm.rate_bits_read(reset=True)
    lm.reset_states(1)
    mix = np.ones(plan.total, dtype=np.float32)
    cand_bits, mix_bits, post, best, margin = ratebulk.context_mix_host(planes, plan.offsets, None, mix)
    preds = np.maximum(plan.sizes - 1, 0)
    delta = 1e-12 * np.maximum(1.0, np.abs(cand_bits).max(axis=1)) + preds * len(CANDIDATES) * 2.0 ** -50
    assert ((margin > 2 * delta) | (margin == 0.0)).all(), (margin, delta)
    assert len(set(best[preds > 0].tolist())) > 1      # (the texts do not all read like one candidate)
    for i, one in enumerate(found):
        a, b = int(plan.offsets[i]), int(plan.offsets[i + 1])
        assert (np.abs(one.bits - cand_bits[i]) <= delta[i]).all() and abs(one.mix_bits - mix_bits[i]) <= delta[i]
        assert (np.abs(one.posterior - post[i]) <= 4 * delta[i]).all()
        assert one.best == best[i] and abs(one.margin - margin[i]) <= 2 * delta[i]
        assert one.probs.shape == (b - a,) and (b == a or one.probs[0] == 1.0)
        np.testing.assert_allclose(one.probs, mix[a:b], rtol=2.0 ** -22, atol=0)


@pytest.mark.parametrize("which", ["small", "wide"])
def test_split_precision_against_the_oracle_rater(which):
    """bits within the first-order bound sum_j SPLIT_BOUND / (p_j ln 2) computed from the double's probabilities; `best` equal
    wherever the double's margin exceeds twice that bound -- which, on the double alone, covers every text with a prediction"""
    from tests.oracle_engine import OracleLM
    from tests.test_rate_suspects import LENGTH, contract_texts
    from tests.test_rater_golden import hip_factory
    texts, _ = contract_texts()
    oracle = raters()[which](OracleLM)
    want = oracle.rate_contexts(texts, CANDIDATES, streams=STREAMS, precision="split")
    per = [oracle.rate_batch(texts, c, streams=STREAMS)[0] for c in CANDIDATES]
    bound = np.array([[(SPLIT_BOUND / (np.maximum(p[i][1:].astype(np.float64), 1e-99) * np.log(2.0))).sum() for p in per]
                      for i in range(len(texts))])
    decided = np.array([one.margin > 2 * bound[i].max() for i, one in enumerate(want)])
    assert decided[[len(t) > 1 for t in texts]].all() and sum(len(t) > LENGTH + 1 for t in texts) >= 3
    hip = raters()[which](hip_factory)
    got = hip.rate_contexts(texts, CANDIDATES, streams=STREAMS, precision="split")
    for i, (g, w) in enumerate(zip(got, want)):
        assert (np.abs(g.bits - w.bits) <= bound[i]).all(), (i, g.bits - w.bits, bound[i])
        if decided[i]:
            assert g.best == w.best
        assert g.probs.dtype == np.float32 and g.probs.shape == w.probs.shape
    # afterwards: a freshly reset single row, split precision
    assert hip.model.states.shape[0] == 1
