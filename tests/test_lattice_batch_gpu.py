"""Lattices decoded in lockstep on the GPU (-m gpu): kl_edge_costs against numpy f64, kl_edge_decode against the statement
`lattice_batch.edge_decode_host` bit for bit (fed the device's own cost array), and `Rater.rate_best_batch` on the HIP engine
against `rate_best(edge_walk=True)` on the HIP engine.

Every device wait is EdgeRound's / walk_host's (20 s), nothing is retried."""
import numpy as np
import pytest

from ocrd_keraslm_amd.lib import lattice_batch
from tests.edge_walk_cases import random_segments, run_pages, summary
from tests.oracle_engine import OracleLM
from tests.test_rater_golden import SEAM, hip_factory, lattice, make_rater

pytestmark = pytest.mark.gpu

KL_ERR_WORKSPACE, KL_ERR_ARG = 4, 5


def _model(depth, width, voc=40):
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_gpu_kernels import make_model
    cfg, w, lm = make_model(depth, width, voc, 1)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    return lm


def _one_edge_arrays(n_pairs):
    """the smallest EdgeBatch that owns n_pairs pairs: one hypothesis, one alternative... of at most 1024 characters each"""
    eb = lattice_batch.EdgeBatch()
    left = n_pairs
    while left:
        k = min(left, 1024)
        eb.add_edge([0.0], [0], [k], [0.25], [0], [0], [], [], [], 3 * k)
        left -= k
    return eb.arrays()


def test_edge_costs_against_numpy_f64():
    """kl_edge_costs on 4096 probabilities against -(np.log(max(p, 1e-99)) / np.log(2.0)) * w + conf in numpy f64.

    The bound.  With u = 2^-53 (half an ulp, relative): ROCm documents its f64 `log` as accurate to 1 ulp, i.e. a relative
    error of at most 2u on l = log(p); numpy's log is glibc's, within 1 ulp as well (2u).  The quotient by the same constant,
    the product with lm_weight and the sum with conf are single IEEE operations, each within u of the exact result of its
    (already perturbed) inputs, on BOTH sides.  So the two results differ by at most
        |bits * w| * ((2u + 2u) + (u + u) + (u + u)) + |result| * (u + u)  <=  (8 |bits * w| + 2 |result|) * u,
    and as conf >= 0 here, |bits * w| <= |result|: at most 10 u |result| = 5 ulp of the result.  The test asserts 5 ulp and
    prints the largest deviation seen."""
    lm = _model(1, 64)
    rng = np.random.default_rng(3)
    n = 4096
    probs = rng.uniform(0, 1, n).astype(np.float32)
    probs[:8] = [0.0, 1.0, np.float32(1.401298464324817e-45), np.float32(1e-30), 0.5, np.nextafter(np.float32(1), np.float32(0)),
                 np.float32(1e-38), np.float32(3e-39)]
    probs[8:1024] = (10.0 ** rng.uniform(-44, 0, 1016)).astype(np.float32)
    arrays = _one_edge_arrays(n)
    arrays["alt_conf"] = rng.uniform(0.0, 3.0, len(arrays["alt_conf"]))
    w = 0.37
    rnd = lm.edge_round(arrays, w, 128, 10)
    rnd.costs_from(probs)
    got = rnd.finish(want_costs=True)["step_cost"]
    p = probs.astype(np.float64)
    bits = -(np.log(np.where(p > 1e-99, p, 1e-99)) / np.log(2.0))
    want = bits * w + arrays["alt_conf"][arrays["pair_alt"]]
    assert np.all(np.isfinite(got))
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    print("kl_edge_costs: largest deviation from numpy f64 %.2f ulp over %d probabilities" % (ulp.max(), n))
    assert ulp.max() <= 5.0, ulp.max()
    clamp = -(np.log(1e-99) / np.log(2.0)) * w + arrays["alt_conf"][arrays["pair_alt"][0]]
    assert abs(got[0] - clamp) <= 5 * np.spacing(clamp) and got[0] > 100       # p = 0: the clamp's cost
    assert got[1] == arrays["alt_conf"][arrays["pair_alt"][1]]                  # p = 1: log 0, the confidence term alone
    rnd2 = lm.edge_round(arrays, w, 128, 10)                                    # two calls: bit-identical
    rnd2.costs_from(probs)
    assert np.array_equal(rnd2.finish(want_costs=True)["step_cost"], got)


# ---------------------------------------------------------------------------------------------------------------- the decode
def _random_batch(rng, n_edges, max_in=10, max_alt=6, max_len=8, pre=True, shapes=None):
    """E ragged edges with random slots; shapes: [(n_in, [alt lengths])] overrides the random shapes"""
    eb = lattice_batch.EdgeBatch()
    slot = 1
    for e in range(n_edges):
        if shapes is not None:
            n_in, lens = shapes[e]
        else:
            n_in = int(rng.integers(1, max_in + 1))
            lens = [int(k) for k in rng.integers(1, max_len + 1, int(rng.integers(1, max_alt + 1)))]
            if e % 7 == 3:
                lens[-1] = 0                                  # an empty alternative
        n_alt = len(lens)
        classes = list(range(n_alt))
        if n_alt >= 3:
            classes[2] = classes[0]                            # equal texts share a class
        n_pre = int(rng.integers(0, 4)) if pre and e % 3 == 0 else 0
        cum = np.sort(rng.uniform(0, 6, n_in)).tolist()
        n = n_in * n_alt
        slots = list(range(slot, slot + n_in + n + n_pre))
        slot += len(slots)
        pre_cost = np.sort(rng.uniform(3, 30, n_pre)).tolist()
        eb.add_edge(cum, slots[:n_in], lens, rng.uniform(0.0, 2.0, n_alt).tolist(), classes, slots[n_in:n_in + n],
                    pre_cost, [int(rng.integers(-1, n_alt)) for _ in range(n_pre)], slots[n_in + n:], 3 * max(max(lens), 1))
    return eb.arrays(), slot


def _compare(lm, arrays, probs, batch_size, beam_width, depth_k=0, dist=0.0, close=None, expect_status=None):
    rnd = lm.edge_round(arrays, 0.5, batch_size, beam_width, depth_k, dist)
    rnd.costs_from(probs)
    got = rnd.finish(want_costs=True)
    count, status, ref, cost, consumed, when = lattice_batch.decode_batch_host(arrays, got["step_cost"], batch_size, beam_width, close)
    desc = arrays["desc"]
    for e in range(len(desc)):
        if expect_status and e in expect_status:
            assert got["status"][e] == 1 and got["count"][e] == 0
            continue
        assert got["status"][e] == 0
        assert got["count"][e] == count[e], e
        k = int(count[e])
        assert np.array_equal(got["ref"][e, :k], ref[e, :k]), e
        assert np.array_equal(got["cost"][e, :k].view(np.int64), cost[e, :k].view(np.int64)), e      # bit for bit
        t0, n = int(desc[e][5]), int(desc[e][0]) * int(desc[e][1])
        assert np.array_equal(got["consumed"][t0:t0 + n], consumed[t0:t0 + n]), e
        for t in range(t0, t0 + n):
            s0 = int(arrays["step_off"][t])
            assert np.array_equal(got["when"][s0:s0 + consumed[t]], when[s0:s0 + consumed[t]]), (e, t)
    return got


@pytest.mark.parametrize("batch_size", [1, 128])
def test_edge_decode_equals_the_statement(batch_size):
    lm = _model(1, 64)
    rng = np.random.default_rng(11 + batch_size)
    # ---- one edge with one track
    arrays, _ = _random_batch(rng, 1, shapes=[(1, [3])], pre=False)
    got = _compare(lm, arrays, rng.uniform(0.05, 1, 3), batch_size, 10)
    assert got["count"][0] == 1 and got["ref"][0, 0] == 0 and got["consumed"][0] == 3
    # ---- 300 ragged edges in one launch (more workgroups than CUs), pre-existing entries, empty alternatives, peaked costs
    arrays, _ = _random_batch(rng, 300)
    probs = rng.uniform(0.001, 1, len(arrays["pair_alt"])) ** 3
    got = _compare(lm, arrays, probs, batch_size, 10)
    assert (got["ref"] < 0).any() and (got["count"] == 10).any() and (got["count"] < 10).any()
    _compare(lm, arrays, probs, batch_size, 3)
    # two launches on the same inputs: bit-identical
    again = _compare(lm, arrays, probs, batch_size, 10)
    for name in ("count", "ref", "cost", "consumed"):
        assert np.array_equal(again[name], got[name])


def test_edge_decode_at_and_above_its_capacity():
    """an edge of exactly 1024 tracks between two small ones; then one of 1025: status set, its neighbours unaffected"""
    lm = _model(1, 64)
    rng = np.random.default_rng(21)
    shapes = [(3, [2, 4]), (128, [1, 2, 1, 3, 2, 1, 2, 1]), (2, [5])]
    arrays, _ = _random_batch(rng, 3, shapes=shapes, pre=False)
    assert int(arrays["desc"][1][0]) * int(arrays["desc"][1][1]) == 1024
    probs = rng.uniform(0.05, 1, len(arrays["pair_alt"]))
    got = _compare(lm, arrays, probs, 128, 10)
    assert got["count"][1] == 10
    _compare(lm, arrays, probs, 1024, 10)                    # the whole edge as one batch
    shapes[1] = (205, [1, 2, 1, 3, 2])                       # 1025 tracks
    arrays, _ = _random_batch(rng, 3, shapes=shapes, pre=False)
    probs = rng.uniform(0.05, 1, len(arrays["pair_alt"]))
    rnd = lm.edge_round(arrays, 0.5, 128, 10)
    rnd.costs_from(probs)
    rnd.out.fill_(0x5a)
    got = rnd.finish(want_costs=True)
    t0 = int(arrays["desc"][1][5])
    assert got["status"].tolist() == [0, 1, 0] and got["count"][1] == 0
    assert np.all(got["consumed"][t0:t0 + 1025] == 0x5a5a5a5a) and np.all(got["ref"][1] == 0x5a5a5a5a)      # nothing written for it
    _compare(lm, arrays, probs, 128, 10, expect_status={1})


@pytest.mark.parametrize("depth,width", [(1, 64), (3, 64), (1, 512), (3, 512)])
def test_edge_decode_clustering_with_planted_twins(depth, width):
    """history clustering: the kernel reads the pool, the statement's predicate is answered from kl_state_dist2.  States are
    multiples of a unit pattern, so every squared distance is either 0 (twins) or at least 4 x the threshold: none lies within a
    relative 1e-6 of it."""
    lm = _model(depth, width)
    rng = np.random.default_rng(31 + depth + width)
    arrays, n_slots = _random_batch(rng, 40, max_in=6, max_alt=5)
    dist = 5.0
    lm.ensure_pool(n_slots + 1)
    # slot s holds level[s] * 10 / sqrt(W) in every unit: the distance between levels a and b is 10 |a - b| (0 or >= 2 x dist)
    level = rng.integers(0, 6, n_slots + 1)
    desc = arrays["desc"]
    for e in range(len(desc)):      # planted twins: alternative 2 (same class as 0) ends where alternative 0 ends
        n_in, n_alt, trk_off = int(desc[e][0]), int(desc[e][1]), int(desc[e][5])
        if n_alt >= 3 and e % 2 == 0:
            for p in range(n_in):
                level[arrays["final_slot"][trk_off + p * n_alt + 2]] = level[arrays["final_slot"][trk_off + p * n_alt]]
    states = np.repeat((level * 10.0 / np.sqrt(width))[:, None, None], 2 * depth, axis=1).repeat(width, axis=2).astype(np.float32)
    lm.pool_write(np.arange(n_slots + 1), states)
    answers = {}

    def close(a, b):
        key = (a, b)
        if key not in answers:
            d2 = [float(lm.state_dist2([a], [b], k).cpu().numpy()[0]) for k in range(depth)]
            assert all(abs(v - dist * dist) > 1e-6 * dist * dist for v in d2)
            answers[key] = all(v < dist * dist for v in d2)
        return answers[key]

    probs = rng.uniform(0.2, 1, len(arrays["pair_alt"]))
    _compare(lm, arrays, probs, 128, 10, depth, dist, close)
    assert any(answers.values()) and not all(answers.values())
    without = lm.edge_round(arrays, 0.5, 128, 10)
    without.costs_from(probs)
    plain = without.finish()
    with_ = lm.edge_round(arrays, 0.5, 128, 10, depth, dist)
    with_.costs_from(probs)
    assert not np.array_equal(plain["ref"], with_.finish()["ref"])      # the twins did go


def test_edge_decode_argument_errors_return_their_codes_without_launching():
    lm = _model(1, 64)
    rng = np.random.default_rng(41)
    arrays, _ = _random_batch(rng, 5, pre=False)
    rnd = lm.edge_round(arrays, 0.5, 128, 10)
    rnd.costs_from(rng.uniform(0.05, 1, len(arrays["pair_alt"])))
    rnd.out.fill_(0x5a)
    lib = lm.lib
    good = rnd.decode_args()
    # positions in kl_edge_decode's argument list
    N_EDGES, DESC, COST, POOL, DEPTH_K, BATCH, BEAM, CAP, OUT, OUT_BYTES = 1, 2, 11, 12, 13, 15, 16, 17, 20, 21

    def call(**changes):
        args = list(good)
        for k, v in changes.items():
            args[{"n_edges": N_EDGES, "desc": DESC, "cost": COST, "pool": POOL, "depth_k": DEPTH_K, "batch": BATCH, "beam": BEAM,
                  "cap": CAP, "out": OUT, "out_bytes": OUT_BYTES, "handle": 0}[k]] = v
        return lib.kl_edge_decode(*args)

    assert call(handle=None) == KL_ERR_ARG
    assert call(n_edges=0) == KL_ERR_ARG
    assert call(desc=None) == KL_ERR_ARG
    assert call(cost=None) == KL_ERR_ARG
    assert call(out=None) == KL_ERR_ARG
    assert call(out=good[OUT] + 4) == KL_ERR_ARG
    assert call(batch=0) == KL_ERR_ARG
    assert call(beam=0) == KL_ERR_ARG
    assert call(cap=0) == KL_ERR_ARG and call(cap=1025) == KL_ERR_ARG
    assert call(depth_k=1, pool=None) == KL_ERR_ARG
    assert call(depth_k=3) == KL_ERR_ARG
    assert call(out_bytes=good[OUT_BYTES] - 8) == KL_ERR_WORKSPACE
    stream = good[-1]
    assert lib.kl_edge_costs(0, rnd.keep[0].data_ptr(), rnd._in("pair_alt"), rnd._in("alt_conf"), 0.5, rnd.cost.data_ptr(), stream) == KL_ERR_ARG
    assert lib.kl_edge_costs(4, None, rnd._in("pair_alt"), rnd._in("alt_conf"), 0.5, rnd.cost.data_ptr(), stream) == KL_ERR_ARG
    assert lib.kl_edge_costs(4, rnd.keep[0].data_ptr(), rnd._in("pair_alt"), rnd._in("alt_conf"), float("nan"), rnd.cost.data_ptr(), stream) == KL_ERR_ARG
    assert lib.kl_edge_decode_out_bytes(0, 10, 5, 5) == 0
    lm.torch.cuda.synchronize()
    assert bool((rnd.out == 0x5a).all())                     # nothing was launched
    assert call() == 0


# ---------------------------------------------------------------------------------------------------------------- the rater
GPU_SEEDS = list(range(200, 220))      # as tests/test_edge_walk_gpu.py, and its rule
MARGIN = 0.05


@pytest.mark.parametrize("beam_width,dist", [(10, 0), (3, 5)])
def test_rate_best_batch_on_the_hip_engine_against_the_single_call(beam_width, dist):
    """The step kernels route by row count, so the batch's and the single call's probabilities may differ in the last bits: a
    seed is compared only if, on the f64 CPU double, the best final hypothesis leads the second by more than 0.05 bits; at
    least 8 of every 10 seeds must be kept."""
    cpu = make_rater(OracleLM, False, True)
    kept, lattices = [], []
    for seed in GPU_SEEDS:
        segs = random_segments(seed, empty=False)
        costs = run_pages(cpu, [segs], beam_width=beam_width, dist=dist, edge_walk=False)[0]["costs"]
        if (costs[1] - costs[0] if len(costs) > 1 else float("inf")) > MARGIN:
            kept.append(seed)
            lattices.append(segs)
    for d0 in range(0, len(GPU_SEEDS), 10):
        assert sum(s in kept for s in GPU_SEEDS[d0:d0 + 10]) >= 8, kept
    single = make_rater(hip_factory, False, True)
    batch = make_rater(hip_factory, False, True)
    built = [lattice(segs) for segs in lattices]
    results = batch.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built], contexts=[17],
                                    beam_width=beam_width, beam_clustering_dist=dist)
    for seed, segs, (path, entropy, tb) in zip(kept, lattices, results):
        path, entropy, tb = batch.next_path(tb[0], ([], tb[1]))
        got = summary(path, entropy, tb)
        want = run_pages(single, [segs], beam_width=beam_width, dist=dist, edge_walk=True)[-1]
        assert got["path"] == want["path"], seed
        assert len(got["path"]) == len(segs)
        assert np.abs(np.array(got["scores"]) - np.array(want["scores"])).max() < 1e-3, seed


def _pages_single(r, case, lattices):
    traceback, pages = None, []
    for segs in lattices:
        g, s, e = lattice(segs)
        path, entropy, traceback = r.rate_best(g, s, e, start_traceback=traceback, context=[17], lm_weight=case["lm_weight"],
                                               beam_width=case["beam_width"], beam_clustering_dist=case["dist"], edge_walk=True)
        pages.append(path)
    pages.append(r.next_path(traceback[0], ([], traceback[1]))[0])
    return pages


def test_golden_lattices_as_one_batch_on_the_hip_engine_and_a_batch_of_one(monkeypatch):
    from ocrd_keraslm_amd.lib.engine import HipLM
    from tests.test_lattice_batch import _golden_batch
    rounds = []
    real = HipLM.edge_round
    monkeypatch.setattr(HipLM, "edge_round", lambda self, *a, **k: rounds.append(1) or real(self, *a, **k))
    r = make_rater(hip_factory, False, True)
    single = make_rater(hip_factory, False, True)
    for cases, lattices in ((SEAM["rate_best"], SEAM["lattices"]), (SEAM["rate_best_ties"], SEAM["tie_lattices"])):
        pages = _golden_batch(r, cases, lattices)
        for k, case in enumerate(cases):
            want = _pages_single(single, case, lattices)
            for (path, _entropy, _tb), ref, one in zip(pages[k], case["pages"], want):
                assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[p[0], p[1]] for p in ref["path"]]
                assert [(el.id, alt.index) for el, alt, _ in path] == [(el.id, alt.index) for el, alt, _ in one]
    assert rounds                                             # the device decode is what ran
    # a batch of one lattice
    segs = random_segments(207, n_edges=12, empty=False)
    g, s, e = lattice(segs)
    (path, entropy, tb), = r.rate_best_batch([g], [s], [e], contexts=[17])
    g, s, e = lattice(segs)
    one = single.rate_best(g, s, e, context=[17], edge_walk=True)
    assert summary(path, entropy, tb)["path"] == summary(*one)["path"]
    assert summary(path, entropy, tb)["hyps"][0] == summary(*one)["hyps"][0]


def test_a_round_with_an_edge_beyond_the_kernels_capacity_on_the_hip_engine(monkeypatch):
    """the limit lowered to 25 tracks: rounds that hold a larger edge are decoded on the host from the same walk, the others on
    the device -- same path as the single call"""
    monkeypatch.setattr(lattice_batch, "MAX_TRACKS", 25)
    segs = [random_segments(seed, n_edges=10, empty=False) for seed in (207, 208)]
    r = make_rater(hip_factory, False, True)
    single = make_rater(hip_factory, False, True)
    built = [lattice(s) for s in segs]
    results = r.rate_best_batch([b[0] for b in built], [b[1] for b in built], [b[2] for b in built], contexts=[17],
                                beam_clustering_dist=5)
    for s, (path, entropy, tb) in zip(segs, results):
        g, a, b = lattice(s)
        one = single.rate_best(g, a, b, context=[17], beam_clustering_dist=5, edge_walk=True)
        got, want = summary(path, entropy, tb), summary(*one)
        assert got["path"] == want["path"] and got["hyps"][0] == want["hyps"][0] and len(got["hyps"][0]) == len(s)
        assert abs(got["costs"][0] - want["costs"][0]) < 1e-2
