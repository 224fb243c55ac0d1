"""Edge walk on the GPU (-m gpu): kl_walk_batch_host through `HipLM.walk_host` against the f64 oracle's chained steps, the
lattice decoder with `edge_walk=True` on the HIP engine against the golden fixtures and against the CPU double's stepwise
decoder, and the OCR-D processor with KERASLM_EDGE_WALK=1.

Bounds are the project's existing ones for chained steps (tests/test_gpu_kernels.py::test_step_batch_parity, DESIGN.md
section 2): probabilities 2e-5 and states 1e-4 in split precision, probabilities 1e-3 in bf16, 1e-4 on the peaked model.
Every device call waits on its arrival word with walk_host's time limit (20 s) and nothing is retried."""
import ctypes as C
import gc
import importlib
import sys

import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests.edge_walk_cases import chained_reference, random_segments, run_pages
from tests.oracle_engine import OracleLM
from tests.test_rater_golden import SEAM, hip_factory, lattice, make_rater
from tests.test_wrapper_processor import SHIM, glyph_equivs, make_workspace, model_file  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _make_model(depth, width, voc, n_ctx, env, monkeypatch, emb_std=0.5):
    from tests.test_gpu_kernels import make_model
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return make_model(depth, width, voc, n_ctx, emb_std=emb_std)      # (the switches are read when the handle is created)


def _lengths(rng, n, mode):
    if mode == "ragged":
        return rng.integers(1, 25, n)
    if mode == "equal":
        return np.full(n, 9)
    return np.ones(n, dtype=np.int64)


def _case(rng, cfg, n, lens, n_parents, duplicate=True):
    """index arrays of one walk: parents with repeats, new states anywhere in the pool, rows in no particular order; the last
    row repeats the first (same parent, same characters) when there are two or more"""
    lens = np.asarray(lens).copy()
    if duplicate and n >= 2:
        lens[-1] = lens[0]
    total = int(lens.sum())
    n_slots = n_parents + total + 11
    perm = rng.permutation(n_slots)
    parents = perm[:n_parents]
    slot_in = parents[rng.integers(0, n_parents, n)]
    slot_step = perm[n_parents:n_parents + total]
    idx = rng.integers(0, cfg.voc_size, total)
    target = rng.integers(0, cfg.voc_size, total)
    ctx = rng.integers(0, 200, (n, cfg.n_ctx))
    if duplicate and n >= 2:
        k = int(lens[0])
        idx[total - k:] = idx[:k]
        target[total - k:] = target[:k]
        ctx[-1] = ctx[0]
        slot_in[-1] = slot_in[0]
    return n_slots, parents, lens, idx, target, ctx, slot_in, slot_step


SHAPES = [
    # depth, width, voc, n_ctx, n, lengths, head_k, env
    # indices in the kernel arguments: one and two row tiles, groups beyond 256 rows, all-equal lengths, a single length-1 row
    (2, 512, 256, 1, 128, "ragged", 2, {}), (2, 512, 256, 1, 256, "ragged", 0, {}), (2, 512, 256, 1, 300, "ragged", 2, {}),
    (2, 512, 256, 1, 50, "equal", 0, {}), (2, 512, 256, 1, 1, "one", 2, {}), (2, 64, 50, 1, 256, "equal", 0, {}),
    (1, 64, 50, 1, 7, "ragged", 1, {}), (3, 128, 60, 1, 50, "ragged", 3, {}),
    # a zero-padded width; a vocabulary of more than 256 characters (a wave takes column tiles in several rounds)
    (2, 100, 50, 1, 50, "ragged", 2, {}), (2, 128, 300, 1, 7, "ragged", 2, {}),
    # the staged upload + chained device-pointer step: 0 / 2 context variables, the switch, 300 rows on the tile kernels
    (2, 512, 64, 0, 50, "ragged", 0, {}), (3, 128, 40, 2, 128, "ragged", 3, {}),
    (2, 512, 256, 1, 7, "ragged", 2, {"KL_HOST_KERNARG": "0"}), (2, 512, 256, 1, 300, "ragged", 0, {"KL_HOST_KERNARG": "0"}),
    # vocabularies of trained models at width 512: no multiple of 16, and more than 256 characters
    (2, 512, 230, 1, 128, "ragged", 2, {}), (2, 512, 300, 1, 300, "ragged", 0, {}),
]


@pytest.mark.parametrize("depth,width,voc,n_ctx,n,mode,head_k,env", SHAPES)
def test_walk_host_parity_with_chained_oracle_steps(monkeypatch, depth, width, voc, n_ctx, n, mode, head_k, env):
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = _make_model(depth, width, voc, n_ctx, env, monkeypatch)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    rng = np.random.default_rng(31)
    n_parents = max(1, n // 3)
    n_slots, parents, lens, idx, target, ctx, slot_in, slot_step = _case(rng, cfg, n, _lengths(rng, n, mode), n_parents)
    lm.ensure_pool(n_slots)
    lm.pool.zero_()
    parent_states = rng.uniform(-0.5, 0.5, (n_parents, 2 * depth, width)).astype(np.float32)
    lm.pool_write(parents, parent_states)
    pool64 = np.zeros((n_slots, 2 * depth, width), dtype=np.float64)
    pool64[parents] = parent_states
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    ref, last = chained_reference(cfg, w64, pool64, [int(k) for k in lens], idx, target, ctx, slot_in, slot_step)

    tprob, heads = lm.walk_host(lens, idx, target, ctx, slot_in, slot_step, head_k=head_k)
    assert tprob.shape == ref.shape and tprob.dtype == np.float32
    worst = np.abs(tprob - ref).max()
    states = lm.pool_read(slot_step)
    worst_state = np.abs(states - pool64[slot_step]).max()
    print("walk parity: max |dp| %.3g, max |dstate| %.3g over %d steps of %d rows" % (worst, worst_state, len(ref), n))
    assert worst < 2e-5, worst
    assert worst_state < 1e-4, worst_state
    if head_k:
        assert heads.shape == (n, head_k, width)
        assert np.abs(heads - pool64[last, :head_k]).max() < 1e-4
        assert np.array_equal(heads, lm.pool_read(last)[:, :head_k])       # the heads ARE the final states' first vectors
    else:
        assert heads is None
    assert np.array_equal(lm.pool_read(parents), parent_states)           # slot_in slots: bit-unchanged
    if n >= 2:                                                              # duplicate rows: bitwise equal
        k = int(lens[0])
        assert np.array_equal(tprob[:k], tprob[len(tprob) - k:])
        assert np.array_equal(states[:k], states[len(states) - k:])
    # two calls on the same inputs: bit-identical
    tprob2, heads2 = lm.walk_host(lens, idx, target, ctx, slot_in, slot_step, head_k=head_k)
    assert np.array_equal(tprob, tprob2)
    assert np.array_equal(states, lm.pool_read(slot_step))
    if head_k:
        assert np.array_equal(heads, heads2)


def test_walk_host_row_order_does_not_matter(monkeypatch):
    """the library orders the rows itself: the same rows handed over in another order give bitwise the same numbers"""
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n = 2, 512, 256, 50
    cfg, w, lm = _make_model(depth, width, voc, 1, {}, monkeypatch)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    rng = np.random.default_rng(32)
    n_slots, parents, lens, idx, target, ctx, slot_in, slot_step = _case(rng, cfg, n, _lengths(rng, n, "ragged"), 9, duplicate=False)
    lm.ensure_pool(n_slots)
    lm.pool.zero_()
    lm.pool_write(parents, rng.uniform(-0.5, 0.5, (9, 2 * depth, width)).astype(np.float32))
    tprob, _ = lm.walk_host(lens, idx, target, ctx, slot_in, slot_step)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    order = rng.permutation(n)
    take = np.concatenate([np.arange(off[i], off[i] + lens[i]) for i in order])
    tprob_p, _ = lm.walk_host(lens[order], idx[take], target[take], ctx[order], slot_in[order], slot_step[take])
    assert np.array_equal(tprob_p, tprob[take])


def test_walk_host_peaked_model_and_bf16(monkeypatch):
    """the peaked model of test_step_batch_peaked_model_split_precision (1e-4 in split precision) and the bf16 bar (1e-3)"""
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n, steps = 2, 512, 256, 96, 96
    cfg, w, lm = _make_model(depth, width, voc, 1, {}, monkeypatch, emb_std=1.0)
    w = dict(w)
    for k in w:
        if k.startswith(("K", "U")):
            w[k] = (w[k] * 2.5).astype(np.float32)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    rng = np.random.default_rng(12)
    lens = np.full(n, steps)
    idx = rng.integers(1, voc, n * steps)
    ctx = rng.integers(0, 200, (n, 1))
    slot_step = 1 + np.arange(n * steps)
    slot_in = np.zeros(n, dtype=np.int64)
    # the target of every (row, step) pair is the oracle's most likely character: the peak itself
    off = np.arange(n) * steps
    st = O.zero_states(cfg, n, np.float64)
    target = np.zeros(n * steps, dtype=np.int64)
    ref = np.zeros(n * steps)
    peak = 0.0
    for t in range(steps):
        p, st = O.step_batch(cfg, w64, idx[off + t], ctx, st)
        target[off + t] = p.argmax(axis=1)
        ref[off + t] = p.max(axis=1)
        peak = max(peak, float(np.median(p.max(axis=1))))
    assert peak > 0.3, peak
    worst = {}
    for prec in (hipabi.KL_PREC_SPLIT, hipabi.KL_PREC_BF16):
        lm.set_weights(w, prec)
        lm.ensure_pool(1 + n * steps)
        lm.pool.zero_()
        tprob, _ = lm.walk_host(lens, idx, target, ctx, slot_in, slot_step)
        worst[prec] = np.abs(tprob - ref).max()
    print("walk on the peaked model: max |dp| split %.3g, bf16 %.3g" % (worst[hipabi.KL_PREC_SPLIT], worst[hipabi.KL_PREC_BF16]))
    assert worst[hipabi.KL_PREC_SPLIT] < 1e-4, worst
    # the bf16 bar on the model the existing bf16 test uses (flat synthetic weights)
    cfg, w, lm = _make_model(depth, width, voc, 1, {}, monkeypatch)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    n, steps = 64, 64
    lens = np.full(n, steps)
    idx, target = rng.integers(1, voc, n * steps), rng.integers(0, voc, n * steps)
    ctx = rng.integers(0, 200, (n, 1))
    slot_step, slot_in = 1 + np.arange(n * steps), np.zeros(n, dtype=np.int64)
    ref, _ = chained_reference(cfg, w64, np.zeros((1 + n * steps, 2 * depth, width)), [steps] * n, idx, target, ctx, slot_in, slot_step)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.ensure_pool(1 + n * steps)
    lm.pool.zero_()
    tprob, _ = lm.walk_host(lens, idx, target, ctx, slot_in, slot_step)
    assert np.abs(tprob - ref).max() < 1e-3, np.abs(tprob - ref).max()


def test_walk_argument_errors_return_their_codes_without_launching(monkeypatch):
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n = 2, 128, 60, 5
    cfg, w, lm = _make_model(depth, width, voc, 1, {}, monkeypatch)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.ensure_pool(64)
    lm.pool.zero_()
    lens = np.array([3, 1, 2, 4, 2], dtype=np.int32)
    total = int(lens.sum())
    idx = np.arange(total, dtype=np.int32) % voc
    ctx = np.zeros((n, 1), dtype=np.int32)
    slot_in = np.zeros(n, dtype=np.int32)
    slot_step = np.arange(1, 1 + total, dtype=np.int32)
    tprob, _ = lm.walk_host(lens, idx, idx, ctx, slot_in, slot_step)      # (a good call first: buffers, workspace, ticket)
    assert np.all(tprob > 0)
    io, lib = lm._hio, lm.lib
    ticket = io["ticket"]
    before = lm.pool_read(np.arange(64))
    stream = C.c_void_p(lm.torch.cuda.current_stream(lm.device).cuda_stream)
    ws, ws_bytes = lm._walk_ws.data_ptr(), lm._walk_ws.numel()

    def call(handle=lm.handle, n=n, lens=lens, idx=idx, head_k=0, heads=io["ptr"]["heads"], ws_bytes=ws_bytes, stage=lm._wstage[0]):
        return lib.kl_walk_batch_host(handle, n, lens.ctypes.data, idx.ctypes.data if idx is not None else None, idx.ctypes.data if idx is not None else None,
                                      ctx.ctypes.data, slot_in.ctypes.data, slot_step.ctypes.data, lm.pool.data_ptr(), head_k,
                                      io["ptr"]["probs"], heads, stage, io["ptr"]["done"], ticket + 1, ws, ws_bytes, stream)

    KL_ERR_STATE, KL_ERR_WORKSPACE, KL_ERR_ARG = 3, 4, 5
    assert call(n=0) == KL_ERR_ARG
    assert call(idx=None) == KL_ERR_ARG
    assert call(stage=None) == KL_ERR_ARG
    assert call(lens=np.array([3, 0, 2, 4, 2], dtype=np.int32)) == KL_ERR_ARG
    assert call(lens=np.array([3, 1025, 2, 4, 2], dtype=np.int32)) == KL_ERR_ARG
    assert call(head_k=2 * depth + 1) == KL_ERR_ARG
    assert call(head_k=1, heads=None) == KL_ERR_ARG
    assert call(ws_bytes=64) == KL_ERR_WORKSPACE
    fresh = lib.kl_create(C.byref(lm.cfg))                                 # never bound, never prepared
    try:
        assert call(handle=fresh) == KL_ERR_STATE
    finally:
        lib.kl_destroy(fresh)
    assert lib.kl_walk_workspace_bytes(lm.handle, 0, 0) == 0 and lib.kl_walk_stage_bytes(lm.handle, 5, 4) == 0
    lm.torch.cuda.synchronize()
    assert int(io["np"]["done"][0]) == ticket                              # nothing was launched: no arrival, no state touched
    assert np.array_equal(lm.pool_read(np.arange(64)), before)


# ---------------------------------------------------------------------------------------------------------------- decoder
def _golden_pages(r, case, lattices):
    traceback = None
    pages = []
    for segs in lattices:
        g, s, e = lattice(segs)
        path, entropy, traceback = r.rate_best(g, s, e, start_traceback=traceback, context=[17], lm_weight=case["lm_weight"],
                                               beam_width=case["beam_width"], beam_clustering_dist=case["dist"], edge_walk=True)
        pages.append((path, entropy, traceback))
    path, entropy, traceback = r.next_path(traceback[0], ([], traceback[1]))
    pages.append((path, entropy, traceback))
    return pages


def _count_walks(monkeypatch):
    from ocrd_keraslm_amd.lib.engine import HipLM
    calls = []
    real = HipLM.walk_host
    monkeypatch.setattr(HipLM, "walk_host", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    return calls


def test_golden_lattices_on_the_hip_engine_with_edge_walk(monkeypatch):
    """the assertions of test_rate_best_matches_reference[hip] / ..._exact_ties_...[hip]: exact paths, 1e-3 scores, 0.1 on
    entropy and beam costs"""
    tol = 1e-3
    calls = _count_walks(monkeypatch)
    r = make_rater(hip_factory, False, True)
    for case in SEAM["rate_best"]:
        for (path, entropy, tb), ref in zip(_golden_pages(r, case, SEAM["lattices"]), case["pages"]):
            assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[a, b] for a, b, _ in ref["path"]]
            scores = np.array([s for _, _, s in path])
            assert np.abs(scores - np.array([s for _, _, s in ref["path"]])).max(initial=0) < tol
            assert abs(entropy - ref["entropy"]) < tol * 100
            assert len(tb[0]) == len(ref["beam"])
            assert np.abs(np.array([n.cum_cost for n in tb[0]]) - np.array(ref["beam"])).max(initial=0) < tol * 100
    assert len(calls) == len(SEAM["rate_best"]) * sum(len(segs) for segs in SEAM["lattices"])      # one walk per edge
    for case in SEAM["rate_best_ties"]:
        for (path, entropy, tb), ref in zip(_golden_pages(r, case, SEAM["tie_lattices"]), case["pages"]):
            assert [[el.id, alt.Unicode] for el, alt, _ in path] == [[a, b] for a, b, _, _ in ref["path"]]
            assert len(tb[0]) == len(ref["beam"])
            assert abs(entropy - ref["entropy"]) < tol * 100


# Seeds of the random lattices (tests/edge_walk_cases.py::random_segments, no empty alternative): all of 200 .. 219.  On the f64
# CPU double the margin between the best and the second-best final hypothesis exceeds 0.05 bits for every one of them at both
# beam widths (checked when the list was committed; the test computes the margins again and asserts the share).
GPU_SEEDS = list(range(200, 220))
MARGIN = 0.05


@pytest.mark.parametrize("beam_width,dist", [(10, 0), (3, 5)])
def test_random_lattices_edge_walk_on_the_gpu_chooses_the_cpu_doubles_path(monkeypatch, beam_width, dist):
    calls = _count_walks(monkeypatch)
    cpu = make_rater(OracleLM, False, True)
    gpu = make_rater(hip_factory, False, True)
    kept = []
    for seed in GPU_SEEDS:
        segs = random_segments(seed, empty=False)
        ref = run_pages(cpu, [segs], beam_width=beam_width, dist=dist, edge_walk=False)
        costs = ref[0]["costs"]
        margin = costs[1] - costs[0] if len(costs) > 1 else float("inf")
        if margin <= MARGIN:
            continue
        kept.append(seed)
        got = run_pages(gpu, [segs], beam_width=beam_width, dist=dist, edge_walk=True)
        assert got[-1]["path"] == ref[-1]["path"], seed
        assert len(got[-1]["path"]) == len(segs)
        assert np.abs(np.array(got[-1]["scores"]) - np.array(ref[-1]["scores"])).max() < 1e-3, seed
    for d0 in range(0, len(GPU_SEEDS), 10):
        decade = GPU_SEEDS[d0:d0 + 10]
        assert sum(s in kept for s in decade) >= 8, (decade, kept)
    assert len(calls) == 30 * len(kept)


# ---------------------------------------------------------------------------------------------------------------- processor
def test_processor_with_edge_walk_switch_chooses_the_same_paths(monkeypatch, tmp_path, model_file):
    """KERASLM_EDGE_WALK=1 through the OCR-D processor (tests/ocrd_shim): same texts, same surviving alternatives, confidences
    within 1e-3 of the run without it -- and the walk really is what ran"""
    def run(where):
        monkeypatch.syspath_prepend(SHIM)
        for name in [m for m in sys.modules if m == "ocrd" or m.startswith(("ocrd.", "ocrd_"))]:
            monkeypatch.delitem(sys.modules, name)
        monkeypatch.delitem(sys.modules, "ocrd_keraslm_amd.wrapper.rate", raising=False)
        mod = importlib.import_module("ocrd_keraslm_amd.wrapper.rate")
        engine = importlib.import_module("ocrd_keraslm_amd.lib.engine")      # (re-imported with the package: count on THIS class)
        real = engine.HipLM.walk_host
        monkeypatch.setattr(engine.HipLM, "walk_host", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
        where.mkdir(parents=True, exist_ok=True)
        ws, pages = make_workspace(mod, where, 3, {1: [('b', 0.9), ('h', 0.85)]})
        proc = mod.KerasRate(ws, {'model_file': model_file, 'textequiv_level': 'glyph', 'alternative_decoding': True,
                                  'beam_width': 4, 'lm_weight': 0.5}, 'OCR-D-IN', 'OCR-D-OUT')
        assert type(proc.rater.model).__name__ == "HipLM"
        switch = proc.rater.edge_walk
        proc.process_workspace(ws)
        texts = [page.get_Page().get_TextRegion()[0].get_TextEquiv()[0].Unicode for page in pages]
        confs = []
        for page in pages:
            for tes in glyph_equivs(page):
                assert len(tes) == 1
                confs.append((tes[0].Unicode, tes[0].conf))
        del proc
        gc.collect()
        return switch, texts, confs, [f.ID for f in ws.mets.find_files(fileGrp='OCR-D-OUT')]

    calls = []
    monkeypatch.delenv("KERASLM_EDGE_WALK", raising=False)
    ref = run(tmp_path / "stepwise")
    assert ref[0] is False and not calls
    monkeypatch.setenv("KERASLM_EDGE_WALK", "1")
    got = run(tmp_path / "walk")
    assert got[0] is True and calls
    assert got[1] == ref[1] and got[3] == ref[3]
    assert [u for u, _ in got[2]] == [u for u, _ in ref[2]]
    for (_, a), (_, b) in zip(got[2], ref[2]):
        assert abs(a - b) < 1e-3, (a, b)

