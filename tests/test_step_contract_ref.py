"""The step contract's references, bounds, checker and case table (tests/step_contract.py), without a GPU.

References: the model reference (f64 over the rounded operands) has to agree with the true reference (the oracle's
step_batch in f64) as closely as the dropped lo x lo term allows -- in split precision inside the project's standing
bounds; the distance in bf16 precision is printed.
Bounds: for every case and precision the weakest fault of the catalogue, planted in the model, has to move the result
by at least 8 tol = 64 E32.  Both sides come from references alone.
Checker: planted violations -- a write into a foreign slot, a write behind probs, a marker left in a written slot, a
non-zero padded unit, every fault of the catalogue -- have to be answered with the promise they break, and the
unplanted model passes.
Routes: kl_test_step_route is the plan the dispatch itself asks, host only; kl_bind launches nothing, so a handle bound
to placeholder addresses answers it.  Every case has to take the route its table entry names and every value of every
route field has to be reached."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import step_contract as S  # noqa: E402

PRECS = (S.PREC_SPLIT, S.PREC_BF16)

def _lib():
    from ocrd_keraslm_amd.lib import hipabi
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return hipabi.load()


def route_query(lib, model, n, env=(), ws=True, host=False):
    """kl_test_step_route on a handle bound to placeholder addresses; (return code, route dict)"""
    from ocrd_keraslm_amd.lib import hipabi
    cfg = hipabi.KlConfig(model.depth, model.pwidth, model.V, model.n_ctx, S.CTX_VOCAB, S.CTX_DIM)
    h = lib.kl_create(C.byref(cfg))
    assert h
    try:
        with S.switches(env):
            # (KL_ERR_LAUNCH = 2 on a machine without a GPU: the binding is complete, only the zero page's device address,
            #  which kl_bind resolves last for the thin kernels' launches, is not to be had)
            assert lib.kl_bind(h, 1 << 20, 1 << 30, lib.kl_derived_bytes(h)) in (0, 2)
        view = hipabi.KlStepRoute()
        rc = lib.kl_test_step_route(h, n, int(ws), int(host), C.byref(view))
        return rc, S.route_of(view, model.depth), view
    finally:
        lib.kl_destroy(h)


@pytest.fixture(scope="module")
def world():
    """weights, operands and buffers, built once per (model, precision) / case and shared"""
    cache = {}

    def operands(model, prec):
        key = ("op", model, prec)
        if key not in cache:
            w = S.logical_weights(model)
            flat = S.physical_params(model, w)
            EK, CtxK = S.host_tables(model, flat, prec)
            cache[key] = (w, S.operands(model, flat, EK, CtxK))
        return cache[key]

    def buffers(case):
        key = ("buf", case)
        if key not in cache:
            cache[key] = S.build(case)
        return cache[key]
    return operands, buffers


# ---------------------------------------------------------------- the table
def test_case_names_are_unique():
    names = [c.name for c in S.ALL_CASES]
    assert len(set(names)) == len(names)


def test_table_holds_what_it_must():
    dev = S.DEVICE_CASES
    assert {(m.depth, m.width, m.V, m.n_ctx) for m in S.MODELS} == {
        (2, 64, 50, 1), (2, 128, 60, 1), (2, 256, 40, 1), (2, 512, 256, 1), (2, 512, 230, 2), (2, 768, 50, 0), (2, 1024, 64, 1),
        (2, 100, 50, 1), (2, 200, 50, 1), (2, 128, 1100, 1), (2, 512, 300, 1), (1, 128, 40, 1), (3, 256, 40, 2)}
    assert {c.model for c in dev} == set(S.ALL_MODELS) and set(S.ALL_MODELS) - set(S.MODELS) == {S.M1280}
    rows = {c.n for c in dev}
    assert rows >= {1, 15, 16, 17, 32, 33, 128, 129, 255, 256, 257, 320, 449, 511, 512, 513, 1030}
    assert {c.n for c in dev if c.model is S.M1024} >= {128, 129, 1030}
    assert {c.n for c in dev if c.model is S.M768} >= {200}
    assert {c.n for c in dev if c.model is S.M512 and not c.env} >= {128, 129, 255, 256, 257, 511, 512, 513}
    envs = {c.env for c in dev}
    assert envs >= {(("KL_TILE_ROWS", "128"),), (("KL_INC_TILE", "0"),), (("KL_INC_TILE", "0"), ("KL_INC_SMALL", "0")),
                    (("KL_OUT_FUSED", "0"),), (("KL_OUT_FUSED_MIN", "16"),)}
    host = S.HOST_CASES
    assert {c.n for c in host if c.idx == S.IDX_KERNARG} >= {1, 16, 17, 128, 129, 256}
    assert {c.n for c in host if c.idx == S.IDX_PACKED} >= {257}
    assert any(c.env == (("KL_HOST_KERNARG", "0"),) and c.idx == S.IDX_PACKED for c in host)
    for sel in (lambda c: c.idx == S.IDX_KERNARG, lambda c: c.idx == S.IDX_PACKED):
        assert {(c.by_target, c.head_k > 0) for c in host if sel(c)} >= {(False, False), (True, True), (True, False), (False, True)}
    assert {c.head_k for c in host} == {0, 2} and all(c.head_k in (0, c.model.depth) for c in host)


def test_buffers_hold_what_they_must(world):
    _, buffers = world
    for case in S.ALL_CASES:
        b = buffers(case)
        m, n = case.model, case.n
        assert b.n_slots > n + len(b.parents)
        outs, ins = b.slot_out[:n], b.slot_in[:n]
        assert len(set(outs.tolist())) == n and not set(outs.tolist()) & set(ins.tolist())
        assert b.trap not in outs and b.trap not in ins
        assert (b.slot_in[n:] == b.trap).all() and (b.slot_out[n:] == b.trap).all()
        assert (b.pool[b.trap] == S.MARK_F32).all() and (b.pool[outs] == S.MARK_F32).all() and (b.probs == S.MARK_F32).all()
        assert np.abs(np.diff(np.sort(outs))).max(initial=2) > 1 or n < 3      # scattered, not a run of slots
        h, c = b.states_in()
        assert np.isfinite(h).all() and np.isfinite(c).all() and np.abs(h).max() < 1 and np.abs(h[:, :, :m.width]).min() > 0
        assert (h[:, :, m.width:] == 0).all() and (c[:, :, m.width:] == 0).all()
        assert b.idx.min() >= 0 and b.idx.max() < m.V and b.ctx.min() >= 0 and b.ctx.max() < S.CTX_VOCAB
        assert b.idx.shape == (n + S.GUARD,) and b.ctx.shape[0] == n + S.GUARD
        if n >= 2:
            assert len(set(ins.tolist())) < n                                   # repeated parents
            assert {0, m.V - 1} <= set(b.idx[:n].tolist()) and {0, S.CTX_VOCAB - 1} <= set(b.ctx[:n].reshape(-1).tolist())
            assert (ins[0] != ins[n - 1]) or n == 2


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("model", S.ALL_MODELS, ids=lambda m: m.name)
def test_model_reference_against_true_reference(world, model, capsys):
    operands, buffers = world
    case = min((c for c in S.DEVICE_CASES if c.model is model and c.n >= 16), key=lambda c: c.n)
    b = buffers(case)
    n = case.n
    h_in, c_in = b.states_in()
    for prec in PRECS:
        w, op = operands(model, prec)
        H, Cc = S.model_layers(op, prec, b.idx[:n], b.ctx[:n], h_in, c_in)
        P = S.model_output(op, prec, H[-1].astype(np.float32))
        tp, tH, tC = S.true_reference(model, w, b.idx[:n], b.ctx[:n], h_in, c_in)
        W = model.width
        ds = max(np.abs(H[:, :, :W] - tH).max(), np.abs(Cc[:, :, :W] - tC).max())
        dp = np.abs(P - tp).max()
        assert (H[:, :, W:] == 0).all() and (Cc[:, :, W:] == 0).all()
        with capsys.disabled():
            print("\n  %s n=%d %s: model - true: states %.3g, probabilities %.3g" % (model.name, n, "split" if prec == 3 else "bf16", ds, dp))
        if prec == S.PREC_SPLIT:      # the lo x lo term and the f32 tables are all that separates the two
            assert ds < S.TRUE_STATES / 4 and dp < S.TRUE_PROBS / 4, (ds, dp)
        else:
            assert ds < 0.1 and dp < 0.1, (ds, dp)


@pytest.mark.parametrize("case", S.ALL_CASES, ids=lambda c: c.name)
def test_weakest_fault_is_far_above_the_tolerance(world, case, capsys):
    operands, buffers = world
    for prec in PRECS:
        _, op = operands(case.model, prec)
        dev, (es, ep) = S.fault_deviations(buffers(case), op, prec)
        assert set(dev) == set(S.applicable_faults(case.model, min(case.n, S.FAULT_ROWS), prec))
        weakest = min(dev, key=dev.get)
        with capsys.disabled():
            print("\n  %s %s: E32 states %.3g probs %.3g; weakest fault %s at %.1f tol"
                  % (case.name, "split" if prec == 3 else "bf16", es, ep, weakest, dev[weakest]))
        assert 0 < es < 1e-5 and 0 < ep < 1e-4, (es, ep)
        assert dev[weakest] >= S.TOL_FACTOR, dev


# ---------------------------------------------------------------- the checker
CHECK_CASES = [c for c in S.ALL_CASES if c.name in ("d2w100v50c1-n33", "d2w512v256c1-n16-host-pick-k2", "d3w256v40c2-n33")]


def _refs(world, case, prec):
    operands, buffers = world
    w, op = operands(case.model, prec)
    b = buffers(case)
    return b, S.references(b, w, op, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CHECK_CASES, ids=lambda c: c.name)
def test_checker_passes_the_model_and_names_the_broken_promise(world, case, prec):
    assert len(CHECK_CASES) == 3
    b, refs = _refs(world, case, prec)
    n, m = case.n, case.model
    pool, probs = S.model_result(b, refs)
    metrics = S.check(b, refs, pool, probs)
    assert metrics["state_ratio"] < 1 and metrics["prob_ratio"] < 1      # (the rounding to f32 alone)

    def broken(pool_, probs_):
        with pytest.raises(S.ContractFailure) as e:
            S.check(b, refs, pool_, probs_)
        return e.value.promise
    one = np.float32(0.25).view(np.uint32)
    for slot in (b.trap, int(b.parents[0]), int(np.setdiff1d(np.arange(b.n_slots), np.r_[b.parents, b.slot_out[:n], b.trap])[0])):
        p2 = pool.copy()
        p2[slot, 1, 3] = one
        assert broken(p2, probs) == "slots"
    q2 = probs.copy()
    q2.reshape(-1)[(n if case.by_target else n * m.V)] = one
    assert broken(pool, q2) == "probs-tail"
    q2 = probs.copy()
    q2[-1, -1] = one
    assert broken(pool, q2) == "probs-tail"
    p2 = pool.copy()
    p2[b.slot_out[n - 1], 2 * m.depth - 1, m.width - 1] = S.MARK_F32      # the last row's last unit never written
    assert broken(p2, probs) == "finite"
    q2 = probs.copy()
    q2.reshape(-1)[n - 1] = S.MARK_F32
    assert broken(pool, q2) == "finite"
    if m.pwidth > m.width:
        p2 = pool.copy()
        p2[b.slot_out[0], 0, m.width] = np.float32(1e-30).view(np.uint32)
        assert broken(p2, probs) == "padding"
    for fault in S.applicable_faults(m, n, prec):
        assert broken(*S.model_result(b, refs, fault)) == "model", fault
    # a row that is wrong by the standing bound but not more is the model promise's, not the true reference's
    p2 = pool.copy()
    v = p2[b.slot_out[0], 0].view(np.float32)
    v[0] += np.float32(5e-5)
    assert broken(p2, probs) == "model"
    if case.head_k:
        heads = pool[b.slot_out[:n]].reshape(n, -1)[:, :case.head_k * m.pwidth].copy()
        S.check(b, refs, pool, probs, heads.view(np.float32))
        heads[n - 1, -1] ^= 1
        with pytest.raises(S.ContractFailure) as e:
            S.check(b, refs, pool, probs, heads.view(np.float32))
        assert e.value.promise == "model"


# ---------------------------------------------------------------- the routes
@pytest.mark.parametrize("case", S.ALL_CASES, ids=lambda c: c.name)
def test_case_takes_the_route_its_entry_names(case):
    rc, got, view = route_query(_lib(), case.model, case.n, case.env, case.ws, case.host)
    assert rc == 0
    assert got == S.route_fields(case), (case.route_name, got)
    assert view.lo == 0                       # (bound, not prepared: the GPU tests see the precision's value)


def test_every_route_value_is_reached():
    seen = {}
    for case in S.ALL_CASES:
        for k, v in S.route_fields(case).items():
            seen.setdefault(k, set()).update(v if isinstance(v, tuple) else (v,))
    assert seen["layers"] == {S.TILES, S.CELLS, S.GEMM_FUSED, S.GEMM_PLAIN, S.THIN}
    assert seen["out"] == {S.OUT_FUSED, S.OUT_THIN, S.OUT_BIG}
    assert seen["idx"] == {S.IDX_DEVICE, S.IDX_KERNARG, S.IDX_PACKED}
    assert seen["gathered"] == {0, 1} and seen["depth"] == {1, 2, 3}
    assert seen["nmt"] == {0, 1, 2} and seen["gen"] == {0, 1}
    assert seen["tile_rows"] == {0, 64, 128}
    # the XCD partition: none (every other route: at the tile kernel's widths, multiples of 256, the grid's W / 32 unit
    # blocks always divide by 8, so a tiled step is always partitioned), eight unit-block groups, and row-tile groups
    assert seen["px"] == {0, 4, 8} and seen["py"] == {0, 1, 2}
    # cells with different row tiles per layer, both kernels' index forms, both widths classes at one and two row tiles
    assert any(len(set(c.nmt)) == 2 for c in S.ALL_CASES)
    for idx in (S.IDX_DEVICE, S.IDX_KERNARG):
        assert {(c.gen, c.nmt[0]) for c in S.ALL_CASES if c.layers == S.CELLS and c.idx == idx} >= {(0, 1), (0, 2), (1, 1)}
    assert {(c.gen, c.nmt[0]) for c in S.ALL_CASES if c.layers == S.CELLS} >= {(1, 2)}


def test_route_query_answers_as_the_step_would():
    lib = _lib()
    from ocrd_keraslm_amd.lib import hipabi
    view = hipabi.KlStepRoute()
    assert lib.kl_test_step_route(None, 16, 1, 0, C.byref(view)) == 5                 # KL_ERR_ARG
    cfg = hipabi.KlConfig(2, 512, 256, 1, 200, 10)
    h = lib.kl_create(C.byref(cfg))
    assert lib.kl_test_step_route(h, 16, 1, 0, C.byref(view)) == 3                    # KL_ERR_STATE: nothing bound
    lib.kl_destroy(h)
    assert route_query(lib, S.M512, 0)[0] == 5
    # two context variables: the gathered gate inputs need the workspace (the host entry always has it)
    assert route_query(lib, S.M512C2, 17, ws=False)[0] == 4                            # KL_ERR_WORKSPACE
    assert route_query(lib, S.M512C2, 17, ws=False, host=True)[0] == 0
    # width 1280: layer 0 (K = 1280) fits the cell kernel's LDS, layer 1 (K = 2560) does not -- the step goes to the thin
    # kernel whole (it used to run layer 0 and then fail), from 129 rows on to the tiles
    wide = S.M1280
    assert route_query(lib, wide, 64)[1]["layers"] == S.THIN
    assert route_query(lib, wide, 64, host=True)[1]["idx"] == S.IDX_PACKED
    assert route_query(lib, wide, 129)[1]["layers"] == S.TILES
    assert route_query(lib, S.Model(1, 1280, 64, 1), 64)[1]["layers"] == S.CELLS
    # out_fused_min and the cell kernel's first row count move with their switches
    assert route_query(lib, S.M512, 16, env=(("KL_INC_SMALL_MIN", "17"),))[1]["layers"] == S.THIN
    assert route_query(lib, S.M512, 256, env=(("KL_INC_TILE", "0"), ("KL_INC_SMALL", "0"), ("KL_FUSED_STEP", "0")))[1]["layers"] == S.GEMM_PLAIN
    assert route_query(lib, S.M512, 256, env=(("KL_INC_TILE", "0"), ("KL_INC_SMALL", "0")), ws=False)[1]["layers"] == S.THIN
