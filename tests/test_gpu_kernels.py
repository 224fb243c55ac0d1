"""GPU parity tests (run with -m gpu on an MI355X): every test calls the HIP path
through the C ABI (ocrd_keraslm_amd/libkeraslm_hip.so) and compares with the numpy
oracle (oracle/lstm_oracle.py) on the same seeded inputs.

Tolerances: north_star asks for probabilities within 1e-3 of the reference; the
split-bf16 inference path is held to 2e-5, the bf16 training path to bf16-level
relative error on gradients (stated per test)."""
import ctypes as C

import numpy as np
import pytest

from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def bf16_bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def dev(a):
    torch = _torch()
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("M,N,K,out_mode,splits", [
    (128, 128, 64, 0, 1), (200, 136, 72, 0, 1), (64, 2048, 512, 1, 1), (1, 16, 8, 0, 1),
    (512, 2048, 4096, 2, 8), (130, 70, 200, 2, 3), (4096, 256, 512, 0, 1),
    # long-K kernel (256 x 128 tiles fed by LDS-DMA): whole tiles, ragged tiles, odd k-step counts
    (512, 256, 16384, 2, 8), (300, 200, 8192, 2, 4), (256, 128, 8256, 2, 1), (100, 520, 12352, 2, 2),
    # ... with plain stores: many-row shapes (row-contiguous f32 epilogue through LDS; ragged last row tile)
    (65536, 128, 256, 0, 1), (33000, 256, 320, 0, 1), (32768, 384, 256, 1, 1),
    # ... several tiles per CU: persistent workgroups, register epilogue (ragged last row tile, ragged column tile, one k-step more than the ring)
    (131072, 128, 512, 0, 1), (66000, 256, 448, 0, 1), (140000, 200, 384, 0, 1), (70000, 512, 64 * 9, 0, 1),
    # ... and its 64 x 128 tile variant for M ~ 1e3 (the incremental step's shapes)
    (1024, 2048, 1536, 0, 1), (600, 3072, 576, 0, 1), (1024, 3072, 512, 1, 1)])
def test_gemm_tn(M, N, K, out_mode, splits):
    torch = _torch()
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A = bf16_bits(rng.standard_normal((M, K)).astype(np.float32))
    B = bf16_bits(rng.standard_normal((N, K)).astype(np.float32) * (1 + np.arange(N)[:, None] % 5))
    bias = rng.standard_normal(N).astype(np.float32)
    ref = bits_to_f32(A).astype(np.float64) @ bits_to_f32(B).astype(np.float64).T + bias
    Ad, Bd, biasd = dev(A), dev(B), dev(bias)
    if out_mode == 1:
        Cd = torch.zeros((M, N), dtype=torch.int16, device="cuda")
    else:
        Cd = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    hipabi.check(lib.kl_test_gemm_tn(ptr(Ad), ptr(Bd), ptr(Cd), ptr(biasd), M, N, K, K, K, N, out_mode, splits, None))
    torch.cuda.synchronize()
    if out_mode == 1:
        got = bits_to_f32(Cd.cpu().numpy().view(np.uint16))
        tol = 1e-2
    else:
        got = Cd.cpu().numpy()
        tol = 1e-5
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= tol * scale, (np.abs(got - ref).max(), scale)


@pytest.mark.parametrize("M,N,K,lda,c_t,b_km", [(256, 128, 1024, 256, 0, 0), (2048, 512, 16384, 2048, 1, 0), (512, 200, 8256, 640, 0, 0),
                                                (1024, 256, 4096, 1024, 1, 0), (256, 64, 64, 256, 0, 0),
                                                # ... with the B operand K-major too (activations as the forward scan writes them)
                                                (2048, 512, 16384, 2048, 1, 1), (256, 512, 8192, 256, 0, 1), (512, 200, 4160, 512, 1, 1),
                                                (256, 128, 64, 320, 0, 1)])
def test_gemm_an(M, N, K, lda, c_t, b_km):
    """the weight-gradient contraction with K-major operands (rows of dZ / of the activations as the scans
    write them, read with the hardware transpose): C (+)= A^T . B^T, optionally accumulated transposed"""
    torch = _torch()
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    rng = np.random.default_rng(M + 3 * N + K)
    A = bf16_bits(rng.standard_normal((K, lda)).astype(np.float32) * (1 + np.arange(lda)[None, :] % 3))
    ldb = (N + 40) if b_km else K
    if b_km:
        B = bf16_bits(rng.standard_normal((K, ldb)).astype(np.float32) * (1 + np.arange(ldb)[None, :] % 5))
        Bmat = bits_to_f32(B)[:, :N].T
    else:
        B = bf16_bits(rng.standard_normal((N, K)).astype(np.float32) * (1 + np.arange(N)[:, None] % 5))
        Bmat = bits_to_f32(B)
    ref = bits_to_f32(A)[:, :M].astype(np.float64).T @ Bmat.astype(np.float64).T
    Ad, Bd = dev(A), dev(B)
    Cd = torch.zeros((N, M) if c_t else (M, N), dtype=torch.float32, device="cuda")
    hipabi.check(lib.kl_test_gemm_an(ptr(Ad), ptr(Bd), ptr(Cd), M, N, K, lda, ldb, M if c_t else N, c_t, b_km, None))
    torch.cuda.synchronize()
    got = Cd.cpu().numpy()
    if c_t:
        got = got.T
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-5 * scale, (np.abs(got - ref).max(), scale)


@pytest.mark.parametrize("M,N,K,split", [(5, 20, 64, 3), (33, 256, 512, 3), (256, 100, 128, 1), (64, 2048, 512, 3)])
def test_thin_gemm(M, N, K, split):
    torch = _torch()
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Wt = (rng.standard_normal((N, K)) * (1 + np.arange(N)[:, None] % 3)).astype(np.float32)
    hi = bf16_bits(Wt)
    lo = bf16_bits(Wt - bits_to_f32(hi))
    Ad, hid, lod = dev(A), dev(hi), dev(lo)
    Cd = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    hipabi.check(lib.kl_test_thin_gemm(ptr(Ad), K, ptr(hid), ptr(lod), K, M, N, K, ptr(Cd), N, split, None))
    torch.cuda.synchronize()
    got = Cd.cpu().numpy()
    if split == 3:
        ref = A.astype(np.float64) @ Wt.astype(np.float64).T
        tol = 3e-5
    else:
        ref = bits_to_f32(bf16_bits(A)).astype(np.float64) @ bits_to_f32(hi).astype(np.float64).T
        tol = 1e-5
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max()


def make_model(depth, width, voc, n_ctx=1, seed=4, emb_std=0.5):
    from ocrd_keraslm_amd.lib.engine import HipLM
    from tests.gradcheck import cached_weights
    cfg = O.ModelConfig(depth, width, voc, n_ctx)
    w = cached_weights(depth, width, voc, n_ctx, seed, emb_std)      # (read-only arrays, shared between tests)
    lm = HipLM(depth, width, voc, n_ctx)
    return cfg, w, lm


# (the routes named here are what kl_test_step_route reports for the shape at its physical width -- 96 and 100 run at 128, 200
#  at 256, 768 at 1024 -- with a workspace and no KL_* switch set; tests/test_step_contract_gpu.py asserts the routes of its cases)
@pytest.mark.parametrize("depth,width,voc,n,n_ctx", [(2, 64, 50, 5, 1), (2, 512, 256, 70, 1), (1, 128, 40, 33, 1),
                                                     (3, 96, 30, 17, 2),
                                                     # 16 <= n < 256: inc_cell_kernel (step_small.hip), one row tile per workgroup up to 128 rows,
                                                     # two above, K = W and 2W, several context variables (thin before: fewer than 16 rows, width 64)
                                                     (2, 512, 256, 128, 1), (2, 512, 256, 200, 1), (3, 256, 40, 100, 2),
                                                     # width 1024 above 128 rows: inc_tile_kernel on 64-row tiles, px 8
                                                     (4, 1024, 64, 130, 2),
                                                     # ... widths 64 and 128 (inc_cell_kernel's GEN instantiation: a staging instruction covers several
                                                     # rows), at any number of rows from 16 on; 520 rows of width 128: out_softmax_kernel behind it
                                                     (2, 64, 50, 40, 1), (2, 64, 50, 300, 0), (2, 128, 60, 128, 1), (3, 128, 60, 520, 2),
                                                     (1, 512, 64, 97, 0),
                                                     # n >= 256: width 512 on inc_tile_kernel (64-row tiles, px 8), width 128 on inc_cell_kernel with two
                                                     # row tiles; thin GEMM + softmax behind both
                                                     (2, 512, 256, 300, 1), (3, 96, 30, 260, 2), (1, 128, 40, 257, 1),
                                                     # n >= 256, widths of 256, 512, 1024: one launch per layer on 64 x 128 tiles with the state
                                                     # rows read through the pool slots (step_tile.hip): whole and ragged row tiles, px 8 and px 4 x py 2,
                                                     # 0 / 1 / 2 context variables; out_softmax_kernel from 512 rows on
                                                     (2, 256, 40, 320, 1), (3, 768, 50, 512, 0), (2, 512, 256, 1024, 1), (2, 512, 64, 449, 2),
                                                     # ... 128-row tiles (two or more 64-row tiles per CU), the last one ragged
                                                     (2, 1024, 64, 1030, 1),
                                                     # cfg5 topology: inc_cell_kernel with one row tile, inc_tile_kernel on 64-row tiles
                                                     (4, 1024, 64, 20, 2), (4, 1024, 64, 272, 2),
                                                     # wide vocabulary (V >= 1024): from 256 rows the plain gather + GEMM + gates_rows and the output
                                                     # projection through the big GEMM; below, inc_cell_kernel and the thin GEMM
                                                     (2, 128, 1100, 300, 1), (1, 64, 1500, 40, 0),
                                                     # zero-padded widths: inc_cell_kernel at 128, inc_tile_kernel at 256
                                                     (2, 100, 50, 30, 1), (2, 200, 50, 260, 1),
                                                     # deeper than four layers: the thin kernel (12 rows), inc_cell_kernel with two row tiles
                                                     (6, 128, 30, 12, 1), (6, 128, 30, 260, 1),
                                                     # vocabularies of trained models (len(chars) + 1: ragged, between 100 and 300), and one between 256
                                                     # and 1024: thin GEMM + softmax behind the cell and tile kernels (out_softmax_kernel ends at V = 256)
                                                     (2, 512, 230, 128, 1), (2, 512, 300, 300, 1), (2, 512, 700, 1024, 1), (2, 128, 230, 40, 1)])
def test_step_batch_parity(depth, width, voc, n, n_ctx):
    """S1 (rating.py:578-639): chained incremental steps through pool slots."""
    torch = _torch()
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.ensure_pool(2 * n)
    rng = np.random.default_rng(3)
    ctx = rng.integers(0, 200, (n, n_ctx))
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, n, np.float64)
    a, b = np.arange(n), np.arange(n, 2 * n)
    worst = 0.0
    for step in range(24):
        idx = rng.integers(0, voc, n)
        ref, st = O.step_batch(cfg, w64, idx, ctx, st)
        probs = lm.step_slots(idx, ctx, a, b).cpu().numpy()
        a, b = b, a
        worst = max(worst, np.abs(probs - ref).max())
    assert worst < 2e-5, worst
    pool = lm.pool_read(a)
    for k in range(2 * depth):
        assert np.abs(pool[:, k] - st[k]).max() < 1e-4


@pytest.mark.parametrize("depth,width,voc,n,env", [
    (2, 512, 256, 300, {"KL_INC_TILE": "0"}),        # inc_cell_kernel with two row tiles per workgroup instead of the tile kernel
    (2, 512, 256, 300, {"KL_INC_TILE": "0", "KL_INC_SMALL": "0"}),      # gather + [hi|lo|hi] GEMM with the cell as epilogue
    (2, 512, 256, 300, {"KL_TILE_ROWS": "128"}),     # 128-row tiles, the last one ragged
    (2, 512, 256, 600, {"KL_OUT_FUSED": "0"}),       # thin GEMM + softmax kernel instead of out_softmax_kernel
    (2, 512, 256, 100, {"KL_OUT_FUSED_MIN": "16"}),  # out_softmax_kernel below its default row count
    (2, 512, 256, 100, {"KL_INC_SMALL": "0"}),       # launch-per-layer thin kernels
    (2, 128, 60, 100, {"KL_INC_SMALL": "0"})])
def test_step_batch_paths_agree(monkeypatch, depth, width, voc, n, env):
    """The incremental step's kernels are chosen by row count and width; every alternative (KL_* switches of INTEGRATION.md)
    computes the same split-precision arithmetic, so chained steps through the pool must agree with the default path to a
    few f32 roundings -- the fall-backs stay exercised although the defaults no longer reach them at these shapes."""
    from ocrd_keraslm_amd.lib import hipabi
    rng = np.random.default_rng(5)
    ctx = rng.integers(0, 200, (n, 1))
    ids = rng.integers(1, voc, (12, n))
    out = {}
    for name, e in (("default", {}), ("alternative", env)):
        with monkeypatch.context() as mp:
            for k, v in e.items():
                mp.setenv(k, v)
            cfg, w, lm = make_model(depth, width, voc)      # (the switches are read when the handle is created)
        lm.set_weights(w, hipabi.KL_PREC_SPLIT)
        lm.ensure_pool(2 * n)
        a, b = np.arange(n), np.arange(n, 2 * n)
        for step in range(len(ids)):
            probs = lm.step_slots(ids[step], ctx, a, b).cpu().numpy()
            a, b = b, a
        out[name] = (probs, lm.pool_read(a))
    assert np.abs(out["default"][0] - out["alternative"][0]).max() < 5e-6
    assert np.abs(out["default"][1] - out["alternative"][1]).max() < 2e-5


@pytest.mark.parametrize("depth,width,voc,n", [(2, 512, 256, 128), (2, 512, 256, 1024), (2, 128, 60, 70), (4, 1024, 64, 1100)])
def test_step_batch_repeatable_bitwise(depth, width, voc, n):
    """No atomics and no order-dependent reductions in the incremental step: the same chained steps from the same pool give
    bitwise the same probabilities and states, run after run (a fragment or an index taken before it had landed would show
    here as a difference between runs)."""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.ensure_pool(2 * n)
    rng = np.random.default_rng(6)
    ctx = rng.integers(0, 200, (n, 1))
    ids = rng.integers(1, voc, (10, n))
    runs = []
    for rep in range(3):
        lm.pool.zero_()
        a, b = np.arange(n), np.arange(n, 2 * n)
        for step in range(len(ids)):
            probs = lm.step_slots(ids[step], ctx, a, b).cpu().numpy()
            a, b = b, a
        runs.append((probs, lm.pool_read(a)))
    for probs, pool in runs[1:]:
        assert np.array_equal(probs, runs[0][0])
        assert np.array_equal(pool, runs[0][1])


@pytest.mark.parametrize("depth,width,voc,n,n_ctx", [(2, 512, 256, 120, 1), (2, 512, 64, 700, 1), (3, 128, 40, 90, 2), (2, 1024, 64, 200, 1)])
def test_step_batch_beam_pattern(depth, width, voc, n, n_ctx):
    """The slots as a beam search uses them (rating.py:809-880): several hypotheses continue the SAME parent (slot_in with
    repeats), their new states go to free slots anywhere in the pool, parents that nobody continues are dropped -- against
    the f64 oracle, which is handed the gathered parent states."""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    n_slots = 3 * n + 5
    lm.ensure_pool(n_slots)
    lm.pool.zero_()
    rng = np.random.default_rng(21)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    ctx = rng.integers(0, 200, (n, n_ctx))
    live = rng.permutation(n_slots)[:n]                        # slots of the current hypotheses (all-zero states)
    st = O.zero_states(cfg, n, np.float64)                     # ... and the oracle's copy of them, row i <-> live[i]
    worst = 0.0
    for step in range(14):
        parents = np.sort(rng.integers(0, n, n))               # row indices into `live`: repeats, and rows left out
        slot_in = live[parents]
        free = np.setdiff1d(np.arange(n_slots), slot_in)       # (a new state must not overwrite a state read in this call)
        slot_out = rng.permutation(free)[:n]
        idx = rng.integers(0, voc, n)
        ref, st = O.step_batch(cfg, w64, idx, ctx, [s[parents] for s in st])
        probs = lm.step_slots(idx, ctx, slot_in, slot_out).cpu().numpy()
        worst = max(worst, np.abs(probs - ref).max())
        live = slot_out
    assert worst < 2e-5, worst
    pool = lm.pool_read(live)
    for k in range(2 * depth):
        assert np.abs(pool[:, k] - st[k]).max() < 1e-4


@pytest.mark.parametrize("depth,width,voc,n,n_ctx,env", [
    # kernel-argument indices (n <= 256, one context variable, widths 64 / 128 / multiples of 256): one and two row tiles
    (2, 512, 256, 120, 1, {}), (2, 512, 256, 30, 1, {}), (2, 512, 64, 256, 1, {}), (2, 128, 60, 128, 1, {}), (3, 256, 40, 7, 1, {}),
    (2, 64, 50, 200, 1, {}), (4, 1024, 64, 100, 1, {}), (2, 512, 256, 1, 1, {}),
    # the same shape through the copy of the packed indices (the fall-back of everything below)
    (2, 512, 256, 120, 1, {"KL_HOST_KERNARG": "0"}),
    # what the kernel-argument form does not take: more than 256 rows, 0 / 2 context variables, padded widths, width 1024 beyond 128 rows
    (2, 512, 64, 700, 1, {}), (3, 128, 40, 90, 2, {}), (2, 512, 64, 40, 0, {}), (2, 100, 50, 30, 1, {}), (2, 1024, 64, 200, 1, {})])
def test_step_host_beam_pattern(monkeypatch, depth, width, voc, n, n_ctx, env):
    """kl_step_batch_host (the step as rate_best / generate issue it, rating.py:809-826, 689-691): HOST index arrays, results
    delivered into host memory and awaited on the arrival word -- with the slots as a beam search uses them (repeated
    parents, new states anywhere in the pool), alternating between whole probability rows and the per-row target
    probability, with and without the head vectors of the new states; against the f64 oracle."""
    from ocrd_keraslm_amd.lib import hipabi
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        cfg, w, lm = make_model(depth, width, voc, n_ctx)      # (the switches are read when the handle is created)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    n_slots = 3 * n + 5
    lm.ensure_pool(n_slots)
    lm.pool.zero_()
    rng = np.random.default_rng(22)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    ctx = rng.integers(0, 200, (n, n_ctx))
    live = rng.permutation(n_slots)[:n]
    st = O.zero_states(cfg, n, np.float64)
    worst = worst_head = 0.0
    for step in range(12):
        parents = np.sort(rng.integers(0, n, n))
        slot_in = live[parents]
        free = np.setdiff1d(np.arange(n_slots), slot_in)
        slot_out = rng.permutation(free)[:n]
        idx = rng.integers(0, voc, n)
        ref, st = O.step_batch(cfg, w64, idx, ctx, [s[parents] for s in st])
        head_k = (0, depth, 1)[step % 3]
        if step % 2:
            target = rng.integers(0, voc, n)
            probs, heads = lm.step_host(idx, ctx, slot_in, slot_out, target=target, head_k=head_k)
            assert probs.shape == (n,)
            worst = max(worst, np.abs(probs - ref[np.arange(n), target]).max())
        else:
            probs, heads = lm.step_host(idx, ctx, slot_in, slot_out, head_k=head_k)
            assert probs.shape == (n, voc)
            worst = max(worst, np.abs(probs - ref).max())
        if head_k:
            assert heads.shape == (n, head_k, width)
            for k in range(head_k):
                worst_head = max(worst_head, np.abs(heads[:, k] - st[k]).max())
        else:
            assert heads is None
        live = slot_out
    assert worst < 2e-5, worst
    assert worst_head < 1e-4, worst_head
    pool = lm.pool_read(live)
    for k in range(2 * depth):
        assert np.abs(pool[:, k] - st[k]).max() < 1e-4
    # ... and interleaved with the device-pointer entry point on the same pool
    idx = rng.integers(0, voc, n)
    free = np.setdiff1d(np.arange(n_slots), live)
    out_a, out_b = free[:n], free[n:2 * n]
    p_dev = lm.step_slots(idx, ctx, live, out_a).cpu().numpy()
    p_host, _ = lm.step_host(idx, ctx, live, out_b)
    assert np.abs(p_dev - p_host).max() < 5e-6
    assert np.abs(lm.pool_read(out_a) - lm.pool_read(out_b)).max() < 2e-5


def test_state_dist2_matches_numpy():
    """kl_state_dist2 (history clustering, rating.py:887-916): squared distances between state entries of pool slots"""
    from ocrd_keraslm_amd.lib import hipabi
    torch = _torch()
    depth, width, voc, n = 2, 512, 64, 70
    cfg, w, lm = make_model(depth, width, voc)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.ensure_pool(2 * n)
    rng = np.random.default_rng(5)
    pool = rng.standard_normal((2 * n, 2 * depth, width)).astype(np.float32)
    lm.pool[:2 * n] = torch.from_numpy(pool).to(lm.pool.device)
    a, b = rng.integers(0, 2 * n, n), rng.integers(0, 2 * n, n)
    for k in range(2 * depth):
        out = lm.state_dist2(a, b, k).cpu().numpy()
        ref = ((pool[a, k].astype(np.float64) - pool[b, k]) ** 2).sum(axis=1)
        assert np.allclose(out, ref, rtol=1e-5), k
    with pytest.raises(Exception):
        lm.state_dist2(a, b, 2 * depth)          # no such state entry


def test_step_batch_peaked_model_split_precision():
    """The 1e-3 bar on a PEAKED model: weights scaled up until the softmax puts most of its mass on a few characters
    (what a trained model does; flat synthetic weights flatter bf16).  Split precision -- the rating default -- must hold
    the bar with room to spare; the plain-bf16 error on the same model is reported in the assertion message."""
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n = 2, 512, 256, 96
    cfg, w, lm = make_model(depth, width, voc, emb_std=1.0)
    for k in w:
        if k.startswith(("K", "U")):
            w[k] = (w[k] * 2.5).astype(np.float32)
    rng = np.random.default_rng(11)
    ctx = rng.integers(0, 200, (n, 1))
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    worst = {}
    for prec in (hipabi.KL_PREC_SPLIT, hipabi.KL_PREC_BF16):
        lm.set_weights(w, prec)
        lm.ensure_pool(2 * n)
        lm.pool.zero_()
        st = O.zero_states(cfg, n, np.float64)
        a, b = np.arange(n), np.arange(n, 2 * n)
        rng2 = np.random.default_rng(12)
        worst[prec], peak = 0.0, 0.0
        for step in range(96):
            idx = rng2.integers(1, voc, n)
            ref, st = O.step_batch(cfg, w64, idx, ctx, st)
            probs = lm.step_slots(idx, ctx, a, b).cpu().numpy()
            a, b = b, a
            worst[prec] = max(worst[prec], np.abs(probs - ref).max())
            peak = max(peak, float(np.median(ref.max(axis=1))))
    assert peak > 0.3, peak                      # the model really is peaked
    assert worst[hipabi.KL_PREC_SPLIT] < 1e-4, worst


def test_step_batch_bf16_within_1e3():
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc, n = 2, 512, 256, 64
    cfg, w, lm = make_model(depth, width, voc)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.ensure_pool(2 * n)
    rng = np.random.default_rng(3)
    ctx = rng.integers(0, 200, (n, 1))
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, n, np.float64)
    a, b = np.arange(n), np.arange(n, 2 * n)
    worst = 0.0
    for step in range(64):
        idx = rng.integers(1, voc, n)
        ref, st = O.step_batch(cfg, w64, idx, ctx, st)
        probs = lm.step_slots(idx, ctx, a, b).cpu().numpy()
        a, b = b, a
        worst = max(worst, np.abs(probs - ref).max())
    assert worst < 1e-3, worst


# The cases of test_forward_window_parity / test_forward_window_counter_handoff that exist to reach ONE arm of the split-precision
# scans' dispatch: (depth, width, B) -> row blocks per workgroup there.  Parity alone would also hold on another arm (or on the
# launch-per-step kernels, which take what the launcher refuses), so the conditions under which the case reaches its arm are
# asserted before any work: 256 compute units, the batch in one piece, and the launcher's arithmetic giving the arm.
SPLIT_ARM_CASES = {(4, 64, 257): 2, (4, 64, 769): 4, (4, 128, 129): 2, (4, 128, 385): 4, (4, 256, 65): 2, (4, 256, 193): 4,
                   (4, 512, 33): 2, (1, 1024, 65): 2, (1, 1024, 193): 4}


def _check_split_arm(lm, depth, width, B):
    want = SPLIT_ARM_CASES.get((depth, width, B))
    if want is None:
        return
    cus = lm.torch.cuda.get_device_properties(lm.device).multi_processor_count
    assert cus >= 256, "this case was chosen for 256 compute units (the scans' grid plan clamps there); %d here" % cus
    assert lm.pwidth == width and lm._rating_groups(B) == [(0, B)]
    n_rb = (B + 15) // 16
    if width == 1024:      # one layer per launch; more than two row blocks (not the eight-unit scan), at most sixteen
        assert 2 < n_rb <= 16
    g = min(256 // ((1 if width == 1024 else depth) * (width // 16)), n_rb)
    assert -(-n_rb // g) == want


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", [(2, 64, 50, 1, 32, 1), (2, 128, 60, 3, 16, 1),
                                                       (1, 128, 40, 1, 64, 1), (2, 512, 256, 2, 24, 1),
                                                       (3, 64, 30, 2, 7, 2),
                                                       # persistent split-precision scan: row blocks > workgroups, 3 layers,
                                                       # the cfg2 rating window
                                                       (3, 256, 30, 40, 9, 2), (2, 512, 64, 200, 5, 1), (2, 512, 256, 1, 256, 1),
                                                       # cfg5 topology (two layers per launch, eight units per workgroup); three
                                                       # layers (a pair and a single one), two row blocks, one layer
                                                       (4, 1024, 64, 2, 6, 2), (3, 1024, 40, 20, 5, 1), (1, 1024, 30, 1, 9, 0),
                                                       # ... more than two row blocks: layer by layer
                                                       (2, 1024, 40, 40, 4, 1),
                                                       # zero-padded widths
                                                       (2, 100, 50, 3, 12, 1), (1, 33, 20, 20, 5, 0),
                                                       # deeper than four layers (launch-per-step kernels, packs of four layers)
                                                       (6, 128, 30, 5, 9, 1), (9, 64, 20, 2, 6, 2),
                                                       # more streams than the persistent split-precision scan takes in one call
                                                       # (256 at depth 2 / width 512, 128 at depth 3): groups of streams
                                                       (2, 512, 64, 300, 4, 1), (3, 512, 40, 270, 3, 2),
                                                       # every row-blocks-per-workgroup arm of the split-precision scans'
                                                       # dispatch (the <width / 32, 2 or 4> instantiations), at the smallest
                                                       # stream count that reaches it.  The counts ASSUME 256 CUs (on fewer the
                                                       # arms move): kl_launch_scan_fwd_split has row groups g = 256 / (depth *
                                                       # width / 16), row blocks n = ceil(B / 16) and ceil(n / g) of them per
                                                       # workgroup; HipLM._rating_groups keeps B <= 64 g streams in one piece.
                                                       #   width 64, depth 4: g = 16 (one piece up to 1024 streams);
                                                       #     B = 257 -> n = 17 -> 2;  B = 769 -> n = 49 -> 4
                                                       (4, 64, 30, 257, 3, 1), (4, 64, 30, 769, 3, 1),
                                                       #   width 128, depth 4: g = 8 (512);  B = 129 -> 9 -> 2;  385 -> 25 -> 4
                                                       (4, 128, 30, 129, 3, 1), (4, 128, 30, 385, 3, 1),
                                                       #   width 256, depth 4: g = 4 (256);  B = 65 -> 5 -> 2;  193 -> 13 -> 4
                                                       (4, 256, 30, 65, 3, 1), (4, 256, 30, 193, 3, 1),
                                                       #   width 512, depth 4: g = 2 (128);  B = 33 -> 3 -> 2  (4: the 200-stream
                                                       #   case above, depth 2: g = 4, n = 13)
                                                       (4, 512, 30, 33, 3, 1),
                                                       #   width 1024, one layer per launch without input weights: g = 256 / 64
                                                       #   = 4 (256); more than two row blocks, so not the eight-unit scan, and at
                                                       #   most 16, fwd_split_layers' limit;  B = 65 -> 5 -> 2;  193 -> 13 -> 4
                                                       (1, 1024, 30, 65, 3, 1), (1, 1024, 30, 193, 3, 1)])
def test_forward_window_parity(depth, width, voc, B, T, n_ctx):
    """F1-F6 stateful windows (rating.py:490, 516): two consecutive windows carry state."""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx)
    _check_split_arm(lm, depth, width, B)
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.reset_states(B)
    rng = np.random.default_rng(9)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, B, np.float64)
    for win in range(2):
        idx = rng.integers(0, voc, (B, T))
        ctx = rng.integers(0, 200, (B, 1, n_ctx)).repeat(T, axis=1)
        tgt = rng.integers(0, voc, (B, T))
        tgt[:, -2:] = -1
        ref, st, _ = O.forward_window(cfg, w64, idx, ctx, st)
        lm.loss_acc.zero_()
        probs = lm.forward_window(idx, ctx, tgt).cpu().numpy()
        assert np.abs(probs - ref).max() < 2e-5
        ce, acc, _ = O.crossentropy(ref, tgt)
        l, a, _ = lm.read_loss()
        assert abs(l - ce) < 1e-4 * max(1, ce)
        assert abs(a - acc) < 1e-6
    states = lm.get_states()
    for k in range(2 * depth):
        assert np.abs(states[:, k] - st[k]).max() < 1e-4


def test_forward_window_width_1024_layer_by_layer(monkeypatch):
    """width 1024, few streams, with the two-layer launches switched off (KL_SPLIT8=0): one persistent scan per layer"""
    monkeypatch.setenv("KL_SPLIT8", "0")
    test_forward_window_parity(4, 1024, 64, 2, 6, 2)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", [(3, 256, 30, 40, 9, 2), (2, 512, 256, 1, 64, 1),
                                                       # two and four row blocks per workgroup (the arithmetic: see the
                                                       # cases of test_forward_window_parity; 256 CUs assumed)
                                                       (4, 64, 30, 257, 3, 1), (4, 64, 30, 769, 3, 1),
                                                       (4, 256, 30, 65, 3, 1), (4, 256, 30, 193, 3, 1)])
def test_forward_window_counter_handoff(monkeypatch, depth, width, voc, B, T, n_ctx):
    """the split-precision scan with its counter hand-off (KL_SPLIT_SENTINEL=0; the default hands over by data sentinels)"""
    monkeypatch.setenv("KL_SPLIT_SENTINEL", "0")
    test_forward_window_parity(depth, width, voc, B, T, n_ctx)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", [(2, 128, 40, 20, 9, 1), (2, 512, 64, 512, 4, 1), (2, 512, 64, 1024, 3, 1),
                                                       (3, 100, 30, 5, 7, 2), (2, 1024, 40, 48, 4, 1), (6, 128, 30, 24, 5, 1)])
def test_validation_windows_bf16(depth, width, voc, B, T, n_ctx):
    """forward_window in bf16 precision (validation after each epoch, rating.py:300-306) takes the training forward --
    the persistent scans -- without the backward: loss, accuracy, probabilities and carried state against the oracle,
    over two consecutive windows."""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.reset_states(B)
    rng = np.random.default_rng(5)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, B, np.float64)
    for win in range(2):
        idx = rng.integers(0, voc, (B, T))
        ctx = rng.integers(0, 200, (B, 1, n_ctx)).repeat(T, axis=1)
        tgt = rng.integers(0, voc, (B, T))
        tgt[:, -1:] = -1
        ref, st, _ = O.forward_window(cfg, w64, idx, ctx, st)
        lm.loss_acc.zero_()
        probs = lm.forward_window(idx, ctx, tgt).cpu().numpy()
        assert np.abs(probs - ref).max() < 1e-2, np.abs(probs - ref).max()
        ce, acc, _ = O.crossentropy(ref, tgt)
        l, a, _ = lm.read_loss()
        assert abs(l - ce) < 2e-2 * max(1, ce), (l, ce)
        assert abs(a - acc) < 2e-2, (a, acc)
        got = lm.get_states()
        for k in range(2 * depth):
            assert np.abs(got[:, k] - st[k]).max() < 3e-2
        st = [got[:, k].astype(np.float64) for k in range(2 * depth)]      # (carry the engine's bf16-rounded state on)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,use_masks", [(1, 64, 40, 2, 8, 1, False), (2, 64, 50, 4, 16, 1, True),
                                                                 (2, 128, 70, 8, 32, 1, True), (3, 64, 30, 3, 8, 2, True),
                                                                 (2, 64, 50, 1, 5, 1, False),
                                                                 # shapes served by the persistent scans (W in 128/256/512)
                                                                 (2, 128, 70, 40, 12, 1, True), (3, 128, 30, 20, 6, 2, True),
                                                                 (1, 256, 40, 5, 9, 1, False), (2, 512, 64, 100, 6, 1, True),
                                                                 (2, 512, 256, 64, 16, 1, True),
                                                                 # many row blocks: layer-sequential backward with wide workgroups
                                                                 (2, 512, 64, 144, 6, 1, True), (2, 256, 40, 272, 4, 1, True),
                                                                 (3, 256, 30, 176, 5, 1, True),
                                                                 # cfg5 topology: depth 4, width 1024, two context variables
                                                                 (4, 1024, 64, 4, 4, 2, True),
                                                                 # width 1024: one thin persistent scan per layer (several row blocks, ragged last one)
                                                                 (4, 1024, 64, 48, 5, 2, True), (2, 1024, 40, 150, 3, 1, False), (2, 1024, 40, 640, 2, 1, True),
                                                                 # any width: hidden units zero-padded to the next width the persistent scans serve
                                                                 (2, 100, 50, 24, 9, 1, True), (3, 40, 30, 5, 7, 2, True), (2, 300, 64, 144, 4, 1, True),
                                                                 (1, 7, 20, 3, 6, 1, False),
                                                                 # deeper than the fused scans' four layers: one persistent scan per layer
                                                                 (6, 128, 30, 24, 5, 1, True), (5, 512, 40, 144, 3, 1, True), (7, 64, 20, 3, 4, 2, False),
                                                                 # wider than 1024: padded to a multiple of 32, launch-per-step kernels
                                                                 (2, 1100, 30, 4, 3, 1, True),
                                                                 # vocabularies of trained models: the fused output layer (V = 256, 8192 rows) in front of the
                                                                 # first-generation backward scan; V = 230 padded to 256 columns at widths 512, 1024 and 128
                                                                 (2, 512, 256, 512, 16, 1, True), (2, 512, 230, 144, 6, 1, True), (2, 1024, 230, 150, 3, 1, False),
                                                                 (2, 128, 230, 40, 12, 1, True)])
def test_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks):
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,use_masks", [(2, 512, 64, 144, 6, 1, True), (2, 512, 64, 40, 7, 2, True),
                                                                 (3, 256, 30, 176, 5, 1, True), (1, 256, 40, 8, 9, 1, False),
                                                                 (2, 256, 40, 272, 4, 1, False),
                                                                 # the shape class that takes this path by default
                                                                 (2, 512, 64, 512, 4, 1, True),
                                                                 # several row blocks per workgroup: sentinel backward, prefetched
                                                                 # tiles, late stores (even and uneven visits; width 256)
                                                                 (2, 512, 64, 1024, 3, 1, True), (2, 512, 64, 1040, 3, 1, True),
                                                                 (2, 256, 40, 1056, 3, 1, True), (2, 512, 64, 2560, 2, 1, True)])
def test_train_window_wide_forward(monkeypatch, depth, width, voc, B, T, n_ctx, use_masks):
    """Layer-sequential forward with 64-unit workgroups (table look-ups fused into the
    layer-0 scan, transposed outputs written by the scans): forced on for small shapes."""
    monkeypatch.setenv("KL_WIDE_FWD_MIN", "1")
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,use_masks,env", [
    (2, 512, 64, 1024, 4, 1, True, {}),                        # 16-row phases, two per workgroup and step
    (2, 512, 64, 2048, 3, 1, True, {}),                        # 16-row phases, four per workgroup
    (2, 512, 64, 2048, 4, 1, True, {"KL_SCAN2_ROWS": "32"}),   # 32-row phases, two per workgroup
    (3, 512, 40, 3072, 3, 1, True, {}),                        # 32-row phases, three per workgroup; three layers
    (2, 512, 64, 1536, 5, 0, False, {}),                       # three 16-row phases; no context variable, no dropout
    (1, 512, 64, 1024, 3, 1, False, {}),                       # one layer: layer-sequential backward because of the G layout
    (2, 512, 64, 2048, 3, 1, True, {"KL_SCAN2_PF": "1"}),      # next tile requested behind the MFMA phase
    (2, 512, 64, 2048, 5, 1, True, {"KL_SCAN2_PF": "2"}),      # tiles requested two phases ahead (four phases per workgroup)
    (2, 512, 64, 3072, 4, 1, True, {"KL_SCAN2_PF": "2"}),      # ... with three 32-row phases forward, six blocks backward
    (2, 512, 64, 1024, 4, 1, True, {"KL_SCAN2_PF": "2"}),      # ... with two phases: every request too early (the re-fetch path)
    # six blocks per step: the 8-wave backward scan with the tile through registers two blocks ahead (lstm_scan_bwd_regtile_kernel);
    # KL_REGTILE=0 / KL_RT_LOCAL=0: the 16-wave kernel / write-through publishes at the same shape
    (2, 512, 64, 3072, 5, 1, True, {}), (2, 512, 64, 3072, 7, 1, False, {}), (3, 512, 40, 3072, 4, 0, True, {}),
    (2, 512, 64, 3072, 5, 1, True, {"KL_REGTILE": "0"}), (2, 512, 64, 3072, 4, 1, True, {"KL_RT_LOCAL": "0"}),
    # several context variables: layer 0's gate inputs gathered into bf16 P rows in front of the scan (kl_launch_p_gather_il)
    (2, 512, 64, 1024, 4, 2, True, {}), (2, 512, 64, 3072, 3, 3, False, {}),
    # vocabularies of trained models (rows and V of tests/test_output_layer_gpu.py, whose return codes show which launcher takes them):
    (2, 512, 256, 1024, 8, 1, True, {}),                       # logits_ce_ws + dh_ws
    (2, 512, 230, 1024, 4, 1, True, {}),                       # dh_ws with pad columns behind the strided softmax (Vp = 256 != V)
    (2, 512, 200, 1024, 4, 1, True, {}),                       # Vp = 224
    (2, 512, 300, 1024, 4, 1, True, {}),                       # V > 256; segment sums and the layer-0 sum table at their largest
    (2, 512, 330, 1024, 4, 1, True, {})])                      # both past their cut-offs: one-hot products, the 16-wave scan's table mode
def test_train_window_scan2(monkeypatch, depth, width, voc, B, T, n_ctx, use_masks, env):
    """Second-generation wide scans (lstm_scan2.hip: no K split in the forward scan, 32-row phases, double-buffered
    tiles, counted waits, gate-interleaved G): gradients, loss and carried state against the f64 oracle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # (32-row phases: the eight-wave forward scan of lstm_scan_fwd8.hip, see test_train_window_fwd8; else the 16-wave one)
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks, want_kernel=("lstm_scan_fwd_wide2_kernel", "lstm_scan_fwd8_kernel"))


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,use_masks,env,want", [
    (2, 512, 64, 3072, 9, 1, True, {}, "lstm_scan_fwd8_kernel"),                       # three 32-row phases per step, tiles two phases ahead; the ring goes round
    (3, 512, 40, 3072, 4, 0, False, {}, "lstm_scan_fwd8_kernel"),                      # three layers, no context variable, no dropout
    (2, 512, 64, 2048, 6, 2, True, {"KL_SCAN2_ROWS": "32"}, "lstm_scan_fwd8_kernel"),  # two phases per step: tiles one phase ahead; two contexts
    (2, 512, 64, 3072, 5, 1, True, {"KL_FWD8_LOCAL": "0", "KL_FWD8_PF": "0"}, "lstm_scan_fwd8_kernel"),   # write-through publishes; tiles one ahead at the top
    (2, 512, 64, 3072, 5, 1, True, {"KL_FWD8_PF": "2"}, "lstm_scan_fwd8_kernel"),      # two ahead at the top: every request too early (the re-fetch path)
    # the counter form (no workgroup barrier in the loop: landed / released / arrival counters, last-arriver publish, strips two phases late)
    (2, 512, 64, 2048, 6, 2, True, {"KL_FWD8_LS": "0", "KL_SCAN2_ROWS": "32"}, "lstm_scan_fwd8_kernel")])
def test_train_window_fwd8(monkeypatch, depth, width, voc, B, T, n_ctx, use_masks, env, want):
    """The eight-wave forward scan (lstm_scan_fwd8.hip, KL_FWD8=1: two unit tiles per wave, no workgroup barrier, tile ring with
    LDS counters, last-arriver publish, layer 0's gate inputs gathered into P rows): gradients, loss and carried state
    against the f64 oracle, with the switches that move its tile requests and its publish path."""
    monkeypatch.setenv("KL_FWD8", "2")      # (also for layer 0, which by default stays on the 16-wave scan's table mode)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks, want_kernel=want)


@pytest.mark.parametrize("depth,B,T,use_masks,env", [
    (1, 3072, 6, False, {}),                                   # one layer: the traced launch IS layer 0's -- three phases per step
    (2, 2048, 9, True, {"KL_SCAN2_ROWS": "32"}),               # two phases per step; the ring of row numbers goes round four times
    (3, 3072, 3, True, {})])                                   # a window as short as the look-ahead of the row numbers
def test_train_window_fwd8_table_mode(monkeypatch, depth, B, T, use_masks, env):
    """Layer 0 on the eight-wave forward scan (round 4; KL_FWD8_TAB=0 switches it off): its gate-input rows are gathered from the table of ALL (character,
    context value) sums, the row numbers of a phase brought into LDS three phases ahead -- gradients, loss and carried state
    against the f64 oracle with 200 context values in play."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_train_window_gradients(depth, 512, 64, B, T, 1, use_masks, want_kernel="lstm_scan_fwd8_kernel")


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,ctx_values,want", [
    (2, 512, 20, 3072, 4, 2, 3, "lstm_scan_fwd_wide2_kernel"),      # 12288 positions onto 20 characters / 3 values per context
    (2, 512, 20, 1024, 5, 1, 2, "lstm_scan_fwd_wide2_kernel"),
    (2, 128, 12, 96, 9, 2, 4, None), (4, 1024, 20, 128, 3, 2, 3, None)])
def test_embedding_gradients_heavy_repetition(depth, width, voc, B, T, n_ctx, ctx_values, want):
    """The scatter of layer 0's input gradient into the embedding tables (rating.py:103-125) and the tied output
    layer's term (rating.py:155-168) with every table row hit hundreds of times: few characters, few context values,
    many streams -- duplicates must be SUMMED (one-hot products / segment sums), compared on the back-propagated
    part alone (tests/gradcheck.py)."""
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, True, want_kernel=(want, "lstm_scan_fwd8_kernel") if want else None, ctx_values=ctx_values)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,use_masks,env", [
    (2, 1024, 40, 16, 5, 1, True, {}),                          # one row block, one workgroup per column group
    (4, 1024, 64, 48, 4, 2, True, {}),                          # three row groups; the cfg5 topology
    (2, 1024, 40, 40, 4, 1, False, {}),                         # ragged last row block (no prefetch: partial tiles)
    (2, 1024, 40, 144, 5, 1, True, {}),                         # nine row blocks on eight row groups: two visits, uneven; prefetched tiles
    (2, 1024, 40, 512, 3, 1, True, {}),                         # four row blocks per workgroup (the cfg5 bench shape's plan)
    (1, 1024, 40, 1024, 2, 0, False, {}),                       # eight per workgroup; one layer, no context, no dropout
    (2, 1024, 40, 17, 1, 1, False, {}),                         # a single step (no tile at all), ragged second row block
    (2, 1024, 40, 272, 2, 1, True, {}),                         # 17 row blocks on 8 row groups: three visits for one group, two for the others
    (2, 1024, 40, 328, 3, 1, True, {}),                         # ... ragged (328 = 20.5 blocks): no tiles requested ahead
    (2, 1024, 40, 256, 4, 1, True, {"KL_W32_LOCAL": "1"})])     # publishes through the XCD's own L2
def test_train_window_width_1024_scans(monkeypatch, depth, width, voc, B, T, n_ctx, use_masks, env):
    """Width 1024: the eight-wave scans of lstm_scan_w32.hip (32 units per workgroup, the tile through LDS, data sentinels),
    forced on from one row block: gradients, loss and carried state against the f64 oracle."""
    monkeypatch.setenv("KL_W32_MIN_RB", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks, want_kernel="lstm_scan_bwd_w32_kernel")


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,use_masks,env,want", [
    (2, 128, 70, 40, 12, 1, True, {"KL_W128_MIN": "1"}, "multi"),      # three row blocks, the last one half full; both layers in one launch
    (3, 128, 30, 20, 6, 2, True, {"KL_W128_MIN": "1"}, "multi"),       # three layers, two context variables
    (1, 128, 40, 24, 7, 1, False, {"KL_W128_MIN": "1"}, "single"),     # one layer, no dropout
    (2, 100, 50, 24, 9, 1, True, {"KL_W128_MIN": "1"}, "multi"),       # width 100 zero-padded to 128
    (2, 128, 50, 600, 5, 1, True, {}, "multi"),                        # the default path from 512 streams
    (2, 128, 70, 40, 12, 1, True, {"KL_W128_MIN": "1", "KL_W128_FUSE": "0"}, "single"),     # input side / gradient from above by products over all steps
    (4, 128, 30, 33, 5, 1, True, {"KL_W128_MIN": "1"}, "multi"),       # four layers, each polling the rows of its neighbour
    (2, 128, 70, 40, 12, 1, True, {"KL_W128_MIN": "1", "KL_W128_MULTI": "0"}, "single"),    # one launch per layer, contractions inside the scans
    (2, 128, 50, 1024, 24, 1, True, {}, "multi"),                      # 2 x 64 workgroups in one launch
    (2, 128, 50, 2064, 3, 1, True, {}, "single"),                      # 2 x 129 row blocks do not fit 256 CUs: one launch per layer
    (3, 128, 30, 20, 6, 1, True, {"KL_W128_MIN": "1", "KL_SENTINEL_ROLL": "0"}, "multi"),   # every polled row a sentinel from the start (default: rolling)
    (2, 128, 30, 20, 2, 1, True, {"KL_W128_MIN": "1"}, "multi"),       # two steps: nothing to roll
    (3, 128, 30, 17, 1, 1, True, {}, "multi"),                         # a single step, ragged second row block
    (2, 128, 40, 40, 6, 0, True, {"KL_W128_MIN": "1"}, "multi"),       # no context variable: layer 0 from the embedding table alone
    (2, 128, 40, 24, 5, 3, True, {"KL_W128_MIN": "1"}, "multi"),       # three context variables: layer 0's gate inputs gathered into rows first
    (1, 128, 40, 24, 7, 1, False, {"KL_W128_MIN": "1", "KL_W128_TABLES": "0"}, "single"),    # ... also with one
    (2, 128, 70, 8, 32, 1, True, {}, "multi"),                         # the default at any stream count since round 4
    (2, 128, 70, 40, 12, 1, True, {"KL_W128": "0"}, "thin"),           # the thin fused scans (16-unit workgroups exchanging state) stay reachable
    # vocabularies of trained models: seven / eight k-steps of the dH contraction, characters on all 16 waves
    (2, 128, 230, 600, 5, 1, True, {}, "multi"), (2, 128, 256, 600, 5, 1, True, {}, "multi"), (2, 128, 200, 600, 5, 1, True, {}, "multi")])
def test_train_window_width_128_scans(monkeypatch, depth, width, voc, B, T, n_ctx, use_masks, env, want):
    """Width 128 (the reference's published model size): the scans of lstm_scan_w128.hip -- a workgroup per 16-row block of
    streams with all hidden units of a layer, no hand-off of state between workgroups; the layers above the first contract
    their inputs (forward) and the gradient from above (backward) inside the scan, and where all layers' workgroups fit the
    CUs at once they run in ONE launch, a layer polling the rows its neighbour publishes: gradients, loss and carried state
    against the f64 oracle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks,
                                 want_kernel={"multi": "lstm_scan_bwd_w128_multi_kernel", "single": "lstm_scan_bwd_w128_kernel",
                                              "thin": "lstm_scan_bwd_kernel"}[want])


@pytest.mark.parametrize("B,T", [(144, 4), (512, 3)])
def test_width_1024_scans_consecutive_windows(monkeypatch, B, T):
    """the width-1024 scans over consecutive windows (sentinels re-armed per window, carried state, replayed graph),
    forced on from one row block: uneven visits with prefetched tiles / four row blocks per workgroup"""
    monkeypatch.setenv("KL_W32_MIN_RB", "1")
    test_train_consecutive_windows_reuse_buffers(2, 1024, 40, B, T)


def test_width_128_scans_consecutive_windows(monkeypatch):
    """the width-128 scans, all layers in one launch, over consecutive windows: the rows a layer polls are sentinels again
    before every window (carried state, replayed graph)"""
    monkeypatch.setenv("KL_W128_MIN", "1")
    test_train_consecutive_windows_reuse_buffers(3, 128, 40, 72, 6)


def test_flag_handoff_survives_changing_shapes():
    """The backward scan's flag hand-off keeps ONE set of flag words and an epoch per engine: windows of changing size and
    length on the same engine (hipGraph replays in between) must give what a fresh engine gives for the same inputs --
    a word left by an earlier, longer window must never pass for one of the current launch."""
    from ocrd_keraslm_amd.lib import hipabi
    depth, width, voc = 2, 512, 64
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    rng = np.random.default_rng(33)
    for B, T in [(1536, 6), (2048, 3), (1536, 3), (3072, 4), (1536, 6)]:
        idx = rng.integers(0, voc, (B, T))
        ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
        tgt = rng.integers(0, voc, (B, T))
        states = (rng.standard_normal((B, 2 * depth, width)) * 0.1).astype(np.float32)
        got = []
        for engine in (lm, None):
            if engine is None:
                _cfg, _w, engine = make_model(depth, width, voc, 1, emb_std=0.3)
                engine.set_weights(w, hipabi.KL_PREC_BF16)
            for _rep in range(2):                      # (the second pass replays the captured graph)
                engine.reset_states(B)
                engine.set_states(states)
                engine.loss_acc.zero_()
                engine.train_window(idx, ctx, tgt, None)
            got.append((engine.read_loss(), engine.get_grads()))
        (l0, g0), (l1, g1) = got
        assert abs(l0[0] - l1[0]) < 1e-4 * max(1.0, abs(l1[0])), (B, T, l0, l1)
        for name in g1:
            scale = np.abs(g1[name]).max() + 1e-12
            assert np.abs(g0[name] - g1[name]).max() / scale < 2e-3, (B, T, name)


@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx", [(6, 128, 30, 5, 7, 1), (2, 128, 40, 20, 9, 1)])
def test_train_window_launch_per_step_path(monkeypatch, depth, width, voc, B, T, n_ctx):
    """KL_SCAN=0: the launch-per-step kernels (the fallback of every shape the scans do not cover), incl. more
    layers than one launch packs"""
    monkeypatch.setenv("KL_SCAN", "0")
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, True)


def check_train_window_gradients(depth, width, voc, B, T, n_ctx, use_masks, want_kernel=None, ctx_values=200):
    """B1-B7 + F7: gradients of mean CE + regularisers vs the f64 oracle.  The HIP
    path computes in bf16 with f32 accumulation: relative error of each gradient
    array is held to 3e-2 of its max-norm (bf16 has 8 mantissa bits) and 1.5e-2 in relative L2 -- for the
    embedding tables E / Ctx* both of the total and of the back-propagated part alone (tests/gradcheck.py: the
    regularisers' analytic part would otherwise hide the tied output layer's and the scatter's contributions)."""
    from ocrd_keraslm_amd.lib import hipabi
    from tests.gradcheck import assert_gradients, small_ctx_tables
    cfg, w, lm = make_model(depth, width, voc, n_ctx, emb_std=0.3)
    w = small_ctx_tables(w)      # (so that f32 resolves the context tables' back-propagated gradient beside the regularisers')
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.reset_states(B)
    rng = np.random.default_rng(21)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    idx = rng.integers(0, voc, (B, T))
    ctx = rng.integers(0, ctx_values, (B, 1, n_ctx)).repeat(T, axis=1)
    tgt = rng.integers(0, voc, (B, T))
    if T > 4:
        tgt[0, -2:] = -1
    st0 = [rng.standard_normal((B, width)) * 0.1 for _ in range(2 * depth)]
    states = np.stack(st0, axis=1).astype(np.float32)   # [B][2L][W]
    import torch
    lm.set_states(states)
    masks = lm.draw_dropout_masks(B) if use_masks else None
    omasks = [None] + [masks[l].astype(np.float64) for l in range(1, depth)] if use_masks else None
    ref_p, ref_st, cache = O.forward_window(cfg, w64, idx, ctx, [s.astype(np.float64) for s in st0], omasks,
                                            keep_cache=True)
    ce, acc, _ = O.crossentropy(ref_p, tgt)
    reg = O.regularisers(cfg, w64)
    g_data = O.backward_window(cfg, w64, idx, ctx, tgt, ref_p, cache, omasks, with_regularisers=False)
    lm.loss_acc.zero_()
    if want_kernel:
        hipabi.check(lm.lib.kl_trace_enable(lm.handle, 1))
    lm.train_window(idx, ctx, tgt, masks)
    if want_kernel:      # the shape must really have taken the kernel under test
        torch.cuda.synchronize()
        names = [lm.lib.kl_trace_kernel_name(lm.handle, k).decode() for k in (0, 1)]
        hipabi.check(lm.lib.kl_trace_enable(lm.handle, 0))
        wanted = (want_kernel,) if isinstance(want_kernel, str) else tuple(want_kernel)
        assert any(k in names for k in wanted), names
    l, a, r = lm.read_loss()
    assert abs(l - ce) < 2e-2 * max(1.0, ce), (l, ce)
    # (the regularisers' value: 1e-5 relative, the bound tests/test_table_grads_gpu.py holds the same kernels to on single tables,
    #  where they land at 0.03 of it or below)
    from tests import table_grads as TG
    assert abs(r - reg) <= TG.REL * abs(reg), (r, reg)
    # accuracy: a position whose two largest reference logits are closer than 1e-3 may fall either way -- the difference is
    # bounded by the share of those positions (from the reference alone) plus one position
    top2 = np.log(np.partition(ref_p, voc - 2, axis=-1)[..., voc - 2:])
    close = float(((top2[..., 1] - top2[..., 0]) < 1e-3).mean())
    print("accuracy %.6f, oracle %.6f, share of close positions %.6f, one position %.6f" % (a, acc, close, 1.0 / (B * T)))
    assert abs(a - acc) <= close + 1.0 / (B * T), (a, acc, close)
    # (the max-norm bound alone would let a term that is off by a few per cent in a small block -- bias, context table --
    # pass; the relative L2 error of every array is 0.3-0.6 % from bf16 rounding alone (tools/diag_scan2_err.py), so
    # 1.5 % separates rounding from a wrong term)
    assert_gradients(lm.layout, lm.get_grads(), g_data, O.regulariser_grads(cfg, w64), rel=1.5e-2, maxn=3e-2,
                     where=(depth, width, voc, B, T, n_ctx))
    st_got = lm.get_states()
    for k in range(2 * depth):
        assert np.abs(st_got[:, k] - ref_st[k]).max() < 2e-2
    # what the scans left in the workspace, the checks without tolerance (tests/window_ref.py): no NaN / Inf halfword in H, G, dZ
    # (a sentinel that survived), the engine's own dummy streams' dZ exactly zero, block 0 = the carried-in state, block T =
    # the carried-out state.  (Stream groups: the workspace holds the last group.)
    from tests.window_ref import exact_checks, read_window
    win = read_window(lm)
    first, n = win["info"]["first"], win["info"]["n"]
    exact_checks(win, states[first:first + n], st_got[first:first + n], n, where=(depth, width, voc, B, T, n_ctx))
    # ... and the weight-gradient stage held to the f64 products of those arrays (tests/window_grads.py), where the window ran as
    # ONE group on the batch as given.  Layer 0's character rows are left to tests/test_window_grads_gpu.py (their allowance
    # for sums near a rounding boundary: see the note in tests/window_grads.py).
    info = win["info"]
    if (info["groups"], info["B"], info["first"], info["n"]) == (1, B, 0, B):
        from tests import window_grads as WG
        from tests.window_ref import read_window_padded
        report, err = WG.check_window_grads(read_window_padded(lm), idx, ctx, lm.params.detach().cpu().numpy(),
                                            lm.grads.detach().cpu().numpy(), lm.layout, width=lm.width,
                                            where=(depth, width, voc, B, T, n_ctx), raise_=False)
        print("weight gradients against the products of the window's arrays:", WG.route_text(win["view"]), "|", WG.ratio_line(report, depth))
        if err is not None and err.parts - {WG.CHARACTERS}:
            raise WG.GradMismatch([f for f in err.failures if f[0] != WG.CHARACTERS], (depth, width, voc, B, T, n_ctx))
        # ... and the tables' gradients (tests/table_grads.py).  These tables are not regulariser-neutral, so the f32 totals do
        # not resolve the back-propagated parts: the precondition and the ratios are reported, the exact checks asserted
        # (dlogits zero beyond the vocabulary, dE zero in the padded columns); tests/test_table_grads_gpu.py is the assertion.
        treport, terr = TG.check_table_grads(read_window_padded(lm), idx, ctx if n_ctx else None, lm.params.detach().cpu().numpy(),
                                             lm.grads.detach().cpu().numpy(), lm.layout, width=lm.width,
                                             where=(depth, width, voc, B, T, n_ctx), raise_=False, precondition=False)
        print("table gradients:", TG.route_text(win["view"]), "|", TG.ratio_line(treport), "| precondition", TG.precondition_line(treport))
        inexact = [f for f in (terr.failures if terr is not None else []) if "non-zero where exactly zero is due" in f]
        if inexact:
            raise WG.GradMismatch(inexact, (depth, width, voc, B, T, n_ctx))


def test_adam_step_matches_oracle():
    from ocrd_keraslm_amd.lib import hipabi
    import torch
    cfg, w, lm = make_model(1, 64, 20)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.ensure_training_buffers()
    rng = np.random.default_rng(5)
    g = (rng.standard_normal(lm.n_params) * 2).astype(np.float32)
    opt = O.Adam(cfg)
    wo = {k: v.copy() for k, v in w.items()}
    for it in range(3):
        lm.grads.copy_(torch.from_numpy(g))
        lm.adam_step()
        gd = {name: g[off:off + rows * cols].reshape(wo[name].shape) for name, off, rows, cols in lm.layout}
        opt.step(wo, gd)
    got = lm.get_weights()
    for k in wo:
        assert np.abs(got[k] - wo[k]).max() < 1e-6, k


@pytest.mark.parametrize("depth,width,voc,B,T", [(2, 128, 50, 20, 12), (2, 512, 64, 40, 8), (2, 512, 64, 144, 5), (3, 1024, 40, 40, 4)])
def test_train_consecutive_windows_reuse_buffers(depth, width, voc, B, T):
    """The persistent scans hand data between workgroups through buffers that are
    re-used by every window: three consecutive windows (carried state, fresh inputs)
    must each match the oracle -- a stale cached line from the previous window would
    show up as a wrong loss / state / gradient here."""
    import torch
    from tests.gradcheck import assert_gradients
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.reset_states(B)
    rng = np.random.default_rng(33)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, B, np.float64)
    for win in range(3):
        idx = rng.integers(0, voc, (B, T))
        ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
        tgt = rng.integers(0, voc, (B, T))
        masks = lm.draw_dropout_masks(B)
        om = [None] + [masks[l].astype(np.float64) for l in range(1, depth)]
        ref_p, st, cache = O.forward_window(cfg, w64, idx, ctx, st, om, keep_cache=True)
        ce, _, _ = O.crossentropy(ref_p, tgt)
        g_data = O.backward_window(cfg, w64, idx, ctx, tgt, ref_p, cache, om, with_regularisers=False)
        lm.loss_acc.zero_()
        lm.train_window(idx, ctx, tgt, masks)
        l, _, _ = lm.read_loss()
        assert abs(l - ce) < 2e-2 * max(1.0, ce), (win, l, ce)
        got_st = lm.get_states()
        for k in range(2 * depth):
            assert np.abs(got_st[:, k] - st[k]).max() < 3e-2, (win, k)
        assert_gradients(lm.layout, lm.get_grads(), g_data, O.regulariser_grads(cfg, w64), rel=2e-2, maxn=4e-2, where=("window", win))
        # keep the oracle's carried state identical to the engine's bf16-rounded one
        st = [got_st[:, k].astype(np.float64) for k in range(2 * depth)]


@pytest.mark.parametrize("depth,width,voc,B,T,use_masks", [(2, 512, 64, 1000, 5, True), (2, 512, 64, 3000, 3, False), (3, 512, 40, 2500, 3, True),
                                                           # (the register-tile backward scan: one mask scale per thread)
                                                           (2, 512, 64, 3000, 8, True),
                                                           # width 1024: up to a multiple of 128 streams (the eight-wave scans' row groups)
                                                           (2, 1024, 40, 300, 4, True)])
def test_train_window_padded_streams(depth, width, voc, B, T, use_masks):
    """A stream count just short of one the second-generation scans take (1000 -> 1024, 3000 -> 3072; 2500 = 1536 + 964 -> 1024)
    is padded with dummy streams (targets -1) and kl_set_loss_rows keeps the means those over the real streams: loss, accuracy,
    gradients and the carried states of the real streams must equal those of the unpadded batch (HipLM.pad_streams = False:
    first-generation scans)."""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, _ = make_model(depth, width, voc)
    rng = np.random.default_rng(14)
    idx = rng.integers(1, voc, (B, T)); tgt = rng.integers(1, voc, (B, T))
    tgt[rng.random((B, T)) < 0.05] = -1                      # (some padded positions among the real streams too)
    ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
    masks = ((rng.random((depth, B, width)) >= 0.1) / 0.9).astype(np.float32) if use_masks else None
    res = {}
    for name, pad in (("plain", False), ("padded", True)):
        lm = make_model(depth, width, voc)[2]
        lm.set_weights(w, hipabi.KL_PREC_BF16)
        lm.pad_streams = pad
        lm.reset_states(B)
        lm.loss_acc.zero_()
        for _ in range(2):
            lm.train_window(idx, ctx, tgt, masks)
        res[name] = (np.array(lm.read_loss()), lm.grads.cpu().numpy().copy(), lm.states.cpu().numpy().copy())
        assert lm.states.shape[0] == B
        # ... and a validation window (bf16 forward, loss only): padded the same way
        lm.forward_window(idx, ctx, tgt, want_probs=False)
        res[name] += (np.array(lm.read_loss()), lm.states.cpu().numpy().copy())
    assert any(lm._padded_streams(b1 - b0, T) != b1 - b0 for b0, b1 in lm._stream_groups(B, T))
    l0, g0, s0, v0, t0 = res["plain"]; l1, g1, s1, v1, t1 = res["padded"]
    assert abs(v0[0] - v1[0]) < 2e-3 * v0[0] and abs(v0[1] - v1[1]) < 2e-3, (v0, v1)
    assert np.abs(t0 - t1).max() < 3e-2
    assert abs(l0[0] - l1[0]) < 1e-3 * l0[0] and abs(l0[2] - l1[2]) < 1e-5 * abs(l0[2]), (l0, l1)
    assert abs(l0[1] - l1[1]) < 2e-3, (l0, l1)
    assert np.abs(s0 - s1).max() < 2e-2
    assert np.linalg.norm(g0 - g1) < 2e-2 * np.linalg.norm(g0), np.linalg.norm(g0 - g1) / np.linalg.norm(g0)


@pytest.mark.parametrize("depth,width,voc,B,T", [(2, 512, 8, 1024, 6), (2, 128, 8, 48, 5),
                                                 # big enough for the fused output layer (V = 256, width 512, B*T >= 8192)
                                                 (2, 512, 256, 1024, 8)])
def test_dummy_stream_targets_count_for_nothing(depth, width, voc, B, T):
    """Target -1 is Keras' all-zero one-hot row (the padded tail of a window, rating.py:1096-1102): no loss, no gradient, but a
    HIT for the accuracy whenever class 0 has the largest probability (arg-max of a zero row is 0).  The dummy streams the engine
    pads a batch with carry target -2 instead: nothing at all.  Same window twice, the last rows once with
    -1 and once with -2: loss and gradients agree, the accuracies differ by exactly the share of positions where class 0 wins."""
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.pad_streams = False
    rng = np.random.default_rng(9)
    idx = rng.integers(0, voc, (B, T)); ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
    tgt = rng.integers(0, voc, (B, T))
    cut = B - B // 8
    out = {}
    for fill in (-1, -2):
        t = tgt.copy(); t[cut:] = fill
        lm.reset_states(B); lm.loss_acc.zero_()
        lm.train_window(idx, ctx, t, None)
        out[fill] = (lm.read_loss(), lm.get_grads())
    lm.reset_states(B)
    probs = lm.forward_window(idx, ctx).cpu().numpy()
    zero_wins = int((probs[cut:].argmax(axis=-1) == 0).sum())
    assert zero_wins > 0                                    # (the case must occur for the test to say anything)
    (l1, a1, _), g1 = out[-1]
    (l2, a2, _), g2 = out[-2]
    assert abs(l1 - l2) < 1e-6 * max(1.0, abs(l1))
    assert abs((a1 - a2) - zero_wins / (B * T)) < 2e-6, (a1, a2, zero_wins)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]) or np.abs(g1[k] - g2[k]).max() <= 1e-6 * np.abs(g1[k]).max(), k


@pytest.mark.parametrize("B,alternatives", [
    (1000, [[(1000, 1000)]]),
    (1280, [[(1280, 1280)], [(1024, 1024), (256, 256)]]),
    (2560, [[(2048, 2048), (512, 512)], [(1536, 1536), (1024, 1024)]]),
    (3000, [[(2048, 2048), (952, 1024)]]),
    (3584, [[(3072, 3072), (512, 512)], [(2048, 2048), (1536, 1536)]]),
    (4096, [[(2048, 2048), (2048, 2048)], [(2560, 2560), (1536, 1536)]])])
def test_stream_plan_is_the_fastest(B, alternatives):
    """HipLM._plan_512 (width 512: round a batch up to whole blocks of 512 streams, as few and as equal groups as the kernels
    hold) against other ways to run the same batch -- as it is on the first-generation scans, the largest fast count peeled
    off, a lopsided split --, each timed here: the rule's choice is within 5 % of the best (no
    table of measured step times in the engine)."""
    import time
    from ocrd_keraslm_amd.lib import hipabi
    torch = _torch()
    depth, width, voc, T = 2, 512, 64, 256      # (the window length of BASELINE.json's training configuration)
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    rng = np.random.default_rng(2)
    idx = torch.from_numpy(rng.integers(1, voc, (B, T)).astype(np.int32)).cuda()
    ctx = torch.from_numpy(rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1).astype(np.int32)).cuda()
    lm.reset_states(B)

    def ms_per_step(plan):
        lm.plan_override = plan
        for _ in range(3):
            lm.train_window(idx, ctx, idx, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(6):
            lm.train_window(idx, ctx, idx, None)
        torch.cuda.synchronize()
        lm.read_loss()      # (raises on a hand-off time-out)
        return (time.perf_counter() - t0) / 6 * 1e3

    chosen = lm._plan_512(B, 0xfffffff0 // (T * 4 * width * 2))
    t_chosen = ms_per_step(None)
    others = {str(p): ms_per_step(p) for p in alternatives if p != chosen}
    print("B=%d: %s %.2f ms; alternatives %s" % (B, chosen, t_chosen, {k: round(v, 2) for k, v in others.items()}))
    assert t_chosen <= 1.05 * min(others.values()), (chosen, t_chosen, others)


@pytest.mark.parametrize("depth,width,voc,B,T,limit,use_masks", [(2, 512, 64, 2048, 6, 1024, True), (2, 512, 64, 2560, 5, 1024, False),
                                                                 (2, 128, 40, 200, 7, 64, True)])
def test_train_window_stream_groups(depth, width, voc, B, T, limit, use_masks):
    """A batch of more streams than one launch sequence addresses (32-bit offsets into a layer's gate rows: 3072 streams at
    cfg2) runs as groups of streams one after the other (engine.train_window); the streams are independent, so loss,
    gradients and carried states must equal those of the whole batch in one piece -- forced here at sizes where both forms
    run (HipLM.max_streams_per_launch)."""
    torch = _torch()
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, _ = make_model(depth, width, voc)
    rng = np.random.default_rng(13)
    idx = rng.integers(1, voc, (B, T)); tgt = rng.integers(1, voc, (B, T))
    ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
    masks = ((rng.random((depth, B, width)) >= 0.1) / 0.9).astype(np.float32) if use_masks else None
    res = {}
    for name, lim in (("whole", 0), ("groups", limit)):
        lm = make_model(depth, width, voc)[2]
        lm.set_weights(w, hipabi.KL_PREC_BF16)
        lm.max_streams_per_launch = lim
        lm.reset_states(B)
        lm.loss_acc.zero_()
        for _ in range(2):      # (two consecutive windows: the carried states of every group go back to its rows)
            lm.train_window(idx, ctx, tgt, masks)
        res[name] = (np.array(lm.read_loss()), lm.grads.cpu().numpy().copy(), lm.states.cpu().numpy().copy())
        # ... and a validation window (bf16 forward on the training workspace) from those states
        p = lm.forward_window(idx, ctx, tgt, want_probs=True).cpu().numpy()
        res[name] += (p, np.array(lm.read_loss()))
    assert len(lm._stream_groups(B, T)) > 1
    l0, g0, s0, p0, v0 = res["whole"]; l1, g1, s1, p1, v1 = res["groups"]
    assert np.abs(p0 - p1).max() < 2e-2 and abs(v0[0] - v1[0]) < 2e-3 * v0[0], (np.abs(p0 - p1).max(), v0, v1)
    assert abs(l0[0] - l1[0]) < 1e-3 * l0[0] and abs(l0[2] - l1[2]) < 1e-5 * abs(l0[2]), (l0, l1)
    assert abs(l0[1] - l1[1]) < 2e-3, (l0, l1)      # (accuracy: a few arg-max near-ties fall differently between the kernel generations)
    assert np.abs(s0 - s1).max() < 2e-2
    assert np.linalg.norm(g0 - g1) < 2e-2 * np.linalg.norm(g0), np.linalg.norm(g0 - g1) / np.linalg.norm(g0)


@pytest.mark.parametrize("B,windows,env", [
    (512, 4, {}), (1024, 2, {}), (264, 3, {}),
    (2048, 2, {}),                                       # four row blocks per workgroup: prefetched tiles, late stores
    (1040, 2, {}),                                       # 65 row blocks on 32 row groups: uneven visits
    (2560, 1, {}),                                       # five row blocks per workgroup (the 8-block instantiation)
    (1032, 2, {}),                                       # a partial last tile: no prefetch
    (512, 4, {"KL_SENTINEL_BWD": "2"}),                  # sentinel backward with ONE block per workgroup (probe-first spin)
    (1024, 3, {"KL_XCD_LOCAL": "1", "KL_XCD_LOCAL_BWD": "1"}),   # XCD-local publishes (plain stores into the shared L2)
    (528, 3, {"KL_XCD_LOCAL": "1", "KL_SENTINEL_BWD": "2", "KL_XCD_LOCAL_BWD": "1"}),    # ... with surplus workgroups exiting
    # second-generation wide scans over consecutive full-length windows (re-armed sentinels, carried state): bf16 accuracy
    (1024, 3, {"KL_SCAN2": "1"}), (2048, 2, {"KL_SCAN2": "1"}), (2048, 2, {"KL_SCAN2": "1", "KL_SCAN2_ROWS": "32"}),
    (3072, 2, {"KL_SCAN2": "1"})])
def test_handoff_flavours_agree_bitwise(B, windows, env):
    """The scans' two hand-off protocols (data sentinels / counters) run the same arithmetic, so over
    consecutive stateful windows the carried states must agree BITWISE -- a stale or torn read in either
    protocol would show as a difference -- and the launch-per-step path must agree to bf16 accuracy
    (tools/check_handoff.py screens hundreds of windows the same way)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "check_handoff", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_handoff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad, g, c = mod.run(B, windows, verbose=False, env_a=env)
    assert bad == 0
    assert g < (3e-2 if env.get("KL_SCAN2") == "1" else 1e-3) and c < 5e-2, (g, c)


@pytest.mark.parametrize("depth,width,voc,B,T", [(2, 128, 50, 6, 12), (2, 512, 64, 128, 9), (1, 64, 30, 3, 5),
                                                 # big enough for the fused output layer (V = 256, width 512, B*T >= 8192)
                                                 (2, 512, 256, 1024, 8),
                                                 # ... a batch the engine pads with dummy windows (1000 -> 1024): the means stay over 1000
                                                 (2, 512, 64, 1000, 6)])
def test_stateless_window_mode(depth, width, voc, B, T):
    """kl_set_window_mode(1): the reference's stateless graph (rating.py:126-129, 1123-1126) -- windows start
    from zero state, ONE target per window at its last position, loss / accuracy are means over the B
    windows, the dropout mask is shared by the whole batch (noise_shape (1, W), rating.py:150)."""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.set_window_mode(True)
    lm.reset_states(B)
    rng = np.random.default_rng(8)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    idx = rng.integers(0, voc, (B, T))
    ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
    last = rng.integers(0, voc, B)
    tgt = np.full((B, T), -1)
    tgt[:, -1] = last
    one = lm.draw_dropout_masks(1)
    masks = np.repeat(one, B, axis=1)
    om = [None] + [masks[l].astype(np.float64) for l in range(1, depth)]
    ref_p, _, cache = O.forward_window(cfg, w64, idx, ctx, O.zero_states(cfg, B, np.float64), om, keep_cache=True)
    p_last = np.clip(ref_p[np.arange(B), -1, last], 1e-7, 1 - 1e-7)
    ce = float(np.mean(-np.log(p_last)))
    acc = float(np.mean(ref_p[:, -1].argmax(axis=1) == last))
    g_ce = O.backward_window(cfg, w64, idx, ctx, tgt, ref_p, cache, om, with_regularisers=False)
    lm.loss_acc.zero_()
    lm.train_window(idx, ctx, tgt, masks)
    l, a, _ = lm.read_loss()
    assert abs(l - ce) < 2e-2 * max(1.0, ce), (l, ce)
    assert abs(a - acc) < 1e-6, (a, acc)
    from tests.gradcheck import assert_gradients
    # (mean over B rows instead of B*T positions; E / Ctx also on the back-propagated part alone)
    assert_gradients(lm.layout, lm.get_grads(), {k: T * v for k, v in g_ce.items()}, O.regulariser_grads(cfg, w64),
                     rel=1.5e-2, maxn=3e-2, where=("stateless", depth, width, B, T))
    # inference in the same mode: probabilities of the last position, loss over the B windows
    lm.prepare(hipabi.KL_PREC_SPLIT)
    lm.reset_states(B)
    lm.loss_acc.zero_()
    ref_i, _, _ = O.forward_window(cfg, w64, idx, ctx, O.zero_states(cfg, B, np.float64))
    probs = lm.forward_window(idx, ctx, tgt).cpu().numpy()
    assert np.abs(probs[:, -1] - ref_i[:, -1]).max() < 2e-5
    l2, a2, _ = lm.read_loss()
    ce_i = float(np.mean(-np.log(np.clip(ref_i[np.arange(B), -1, last], 1e-7, 1 - 1e-7))))
    assert abs(l2 - ce_i) < 1e-4 * max(1, ce_i)
    assert abs(a2 - float(np.mean(ref_i[:, -1].argmax(axis=1) == last))) < 1e-6


@pytest.mark.parametrize("depth,width,voc,B,T", [(2, 128, 40, 4, 16), (2, 512, 64, 272, 6)])
def test_training_trajectory_matches_oracle(depth, width, voc, B, T):
    """Several consecutive optimizer steps (forward, backward, clip + Adam, carried state, fresh dropout
    masks) on the HIP engine and on the f64 oracle from the same start: the loss sequence and the weights
    after the last step stay together (bf16 compute: 2 % on losses, 2e-3 absolute on weights after 6
    steps of lr 1e-3)."""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.reset_states(B)
    lm.ensure_training_buffers()
    rng = np.random.default_rng(77)
    wo = {k: v.astype(np.float64) for k, v in w.items()}
    opt = O.Adam(cfg, dtype=np.float64)
    st = O.zero_states(cfg, B, np.float64)
    for step in range(6):
        idx = rng.integers(0, voc, (B, T))
        ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1)
        tgt = rng.integers(0, voc, (B, T))
        masks = lm.draw_dropout_masks(B)
        om = [None] + [masks[l].astype(np.float64) for l in range(1, depth)]
        ref_p, st, cache = O.forward_window(cfg, wo, idx, ctx, st, om, keep_cache=True)
        ce, _, _ = O.crossentropy(ref_p, tgt)
        g = O.backward_window(cfg, wo, idx, ctx, tgt, ref_p, cache, om)
        opt.step(wo, g)
        lm.loss_acc.zero_()
        lm.train_window(idx, ctx, tgt, masks)
        lm.adam_step()
        l, _, _ = lm.read_loss()
        assert abs(l - ce) < 2e-2 * max(1.0, ce), (step, l, ce)
    got = lm.get_weights()
    for k in wo:
        assert np.abs(got[k] - wo[k]).max() < 2e-3, k
    states = lm.get_states()
    for k in range(2 * depth):
        assert np.abs(states[:, k] - st[k]).max() < 3e-2


def test_random_shapes_sweep():
    """a fixed-seed slice of tools/fuzz_parity.py: random depth / width / vocabulary / contexts / batch /
    window length (odd batch sizes, no context variable, 1-step windows ...) against the f64 oracle"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(14, 3, verbose=False) == 0
