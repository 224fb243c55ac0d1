"""Layer 0's table gradients as sorted segment sums (segsum.hip) through the test entry kl_test_segment_sums.

dZ holds small integers in [-4, 4] as bf16, so every f32 partial sum is exact whatever the order of the additions: the
reference is an integer numpy sum per key and the comparison is bitwise, with no tolerance.  Both result tables and the
workspace start out as junk -- the launcher owns their zeroing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bf16_bits_of_small_ints(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)      # (exact: |x| <= 4)


def _reference(dz, idx, ctx, n_ctx, V, R):
    """dz [T*B][cols] integers, time-major rows; idx [B][T]; ctx [B][T][n_ctx]"""
    idx_tm = idx.T.reshape(-1)
    ok = (idx_tm >= 0) & (idx_tm < V)
    dEK = np.zeros((V, dz.shape[1]), np.int64)
    np.add.at(dEK, idx_tm[ok], dz[ok])
    dCtxK = None
    if n_ctx > 0:
        c_tm = ctx[:, :, 0].T.reshape(-1)
        okc = (c_tm >= 0) & (c_tm < R)
        dCtxK = np.zeros((R, dz.shape[1]), np.int64)
        np.add.at(dCtxK, c_tm[okc], dz[okc])
    return dEK, dCtxK


class _Run:
    """device buffers of one shape; call() runs the launcher on new ids / rows without touching results or workspace"""

    def __init__(self, cols, B, T, V, R, n_ctx, ld=None):
        import torch
        from ocrd_keraslm_amd.lib import hipabi
        self.torch, self.hipabi, self.lib = torch, hipabi, hipabi.load()
        self.cols, self.B, self.T, self.V, self.R, self.n_ctx = cols, B, T, V, R, n_ctx
        self.ld = ld or cols
        n = self.lib.kl_test_segment_sums_ws_bytes(B, T, n_ctx, V, R)
        assert n > 0
        self.ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        self.dEK = torch.full((V, cols), float("nan"), dtype=torch.float32, device="cuda")
        self.dCtxK = torch.full((max(R, 1), cols), float("nan"), dtype=torch.float32, device="cuda")

    def call(self, dz, idx, ctx):
        torch = self.torch
        BT = self.B * self.T
        rows = np.full((BT, self.ld), 3, np.int64)      # (the columns between cols and ld must not be read into any sum)
        rows[:, :self.cols] = dz
        dzd = torch.from_numpy(_bf16_bits_of_small_ints(rows).view(np.int16)).cuda()
        idxd = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
        ctxd = torch.from_numpy(np.ascontiguousarray(ctx, dtype=np.int32)).cuda() if self.n_ctx > 0 else None
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self.hipabi.check(self.lib.kl_test_segment_sums(p(dzd), self.ld, self.B, self.T, self.cols, p(idxd), p(ctxd), self.n_ctx,
                                                        self.V, self.R, p(self.dEK), p(self.dCtxK) if self.n_ctx > 0 else None,
                                                        p(self.ws), None))
        torch.cuda.synchronize()
        ref_e, ref_c = _reference(dz, idx, ctx, self.n_ctx, self.V, self.R)
        got_e = self.dEK.cpu().numpy()
        assert np.array_equal(got_e.view(np.uint32), ref_e.astype(np.float32).view(np.uint32)), \
            ("dEK", np.argwhere(got_e != ref_e)[:5])
        if self.n_ctx > 0:
            got_c = self.dCtxK.cpu().numpy()
            assert np.array_equal(got_c.view(np.uint32), ref_c.astype(np.float32).view(np.uint32)), \
                ("dCtxK", np.argwhere(got_c != ref_c)[:5])


def _rows(rng, BT, cols):
    return rng.integers(-4, 5, (BT, cols))


def test_a_less_than_one_share():
    """15 rows: less than one unrolled group beyond the first, B no multiple of 8, narrow rows (32 lanes), padded row stride"""
    rng = np.random.default_rng(1)
    B, T, V, R, cols = 3, 5, 40, 200, 256
    r = _Run(cols, B, T, V, R, 1, ld=cols + 8)
    r.call(_rows(rng, B * T, cols), rng.integers(0, V, (B, T)), rng.integers(0, R, (B, T, 1)))


def test_b_heavy_repetition():
    rng = np.random.default_rng(2)
    B, T, V, R, cols = 24, 5, 20, 3, 2048
    r = _Run(cols, B, T, V, R, 1)
    r.call(_rows(rng, B * T, cols), rng.integers(0, 3, (B, T)), rng.integers(0, 2, (B, T, 1)))


@pytest.mark.parametrize("B,T", [(1040, 3), (1043, 3)])
def test_c_every_pair_distinct(B, T):
    """runs of length 1 throughout; 1043 x 3 = 3129 rows leave one row for the last share whatever its (even) size"""
    rng = np.random.default_rng(3)
    V, R, cols = 256, 200, 2048
    BT = B * T
    pair = rng.permutation(V * R)[:BT]      # (3120 / 3129 of the 51200 pairs, each once, in no order)
    v_tm, c_tm = pair // R, pair % R
    idx = v_tm.reshape(T, B).T
    ctx = c_tm.reshape(T, B).T[:, :, None]
    r = _Run(cols, B, T, V, R, 1)
    r.call(_rows(rng, BT, cols), idx, ctx)


def test_d_one_run_over_many_shares():
    rng = np.random.default_rng(4)
    B, T, V, R, cols = 1024, 4, 256, 200, 2048
    r = _Run(cols, B, T, V, R, 1)
    share = r.lib.kl_test_segment_sums_share(B, T)
    assert 0 < share and B * T >= 3 * share, share      # the one run spans at least three shares
    r.call(_rows(rng, B * T, cols), np.full((B, T), 77), np.full((B, T, 1), 123))


def test_e_wide_rows_second_context_column_ignored():
    rng = np.random.default_rng(5)
    B, T, V, R, cols = 128, 3, 20, 3, 4096
    ctx = np.stack([rng.integers(0, R, (B, T)), rng.integers(-5, 50, (B, T))], axis=2)
    r = _Run(cols, B, T, V, R, 2)
    r.call(_rows(rng, B * T, cols), rng.integers(0, V, (B, T)), ctx)


def test_f_invalid_ids_dropped_independently():
    rng = np.random.default_rng(6)
    B, T, V, R, cols = 64, 4, 30, 5, 2048
    idx = rng.choice(np.array([-1, V, V + 7] + list(range(V))), (B, T))
    ctx = rng.choice(np.array([-1, R, R + 3] + list(range(R))), (B, T, 1))
    both = (idx < 0) | (idx >= V)
    assert (both & ((ctx[:, :, 0] >= 0) & (ctx[:, :, 0] < R))).any() and (~both & (ctx[:, :, 0] >= R)).any()
    r = _Run(cols, B, T, V, R, 1, ld=cols + 64)
    r.call(_rows(rng, B * T, cols), idx, ctx)


def test_g_no_context_variable():
    rng = np.random.default_rng(7)
    B, T, V, cols = 64, 4, 30, 2048
    r = _Run(cols, B, T, V, 0, 0)
    r.call(_rows(rng, B * T, cols), rng.integers(-1, V + 1, (B, T)), None)


def test_h_second_call_on_the_same_workspace():
    """case b twice, other ids and rows, nothing zeroed in between: stale counters, order or sums would show"""
    rng = np.random.default_rng(8)
    B, T, V, R, cols = 24, 5, 20, 3, 2048
    r = _Run(cols, B, T, V, R, 1)
    r.call(_rows(rng, B * T, cols), rng.integers(0, 3, (B, T)), rng.integers(0, 2, (B, T, 1)))
    r.call(_rows(rng, B * T, cols), rng.integers(10, V, (B, T)), rng.integers(1, R, (B, T, 1)))
