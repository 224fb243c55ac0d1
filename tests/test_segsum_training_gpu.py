"""Whole training windows with layer 0's table gradients as sorted segment sums (the default) and as one-hot products
(KL_SEGSUM=0), against the f64 oracle: the same check, bounds and helper as the window tests of test_gpu_kernels.py."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests.test_gpu_kernels import check_train_window_gradients, make_model

pytestmark = pytest.mark.gpu


def _switch(monkeypatch, segsum):
    # (the engine reads the switch when it creates its handle: every case below builds a new one)
    if segsum:
        monkeypatch.delenv("KL_SEGSUM", raising=False)
    else:
        monkeypatch.setenv("KL_SEGSUM", "0")


@pytest.mark.parametrize("segsum", [True, False])
@pytest.mark.parametrize("depth,width,voc,B,T,n_ctx,ctx_values", [
    (2, 512, 20, 1024, 5, 1, 2),        # two context values: runs of thousands of rows, split over many shares
    (2, 512, 64, 3072, 3, 1, 200),      # the flagship's stream count
    (2, 128, 12, 96, 9, 2, 4),          # two context variables: the second stays a one-hot product
    (4, 1024, 20, 128, 3, 2, 200),      # width 1024: rows of 8 KiB in column slabs
    (1, 64, 40, 2, 8, 1, 200)])         # 16 rows of 256 columns
def test_train_window_gradients(monkeypatch, segsum, depth, width, voc, B, T, n_ctx, ctx_values):
    _switch(monkeypatch, segsum)
    check_train_window_gradients(depth, width, voc, B, T, n_ctx, False, ctx_values=ctx_values)


def test_workspace_shrinks_by_the_one_hot_matrices(monkeypatch):
    """the default really plans the segment sums: the training workspace loses OHT and OHC[0] and gains the sort's arrays"""
    import ctypes as C
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    cfg = hipabi.KlConfig(2, 512, 256, 1, 200, 10)
    B, T = 3072, 256
    sizes = {}
    for segsum in (True, False):
        _switch(monkeypatch, segsum)
        h = lib.kl_create(C.byref(cfg))
        sizes[segsum] = lib.kl_window_workspace_bytes(h, B, T, 1)
        lib.kl_destroy(h)
    onehots = (256 + 200) * B * T * 2
    sort = lib.kl_test_segment_sums_ws_bytes(B, T, 1, 256, 200)
    assert abs((sizes[False] - sizes[True]) - (onehots - sort)) <= 1024, (sizes, onehots, sort)


@pytest.mark.parametrize("segsum", [True, False])
def test_consecutive_windows_sort_again(monkeypatch, segsum):
    """two windows with different ids on one engine: the second replays the first one's graph on new ids in the same
    buffers, so the order must be rebuilt and the sums must not carry over"""
    from tests.gradcheck import assert_gradients
    from ocrd_keraslm_amd.lib import hipabi
    _switch(monkeypatch, segsum)
    depth, width, voc, B, T = 2, 512, 64, 1024, 4
    cfg, w, lm = make_model(depth, width, voc, 1, emb_std=0.3)
    lm.set_weights(w, hipabi.KL_PREC_BF16)
    lm.reset_states(B)
    rng = np.random.default_rng(35)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    st = O.zero_states(cfg, B, np.float64)
    for win in range(2):
        idx = rng.integers(0, voc, (B, T)) if win == 0 else rng.integers(voc // 2, voc, (B, T))
        ctx = rng.integers(0, 200, (B, 1, 1)).repeat(T, axis=1) if win == 0 else rng.integers(0, 3, (B, T, 1))
        tgt = rng.integers(0, voc, (B, T))
        ref_p, st, cache = O.forward_window(cfg, w64, idx, ctx, st, None, keep_cache=True)
        ce, _, _ = O.crossentropy(ref_p, tgt)
        g_data = O.backward_window(cfg, w64, idx, ctx, tgt, ref_p, cache, None, with_regularisers=False)
        lm.loss_acc.zero_()
        lm.train_window(idx, ctx, tgt, None)
        l, _, _ = lm.read_loss()
        assert abs(l - ce) < 2e-2 * max(1.0, ce), (win, l, ce)
        got_st = lm.get_states()
        # (bounds of test_train_consecutive_windows_reuse_buffers)
        assert_gradients(lm.layout, lm.get_grads(), g_data, O.regulariser_grads(cfg, w64), rel=2e-2, maxn=4e-2, where=("window", win))
        st = [got_st[:, k].astype(np.float64) for k in range(2 * depth)]
