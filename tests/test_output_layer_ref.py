"""tests/output_layer_ref.py against the oracle on the same probabilities (no GPU): loss, accuracy and per-position loss of
oracle.crossentropy, and the `dlog` lines of oracle.backward_window -- read off grads["E"] = dlog^T . h_top with an identity for
h_top and all-zero gates, so that nothing else of the backward pass contributes."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests.output_layer_ref import softmax_ce_ref


def _case(seed, B, T, V):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, T, V)) * 2.5
    tgt = rng.integers(0, V, (B, T))
    tgt[rng.random((B, T)) < 0.2] = -1
    # peaked rows on both sides of the clip, a tie with character 0 under a padded and under a real target
    z[0, 0] = 0.0; z[0, 0, 3] = 40.0; tgt[0, 0] = 3
    z[1, 0] = 0.0; z[1, 0, 3] = 40.0; tgt[1, 0] = 4
    z[2, T - 1] = -1.0; z[2, T - 1, 0] = z[2, T - 1, V - 1] = 7.0; tgt[2, T - 1] = -1
    z[3, T - 1] = -1.0; z[3, T - 1, 0] = z[3, T - 1, V - 1] = 7.0; tgt[3, T - 1] = V - 1
    return z, tgt


@pytest.mark.parametrize("B,T,V", [(4, 5, 7), (6, 1, 30), (4, 6, 5)])
def test_reference_matches_oracle(B, T, V):
    z, tgt = _case(B * 100 + V, B, T, V)
    probs = O.softmax(z)
    z_tm = z.transpose(1, 0, 2).reshape(T * B, V)
    ref = softmax_ce_ref(z_tm, tgt, 1.0 / (B * T), ld_dl=V + 3)
    ce, acc, l = O.crossentropy(probs, tgt)
    assert abs(ref["loss"].sum() - ce) < 1e-12
    assert abs(ref["hit"].sum() - acc) < 1e-12
    assert np.abs(ref["loss"].reshape(T, B).T * (B * T) - l).max() < 1e-12
    assert (ref["dlogits"][:, V:] == 0).all()
    # dlog through backward_window: depth 1, no context, width B*T, h_top = identity, gates zero -> grads["E"] = dlog^T
    W = B * T
    cfg = O.ModelConfig(1, W, V, 0)
    w = {name: np.zeros(shape) for name, shape in cfg.param_shapes()}
    zeros = np.zeros((B, T, W))
    cache = {"h": [np.eye(W).reshape(B, T, W)], "gates": [np.zeros((B, T, 4, W))], "c": [zeros], "x": [zeros], "hpre": [zeros],
             "states_in": [np.zeros((B, W)), np.zeros((B, W))]}
    g = O.backward_window(cfg, w, np.zeros((B, T), np.int64), np.zeros((B, T, 0), np.int64), tgt, probs, cache,
                          with_regularisers=False)
    dlog = g["E"].T.reshape(B, T, V)
    got = ref["dlogits"][:, :V].reshape(T, B, V).transpose(1, 0, 2)
    assert np.abs(got - dlog).max() < 1e-12
    assert np.abs(dlog).max() > 0
    assert (got[0, 0] == 0).all() and (got[1, 0] == 0).all()      # both peaked rows are clipped: no gradient


def test_reference_dummy_streams_and_last_only():
    B, T, V = 5, 4, 9
    z, tgt = _case(1, B, T, V)
    z_tm = z.transpose(1, 0, 2).reshape(T * B, V)
    inv = 1.0 / 7
    full = softmax_ce_ref(z_tm, tgt, inv)
    dummy = tgt.copy()
    dummy[3] = -2
    r = softmax_ce_ref(z_tm, dummy, inv)
    rows3 = np.arange(T) * B + 3
    assert (r["dlogits"][rows3] == 0).all() and (r["loss"][rows3] == 0).all() and (r["hit"][rows3] == 0).all()
    keep = np.setdiff1d(np.arange(B * T), rows3)
    for k in ("dlogits", "loss", "hit"):
        assert np.array_equal(r[k][keep], full[k][keep])
    last = softmax_ce_ref(z_tm, tgt, inv, last_only=True)
    for k in ("dlogits", "loss", "hit"):
        assert (last[k][:(T - 1) * B] == 0).all()
        assert np.array_equal(last[k][(T - 1) * B:], full[k][(T - 1) * B:])
    assert last["hit"][(T - 1) * B + 2] == inv and last["hit"][(T - 1) * B + 3] == 0      # tie: padded target hits, V - 1 does not
