"""The output layer of a training window in plain numpy, f64: what the softmax / cross-entropy / dH kernels are held to
(tests/test_output_layer_gpu.py) and what tests/test_output_layer_ref.py pins to oracle.crossentropy / backward_window.

Rows are time-major, r = t * B + b, the target of row r is tgt[b][t]: -1 = padded position (no loss, no gradient, a hit when
the first maximum is character 0 -- Keras' argmax of an all-zero row), < -1 = dummy stream (counts for nothing); `last_only`
drops every position but t = T - 1 (neither target nor accuracy).  Probabilities outside [1e-7, 1 - 1e-7] are clipped in the
loss and carry no gradient (rating.py:255-258 through Keras)."""
import numpy as np

CLIP = 1e-7


def logits_ref(X, E, V):
    """X [M][W], E [>= V][W] (bf16 values are exact in f64) -> z [M][V]"""
    return np.asarray(X, np.float64) @ np.asarray(E, np.float64)[:V].T


def softmax_ce_ref(z, tgt, inv_count, last_only=False, ld_dl=None):
    """z [B*T][V] time-major, tgt [B][T] -> dict of per-row arrays; dlogits is [B*T][ld_dl] with zeros from column V on"""
    z = np.asarray(z, np.float64)
    (M, V), (B, T) = z.shape, tgt.shape
    assert M == B * T
    t = np.asarray(tgt, np.int64).T.reshape(-1)
    counts = t >= -1
    if last_only:
        counts &= np.repeat(np.arange(T), B) == T - 1
    valid = counts & (t >= 0)
    tsafe = np.where(valid, t, 0)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    s = e.sum(axis=1)
    p = e / s[:, None]
    rows = np.arange(M)
    pt = p[rows, tsafe]
    one_minus_pt = (s - e[rows, tsafe]) / s
    active = valid & (pt >= CLIP) & (pt <= 1 - CLIP)
    onehot = np.zeros_like(p)
    onehot[rows, tsafe] = 1.0
    dlogits = np.zeros((M, V if ld_dl is None else ld_dl))
    dlogits[:, :V] = (p - onehot) * active[:, None] * inv_count
    loss = np.where(valid, -np.log(np.clip(pt, CLIP, 1 - CLIP)), 0.0) * inv_count
    amax = z.argmax(axis=1)                       # (the first maximum)
    hit = np.where(counts & (amax == tsafe), inv_count, 0.0)
    top2 = np.partition(z, V - 2, axis=1)[:, V - 2:] if V > 1 else np.stack([z[:, 0] - np.inf, z[:, 0]], axis=1)
    return {"p": p, "pt": pt, "one_minus_pt": one_minus_pt, "valid": valid, "counts": counts, "active": active,
            "dlogits": dlogits, "loss": loss, "hit": hit, "amax": amax, "gap": top2[:, 1] - top2[:, 0]}


def dh_ref(dlogits, E):
    """dH = dlogits . E over the columns both have -> (dH [M][W], sum_k |a_k| |b_k| per element, for the rounding bounds)"""
    a, b = np.asarray(dlogits, np.float64), np.asarray(E, np.float64)
    k = min(a.shape[1], b.shape[0])
    return a[:, :k] @ b[:k], np.abs(a[:, :k]) @ np.abs(b[:k])
