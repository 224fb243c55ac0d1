"""kl_adam_step_scaled, the last link of every training step, held to the one-step contract of tests/adam_contract.py: the
header's formula in f64 from the f32 numbers the call receives, bounds from counting f32 roundings (4 u of m's and of v's
two terms, 8 u of the update + u |p|; u = 2^-24), p, m, v bit-unchanged where g, m and v are all zero, the padding of a
padded width exactly zero.  p, m, v and the gradients are set directly on the engine's tensors before every call, so every
reference starts from the numbers the step itself started from; one call per combination of

  model        (1, 64, 20) and (2, 100, 50) at padded width 128 (a parameter count that is no multiple of the block size)
  hyper        Keras' defaults and lr 3e-3, b1 0.8, b2 0.99, eps 1e-5, clip 0.25
  grad_scale   1, 0.5, 1/3, 1/8
  t            1, 2, 10, 1000, 100000

on the segments of tests/adam_contract.py (the clip's edge to the ulp, zero and decaying moments, gradients so small that
eps dominates the root, what the scale moves across the clip).  tests/test_adam_contract_ref.py shows on the CPU that an
f32 restatement of the kernel passes and that nine mistakes do not.

Observed on an MI355X (largest error / bound over the 80 calls of a model and hyper-parameter set; the bound is 1.00):

  model            hyper     p     m     v
  (1, 64, 20)      defaults  0.99  0.48  0.86
  (1, 64, 20)      second    0.99  0.48  0.78
  (2, 100, 50)     defaults  1.00  0.48  0.88
  (2, 100, 50)     second    1.00  0.52  0.79

(p lands on its bound by construction: where the update is small beside p the bound IS the half ulp of the final
subtraction, u |p| for a p just above a power of two -- the more parameters, the closer one of them lies to one.  v is
largest at grad_scale 1/3, the one scale whose product with g rounds.  16 tests in 1.3 s.  Run with -s for the lines.)
"""
import numpy as np
import pytest

from tests import adam_contract as A

pytestmark = pytest.mark.gpu

_engines = {}


def _engine(model):
    """one engine per model for the module (a call leaves nothing behind that the next one reads: p, m, v and the gradients
    are all set before it)"""
    if model not in _engines:
        from ocrd_keraslm_amd.lib import hipabi
        from ocrd_keraslm_amd.lib.engine import HipLM
        from tests.gradcheck import cached_weights
        depth, width, voc = model
        lm = HipLM(depth, width, voc, 1)
        lm.set_weights(cached_weights(depth, width, voc, 1, 4, 0.3), hipabi.KL_PREC_BF16)
        lm.ensure_training_buffers()
        live = np.zeros(lm.n_params, dtype=bool)
        for name, off, rows, cols in lm.layout:
            live[off:off + rows * cols] = lm._pad(name, np.ones(lm._logical_shape(name), dtype=np.float32)).reshape(-1) != 0
        _engines[model] = (lm, live)
    return _engines[model]


def _step(lm, inp, t, hp, scale):
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    from ocrd_keraslm_amd.lib.engine import _ptr
    with lm._launch():
        for dst, key in ((lm.params, "p"), (lm.grads, "g"), (lm.adam_m, "m"), (lm.adam_v, "v")):
            dst.copy_(torch.from_numpy(inp[key]))
        lr, b1, b2, eps, clip = hp
        hipabi.check(lm.lib.kl_adam_step_scaled(lm.handle, _ptr(lm.grads), float(scale), _ptr(lm.adam_m), _ptr(lm.adam_v), int(t),
                                                lr, b1, b2, eps, clip, lm._stream()), "kl_adam_step_scaled")
    torch.cuda.synchronize()
    return {k: a.detach().cpu().numpy() for k, a in (("p", lm.params), ("m", lm.adam_m), ("v", lm.adam_v))}, lm.grads.cpu().numpy()


@pytest.mark.parametrize("scale", A.SCALES, ids=lambda s: "scale-%.3g" % s)
@pytest.mark.parametrize("hyper", sorted(A.HYPER))
@pytest.mark.parametrize("model", A.MODELS, ids=lambda m: "x".join(map(str, m)))
def test_adam_one_step_contract(model, hyper, scale):
    lm, live = _engine(model)
    assert lm.n_params % 256 != 0 and (not live.all()) == lm.padded == (model == A.MODELS[1])
    hp = A.HYPER[hyper]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for t in A.STEPS:
        inp = A.make_inputs(lm.n_params, hp, scale, seed=t, live=live)
        got, g_after = _step(lm, inp, t, hp, scale)
        assert np.array_equal(g_after.view(np.uint32), inp["g"].view(np.uint32))      # (the gradients are read, never written)
        ref = A.reference(inp["p"], inp["g"], inp["m"], inp["v"], t, *hp, scale)
        rep = A.check(got, ref, live, where=(model, hyper, scale, t))
        worst = {k: max(worst[k], rep[k]) for k in worst}
    print("ADAM RATIOS | %s | %s | scale %.4g | p %.2f | m %.2f | v %.2f" % (model, hyper, scale, worst["p"], worst["m"], worst["v"]))
