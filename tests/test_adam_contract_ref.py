"""The one-step Adam contract (tests/adam_contract.py) without a GPU: its f64 reference against the oracle's Adam, an f32
restatement of the kernel inside every bound on every input the GPU test uses, and nine mistakes each rejected."""
import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests import adam_contract as A

N = 20011      # (no multiple of the launch's block size, like the second model's parameter count)


def _live():
    """a padding pattern like a padded width's: 28 of every 128 positions are padding"""
    return (np.arange(N) % 128) < 100


def _combinations():
    return [(h, s, t) for h in A.HYPER for s in A.SCALES for t in A.STEPS]


def test_reference_is_the_oracles_adam():
    """on ordinary gradients, three steps from zero moments: the f64 reference (chained here, one step at a time) and
    oracle.Adam in f64 agree to 1e-4 relative -- what is left is the constant 1 - b2, which the oracle forms from the decimal
    0.999 and the contract from the f32 number"""
    cfg = O.ModelConfig(1, 64, 20)
    rng = np.random.default_rng(5)
    w = {k: v.astype(np.float64) for k, v in O.init_weights(cfg, seed=4, emb_std=0.5).items()}
    opt = O.Adam(cfg, dtype=np.float64)
    lr, b1, b2, eps, clip = A.HYPER["defaults"]
    prev_m = {k: np.zeros(v.shape) for k, v in w.items()}
    prev_v = {k: np.zeros(v.shape) for k, v in w.items()}
    for t in (1, 2, 3):
        grads = {k: (rng.standard_normal(v.shape) * 0.3).astype(np.float32) for k, v in w.items()}
        before = {k: v.copy() for k, v in w.items()}
        opt.step(w, {k: g.astype(np.float64) for k, g in grads.items()})
        # one step of the reference from the oracle's own p, m, v of the step before (the f32 copies of them)
        for k in w:
            ref = A.reference(before[k], grads[k], prev_m[k], prev_v[k], t, lr, b1, b2, eps, clip, 1.0)
            upd = before[k] - w[k]
            got = before[k].astype(np.float32).astype(np.float64) - ref["p"]
            assert np.abs(got - upd).max() <= 1e-4 * np.abs(upd).max(), (t, k)
            assert np.abs(ref["m"] - opt.m[k]).max() <= 1e-4 * np.abs(opt.m[k]).max(), (t, k)
            assert np.abs(ref["v"] - opt.v[k]).max() <= 1e-4 * np.abs(opt.v[k]).max(), (t, k)
        prev_m = {k: opt.m[k].copy() for k in w}
        prev_v = {k: opt.v[k].copy() for k in w}


def test_inputs_hold_every_kind():
    live = _live()
    for name in A.HYPER:
        for s in A.SCALES:
            inp = A.make_inputs(N, A.HYPER[name], s, live=live)
            clip = np.float32(A.HYPER[name][4])
            gs = inp["g"] * np.float32(s)
            for k, kind in enumerate(A.KINDS):
                assert ((inp["kind"] == k) & live).sum() >= 100, kind
            edge = live & (inp["kind"] == A.KINDS.index("edge"))
            assert (np.abs(gs[edge]) == clip).any() and (np.abs(gs[edge]) > clip).any() and (np.abs(gs[edge]) < clip).any()
            assert (np.abs(gs[edge]) >= clip * 9e5).any() and (gs[edge] > 0).any() and (gs[edge] < 0).any()
            across = live & np.isin(inp["kind"], (A.KINDS.index("across0"), A.KINDS.index("across")))
            if s != 1.0:      # what the scale moves across the clip, both signs
                moved = across & (np.abs(inp["g"]) > clip) & (np.abs(gs) < clip)
                assert (inp["g"][moved] > 0).any() and (inp["g"][moved] < 0).any()
            assert (across & (np.abs(gs) > clip)).any()
            tiny = live & (inp["kind"] == A.KINDS.index("tiny"))
            assert np.abs(inp["g"][tiny]).max() <= 1e-6 and np.abs(inp["g"][tiny]).min() >= 1e-12
            assert not inp["m"][tiny].any() and not inp["v"][tiny].any()
            assert (inp["v"].astype(np.float64) >= inp["m"].astype(np.float64) ** 2 * (1 - 1e-6)).all()
            both = live & (inp["g"] != 0) & (inp["m"] != 0)
            assert np.abs(inp["p"][both]).min() >= A.P_FLOOR
            assert not any(inp[k][~live].any() for k in "pgmv")
            # in the tiny segment eps dominates the root and the update is still many ulps of p
            hp = A.HYPER[name]
            ref = A.reference(inp["p"], inp["g"], inp["m"], inp["v"], 1, *hp, s)
            assert (np.sqrt(ref["v"][tiny]) < 0.5 * hp[3]).all()
            ulps = (np.abs(ref["delta"][tiny]) / (np.abs(inp["p"][tiny]) * 2.0 ** -23)).max()
            assert ulps >= (1000 if (name, s) == ("defaults", 1.0) else 100), (name, s, ulps)


def test_restatement_is_within_every_bound():
    live = _live()
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for name, s, t in _combinations():
        hp = A.HYPER[name]
        inp = A.make_inputs(N, hp, s, seed=t, live=live)
        args = (inp["p"], inp["g"], inp["m"], inp["v"], t) + hp + (s,)
        rep = A.check(A.restate_f32(*args), A.reference(*args), live, where=(name, s, t))
        worst = {k: max(worst[k], rep[k]) for k in worst}
    print("ADAM RATIOS | f32 restatement | p %.2f | m %.2f | v %.2f" % (worst["p"], worst["m"], worst["v"]))


# where each mistake must show: (hyper-parameters, grad_scale, t)
_SHOWS = {"eps inside the root": ("defaults", 1.0, 10), "eps dropped": ("defaults", 1.0, 1), "clip before scale": ("defaults", 0.5, 10),
          "scale ignored": ("second", 1.0 / 3.0, 2), "no bias correction": ("defaults", 1.0, 1), "t frozen at 1": ("defaults", 1.0, 1000),
          "default b2 hard-coded": ("second", 1.0, 10), "clip by norm": ("defaults", 1.0, 2), "m updated with b2": ("second", 0.125, 100000)}


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_mistakes_are_rejected(variant):
    name, s, t = _SHOWS[variant]
    hp = A.HYPER[name]
    live = _live()
    inp = A.make_inputs(N, hp, s, seed=t, live=live)
    args = (inp["p"], inp["g"], inp["m"], inp["v"], t) + hp + (s,)
    ref = A.reference(*args)
    A.check(A.restate_f32(*args), ref, live)
    rep, bad = A.check(A.restate_f32(*args, variant=variant), ref, live, raise_=False)
    print(variant, rep, [b[:2] for b in bad])
    assert bad, (variant, rep)
    with pytest.raises(AssertionError):
        A.check(A.restate_f32(*args, variant=variant), ref, live)


def test_exact_checks_see_one_bit():
    hp = A.HYPER["defaults"]
    live = _live()
    inp = A.make_inputs(N, hp, 1.0, live=live)
    args = (inp["p"], inp["g"], inp["m"], inp["v"], 2) + hp + (1.0,)
    ref = A.reference(*args)
    zero = int(np.flatnonzero(live & (inp["kind"] == A.KINDS.index("zero")))[0])
    got = A.restate_f32(*args)
    got["p"][zero] = np.nextafter(got["p"][zero], np.float32(2))
    with pytest.raises(AssertionError, match="all zero"):
        A.check(got, ref, live)
    got = A.restate_f32(*args)
    got["v"][int(np.flatnonzero(~live)[-1])] = 1e-30
    with pytest.raises(AssertionError, match="padding"):
        A.check(got, ref, live)
