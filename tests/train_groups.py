"""What HipLM.train_window / forward_window do ABOVE the kernels of a window -- cut a batch into stream groups, pad the last
one with dummy streams, run each with kl_set_loss_rows, compose gradients, loss and accuracy as size-weighted sums, add the
regulariser once, carry a padded group's states through a side buffer, extend its keep-masks -- as cases, inputs and f64
references.  CPU only: used by tests/test_train_groups_gpu.py and by tests/test_window_view_ref.py (the inputs' floor share
and near-tie share, from the oracle alone).

A group of n real streams run as Bp is, for the reference, a window of its own: the group's streams followed by the engine's
dummy streams -- idx 0, ctx 0, zero state, targets -2, keep-masks repeating the group's first Bp - n --, n_real = n and the
mean over count = n * T positions.  Its references are oracle/lstm_oracle.py's alone, as in tests/window_ref.py.

Composition rule (`check_composition`): the engine forms sum_i (n_i / B) part_i in f32 -- one rounding of the weight, one of
each product, one of each sum.  Per element the result is held to 4 k u sum_i |(n_i / B) part_i| with k groups and u = 2^-24
(that count doubled), against the same sum formed in f64 from the captured parts; where every part is exactly zero the
result is exactly zero.

Near ties (`near_tie_share`): bf16 probabilities are within 1e-2 of f64 (include/keraslm_hip.h), so a position whose two
largest f64 probabilities lie within 1e-2 of each other may fall either way in the accuracy; the accuracy of a group may
differ from the oracle's by the share of such positions, and that share must itself be at most NEAR_TIE_MAX = 5 %, or the
check would say nothing.  With the embeddings of standard deviation 0.3 that the sibling modules use the distributions are
nearly flat -- 30 % of the positions are near ties at width 512, 99 % at width 128 --, so these cases draw their embeddings
with standard deviation EMB_SPREAD / sqrt(width) = 32 / sqrt(width) (1.41, 1.0, 2.83: a logit spread that does not depend
on the width), which leaves 1 .. 3 % near ties (tests/test_window_view_ref.py prints and caps them).

Distributions that peaked give a random target a probability below the loss clip of 1e-7 at 1 .. 4 % of the positions, and
dozens more lie within bf16 accuracy of the clip: there the kernels and the oracle may disagree on whether the position has
a gradient at all, and one such position moves its 16-stream tile of dZ by a quarter -- which is not what these tests are
about.  `settle_targets` therefore moves every target whose f64 probability is below TARGET_P_MIN = 1e-6 -- ten times the
clip, where bf16 moves a probability by a few per cent -- to the position's most probable class, decided from the oracle
alone before the engine sees the window (4 .. 13 % of a batch's targets); as a side effect the accuracy is 7 .. 19 %, no
longer the 1 / V of random targets.
"""
from collections import namedtuple

import numpy as np

from oracle import lstm_oracle as O
from tests import window_ref as R

U = 2.0 ** -24
NEAR_TIE = 1e-2
NEAR_TIE_MAX = 0.05
EMB_SPREAD = 32.0
TARGET_P_MIN = 1e-6

Group = namedtuple("Group", "b0 b1 Bp")
GroupCase = namedtuple("GroupCase", "name case plan_override max_streams groups checked route")

_W2, _F8, _BW2, _RT = R._W2, R._F8, R._BW2, R._RT
_KM_SEG = 1 | 8      # kl_window_view.wg_route: K-major products, layer 0 by segment sums (tests/window_grads.py)
_TR_SEG = 4 | 8      # ... explicit transposes


def _gcase(name, shape, groups, fwd, bwd, route, checked=None, plan=None, max_streams=0):
    groups = [Group(*g) for g in groups]
    route = [route] * len(groups) if isinstance(route, tuple) else list(route)
    assert len(route) == len(groups)
    return GroupCase(name, R._case(name, "stream groups", {}, shape, fwd, bwd), plan, max_streams, groups,
                     tuple(range(len(groups))) if checked is None else tuple(checked), route)


# each the smallest shape that takes its path.  route: (second-generation scans, wg_route, wg_pair_mask, wg_db_scan_mask) that
# the view of a checked group must show, one for all groups or one per group.  The weight-gradient products run K-major, dU
# and dK of layer 1 in one paired launch, wherever the group's Bp * T is a multiple of 64: every group
# here but the last of w128-ragged, whose 8 x 7 = 56 rows go through explicit transposes
CASES = [
    # one group, 1040 -> 1536 streams: 65 real row blocks of 16 on 32 row groups, then 31 all-dummy blocks (1040 = 65 x 16: the
    # dummies start on a block boundary; half-dummy blocks come with 520, 3000 and 588 below)
    _gcase("pad-one", (2, 512, 64, 1040, 3), [(0, 1040, 1536)], (_W2, _F8), _BW2, (True, _KM_SEG, 0b10, 0b11)),
    # an unpadded group, then a padded one of 520 = 32.5 blocks: a half-dummy block, and a side buffer beside an in-place group
    _gcase("two-groups", (2, 512, 64, 1544, 3), [(0, 1024, 1024), (1024, 1544, 1024)], (_W2, _F8), _BW2, (True, _KM_SEG, 0b10, 0b11),
           plan=[(1024, 1024), (520, 1024)]),
    # 3000 -> 3072: the register-tile backward scan (one mask scale per thread: the repeated masks), 187.5 real blocks
    _gcase("regtile-pad", (2, 512, 64, 3000, 3), [(0, 3000, 3072)], (_W2, _F8), _RT, (True, _KM_SEG, 0b10, 0b11)),
    # width 1024: 512 + 588 -> 640 on the eight-wave scans (36.75 real blocks); the padded group is checked (its f64
    # reference is the expensive one), both enter the composition
    _gcase("w1024", (2, 1024, 40, 1100, 3), [(0, 512, 512), (512, 1100, 640)], "lstm_scan_fwd_w32_kernel", "lstm_scan_bwd_w32_kernel",
           (False, _KM_SEG, 0b10, 0b11), checked=(1,)),
    # width 128, groups forced by max_streams_per_launch: 64 + 64 + 64 + 8, no padding, a ragged last group
    _gcase("w128-ragged", (2, 128, 40, 200, 7), [(0, 64, 64), (64, 128, 64), (128, 192, 64), (192, 200, 8)],
           ("lstm_scan_fwd_w128_multi_kernel", "lstm_scan_fwd_w128_kernel"), ("lstm_scan_bwd_w128_multi_kernel", "lstm_scan_bwd_w128_kernel"),
           [(False, _KM_SEG, 0b10, 0b11)] * 3 + [(False, _TR_SEG, 0, 0b11)], max_streams=64),
]
VALIDATION = CASES[1]


def weights(gc):
    """`oracle.init_weights` with embeddings of standard deviation 32 / sqrt(width) (see the module text)"""
    from tests.gradcheck import cached_weights
    c = gc.case
    return cached_weights(c.depth, c.width, c.voc, c.n_ctx, 4, EMB_SPREAD / np.sqrt(c.width))


def batch_inputs(gc, seed=21, states=None):
    """`window_ref.make_inputs` of the batch with ALL streams real: keep-masks, a padded tail (-1) in stream 0, carried-in states
    of standard deviation 0.5 (or `states`); the streams make_inputs turns into dummies get targets of their own"""
    c = gc.case
    inp = R.make_inputs(c, seed=seed, states=states)
    rng = np.random.default_rng(1000 + seed)
    inp["tgt"][inp["n_real"]:] = rng.integers(0, c.voc, (c.B - inp["n_real"], c.T))
    inp["n_real"] = c.B
    assert (inp["tgt"] >= -1).all() and (inp["tgt"][0] == -1).any()
    return inp


def group_case(gc, g):
    c = gc.case
    return R._case("%s[%d:%d]" % (gc.name, g.b0, g.b1), c.family, {}, (c.depth, c.width, c.voc, g.Bp, c.T), c.fwd, c.bwd, n_ctx=c.n_ctx)


def group_inputs(inp, g):
    """the window the engine makes of group g of the batch `inp`: its streams, then Bp - n dummy streams (see the module text)"""
    n, extra = g.b1 - g.b0, g.Bp - (g.b1 - g.b0)
    assert extra <= n
    rows = lambda a, fill: np.concatenate([a[g.b0:g.b1], np.full((extra,) + a.shape[1:], fill, dtype=a.dtype)])
    m = inp["masks"][:, g.b0:g.b1]
    return dict(idx=rows(inp["idx"], 0), ctx=rows(inp["ctx"], 0), tgt=rows(inp["tgt"], -2), states=rows(inp["states"], 0),
                masks=np.concatenate([m, m[:, :extra]], axis=1), n_real=n, seed=inp["seed"])


def near_tie_share(probs):
    """the share of positions whose two largest probabilities lie within NEAR_TIE of each other"""
    V = probs.shape[-1]
    top2 = np.partition(probs, V - 2, axis=-1)[..., V - 2:]
    return float(((top2[..., 1] - top2[..., 0]) <= NEAR_TIE).mean())


def group_forward(case, w, ginp, dropout=True):
    """the f64 forward pass of one group's window (`case`: `group_case`, ginp: `group_inputs`), kept for `settle_targets` and
    `group_oracle`; dropout=False: a validation window, no keep-masks"""
    cfg = O.ModelConfig(case.depth, case.width, case.voc, case.n_ctx)
    L = case.depth
    wd = {k: v.astype(np.float64) for k, v in w.items()}
    st = [ginp["states"][:, k].astype(np.float64) for k in range(2 * L)]
    om = [None] + [ginp["masks"][l].astype(np.float64) for l in range(1, L)] if dropout else None
    probs, st_out, cache = O.forward_window(cfg, wd, ginp["idx"], ginp["ctx"], st, om, keep_cache=True)
    return dict(cfg=cfg, wd=wd, om=om, probs=probs, states_out=np.stack(st_out, axis=1), cache=cache)


def settle_targets(fw, ginp):
    """Replaces, in place, every target whose f64 probability is below TARGET_P_MIN by the position's most probable class
    (see the module text) -> how many were replaced.  Afterwards every target's probability is in [TARGET_P_MIN, 1 - TARGET_P_MIN]."""
    n = ginp["n_real"]
    p, tgt = fw["probs"][:n], ginp["tgt"][:n]
    valid = tgt >= 0
    pt = np.take_along_axis(p, np.where(valid, tgt, 0)[..., None], axis=-1)[..., 0]
    low = valid & (pt < TARGET_P_MIN)
    tgt[low] = p.argmax(axis=-1)[low]
    pt = np.take_along_axis(p, np.where(valid, tgt, 0)[..., None], axis=-1)[..., 0][valid]
    assert pt.min() >= TARGET_P_MIN and pt.max() <= 1.0 - TARGET_P_MIN, (pt.min(), pt.max())
    return int(low.sum())


def group_oracle(case, fw, ginp, backward=True):
    """The f64 oracle of one group's window behind `group_forward` -> dict(ce, acc, near_ties: over the group's REAL streams;
    states_out [n][2L][W] f64; and with `backward`: ref64 -- the canonical arrays of `window_ref.references` over all Bp streams
    --, g_data -- the gradient of the mean CE over the n * T real positions, without the regularisers)"""
    T, n = case.T, ginp["n_real"]
    probs, cache = fw["probs"], fw["cache"]
    ce, acc, _ = O.crossentropy(probs[:n], ginp["tgt"][:n])
    out = dict(ce=float(ce), acc=float(acc), near_ties=near_tie_share(probs[:n]), states_out=fw["states_out"][:n])
    if backward:
        g, dz = O.backward_window(fw["cfg"], fw["wd"], ginp["idx"], ginp["ctx"], ginp["tgt"], probs, cache, fw["om"], with_regularisers=False,
                                  keep_dz=True, count=n * T)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        out["ref64"] = dict(h=[f32(a) for a in cache["hpre"]], c=[f32(a) for a in cache["c"]], gates=[f32(a) for a in cache["gates"]],
                            dz=[f32(a) for a in dz])
        out["g_data"] = g
    return out


def settle_batch(gc, w, inp, dropout=True):
    """every group of the batch `inp` as a window of its own, forward pass done and targets settled (also in `inp`, in place)
    -> [(Group, group case, group inputs, forward)], and how many targets were replaced"""
    out, replaced = [], 0
    for g in gc.groups:
        ginp = group_inputs(inp, g)
        case = group_case(gc, g)
        fw = group_forward(case, w, ginp, dropout)
        replaced += settle_targets(fw, ginp)
        inp["tgt"][g.b0:g.b1] = ginp["tgt"][:g.b1 - g.b0]
        out.append((g, case, ginp, fw))
    return out, replaced


def carried_states(gc, w, inp):
    """the f64 oracle's carried-out states of the whole batch `inp` (every stream real, no dummies needed) as f32 [B][2L][W]:
    what a second window starts from where no engine is at hand"""
    ginp = group_inputs(inp, Group(0, gc.case.B, gc.case.B))
    cfg = O.ModelConfig(gc.case.depth, gc.case.width, gc.case.voc, gc.case.n_ctx)
    L = gc.case.depth
    _p, st_out, _c = O.forward_window(cfg, {k: v.astype(np.float64) for k, v in w.items()}, ginp["idx"], ginp["ctx"],
                                      [ginp["states"][:, k].astype(np.float64) for k in range(2 * L)],
                                      [None] + [ginp["masks"][l].astype(np.float64) for l in range(1, L)])
    return np.stack(st_out, axis=1).astype(np.float32)


def check_composition(parts, sizes, got, where=""):
    """parts: the groups' f32 arrays; sizes: their real stream counts; got: what the engine composed (see the module text).
    -> the largest error / bound"""
    B, k = sum(sizes), len(parts)
    terms = [(n / B) * np.asarray(p, dtype=np.float64) for n, p in zip(sizes, parts)]
    ref = sum(terms)
    bound = 4 * k * U * sum(np.abs(t) for t in terms)
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    zero = bound == 0
    assert not got[zero].any(), (where, "non-zero where every group's part is exactly zero", int(np.flatnonzero(got.ravel() * zero.ravel())[0]))
    over = err[~zero] / bound[~zero]
    worst = float(over.max()) if over.size else 0.0
    assert worst <= 1.0 and not np.isnan(err).any(), (where, "composition beyond 4 k u sum |w_i part_i|", worst)
    return worst
