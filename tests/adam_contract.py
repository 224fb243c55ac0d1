"""kl_adam_step_scaled held to a ONE-STEP contract: the formula of include/keraslm_hip.h in f64, from the f32 numbers the call
receives, against what one call makes of given p, m, v and gradients.

  g_c  = clip(g * grad_scale, -clip, clip)                      (the scale BEFORE the clip)
  m'   = b1 m + (1 - b1) g_c          v' = b2 v + (1 - b2) g_c^2
  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
  p'   = p - lr_t m' / (sqrt(v') + eps)                         (eps OUTSIDE the root)

`reference` takes lr, b1, b2, eps, clip and grad_scale as the f32 values the C call receives and forms 1 - b1 and 1 - b2 from
those: both differences are exact in f32 for b in [0.5, 1], so the f64 constants ARE the kernel's (`1 - 0.999` formed from the
decimal number is 4.7e-5 away from it, which is why tests/test_gpu_kernels.py::test_adam_step_matches_oracle cannot go below
1e-6 absolute).  Every reference starts from the p, m, v the step itself started from, so nothing compounds.

`check` -- bounds from counting f32 roundings (u = 2^-24 is one), nothing measured:
  m'   4 u (|b1 m| + |(1 - b1) g_c|)        one rounding each of g * scale, the two products and the sum: at most 3 u of the
                                             terms, plus one
  v'   4 u (|b2 v| + |(1 - b2) g_c^2|)      the same count with g_c^2 (the rounding of g * scale counts twice): 2 u + 5 u of
                                             the two terms at the very worst, 4 u of both is a rounding count doubled
  p'   8 u |D| + u |p|                       D the f64 update: lr_t, the product, the root (half of v's error), + eps, the
                                             quotient, m's own error -- about 8 roundings of D, each 0.4 u in the mean --, and
                                             the final subtraction, half an ulp of p'
and without tolerance: where g, m and v are all zero p, m, v keep their BITS (this is how the padded hidden units of a padded
width stay out of training), and positions outside `live` (the padding) are exactly zero afterwards.

The bound of p' is relative to D.  m' = b1 m + (1 - b1) g_c cancels where the two terms have opposite signs, and then m's
rounding error, 3 u (|b1 m| + |(1 - b1) g_c|), is NOT small beside D ~ m'.  Its share of p' is at most
3 u lr_t (|b1 m| + |(1 - b1) g_c|) / sqrt(v'); with v >= m^2 (true of Adam's own moments, and of the ones drawn here) Cauchy's
inequality gives (b1 |m| + (1 - b1) |g_c|) / sqrt(b2 m^2 + (1 - b2) g_c^2) <= sqrt(b1^2 / b2 + (1 - b1)^2 / (1 - b2)) = 3.3
(0.9, 0.999) or 2.2 (0.8, 0.99), and lr_t <= lr: 1e-2 u and 2e-2 u.  `make_inputs` therefore keeps |p| >= P_FLOOR = 0.05
wherever non-zero moments meet a non-zero gradient, so that the u |p| term covers it; where the moments are zero nothing
cancels and p is anything, zero included.

`make_inputs` lays the cases out as CHUNK-long segments of the flat vector, kind after kind, again and again to its end (so
every kind also lies in the last, partial launch block and around the padding):
  edge      |g * scale| exactly `clip`, one and two ulps of g above and below, and 1e6 times above; both signs; moments set
  zero      g = 0 on zero moments: bit-unchanged
  decay     g = 0 on non-zero moments: decay only
  tiny      |g| log-uniform in [1e-12, 1e-6] on zero moments: eps dominates sqrt(v'), the update is still up to thousands
            of ulps of p  (|g * scale| >= 1e-13: g_c^2 and (1 - b2) g_c^2 are normal f32 numbers)
  plain0    N(0, 0.3) on zero moments, p of any size
  plain     N(0, 0.3) on non-zero moments
  across0   g = +-clip x {0.9, 1.5, 2.5, 6} and +-clip x {0.9, 1.5} / scale on zero moments: what a scale below 1 moves from
            above the clip to below it, what stays above, what the clip would cut to a different number had it come first
  across    the same on non-zero moments
`restate_f32` is the kernel in numpy f32 and, with `variant`, the mistakes tests/test_adam_contract_ref.py tells apart.
Used by tests/test_adam_contract_ref.py (CPU) and tests/test_adam_contract_gpu.py.
"""
import numpy as np

U = 2.0 ** -24
P_FLOOR = 0.05
CHUNK = 48
KINDS = ("edge", "zero", "decay", "tiny", "plain0", "plain", "across0", "across")

# (lr, b1, b2, eps, clip): Keras' defaults as the engine passes them, and a second set
HYPER = {"defaults": (1e-3, 0.9, 0.999, 1e-7, 1.0), "second": (3e-3, 0.8, 0.99, 1e-5, 0.25)}
SCALES = (1.0, 0.5, 1.0 / 3.0, 0.125)
STEPS = (1, 2, 10, 1000, 100000)
MODELS = ((1, 64, 20), (2, 100, 50))      # the second: padded width 128, a parameter count that is no multiple of 256

VARIANTS = ("eps inside the root", "eps dropped", "clip before scale", "scale ignored", "no bias correction", "t frozen at 1",
            "default b2 hard-coded", "clip by norm", "m updated with b2")


def _f(x):
    return float(np.float32(x))


def step_size(t, lr, b1, b2):
    """lr_t in f64 from the f32 hyper-parameters"""
    lr, b1, b2 = _f(lr), _f(b1), _f(b2)
    return lr * np.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t))


def reference(p, g, m, v, t, lr, b1, b2, eps, clip, grad_scale):
    """-> dict(p, m, v: the f64 results; delta; bound_p, bound_m, bound_v; untouched: where g, m and v are all zero; old: the
    f32 (p, m, v) the step started from)"""
    old = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (p, m, v))
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    b1, b2, eps, clip, s = _f(b1), _f(b2), _f(eps), _f(clip), _f(grad_scale)
    gc = np.clip(g * s, -clip, clip)
    m1a, m1b = b1 * m, (1.0 - b1) * gc
    v1a, v1b = b2 * v, (1.0 - b2) * gc * gc
    m1, v1 = m1a + m1b, v1a + v1b
    delta = step_size(t, lr, b1, b2) * m1 / (np.sqrt(v1) + eps)
    return dict(p=p - delta, m=m1, v=v1, delta=delta, bound_m=4 * U * (np.abs(m1a) + np.abs(m1b)),
                bound_v=4 * U * (np.abs(v1a) + np.abs(v1b)), bound_p=8 * U * np.abs(delta) + U * np.abs(p),
                untouched=(g == 0) & (m == 0) & (v == 0), old=old)


def check(got, ref, live=None, where="", raise_=True):
    """got: dict(p, m, v) f32 arrays after the step; ref: `reference`'s dict; live: bool per position, False in the padding of a
    padded-width model.  -> {p, m, v: the largest error / bound}; raises AssertionError naming every array beyond its bound
    (the worst position, what it got and what is due) and every exact check that failed -- or, with raise_=False, returns
    (report, list of failures)."""
    report, bad = {}, []
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    for k, name in enumerate(("p", "m", "v")):
        a = np.asarray(got[name], dtype=np.float32)
        err = np.abs(a.astype(np.float64) - ref[name])
        bound = ref["bound_" + name]
        over = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        over = np.where(np.isnan(err), np.inf, over)
        i = int(np.argmax(over))
        report[name] = float(over[i])
        if not over[i] <= 1.0:
            bad.append((name, "%d positions beyond their bound" % int((~(over <= 1.0)).sum()), "worst at %d" % i, "got %.9g" % a[i],
                        "due %.9g" % ref[name][i], "error %.3g" % err[i], "bound %.3g" % bound[i]))
        same = bits(a) == bits(ref["old"][k])
        if not same[ref["untouched"]].all():
            j = int(np.flatnonzero(ref["untouched"] & ~same)[0])
            bad.append((name, "changed where g, m and v are all zero", "first at %d" % j, "got %.9g" % a[j], "was %.9g" % ref["old"][k][j]))
        if live is not None and a[~live].any():
            bad.append((name, "non-zero in the padding", "first at %d" % int(np.flatnonzero(~live & (a != 0))[0])))
    if not raise_:
        return report, bad
    assert not bad, (where, bad)
    return report


def _ulps(x, k):
    """the f32 number k ulps from x, away from zero for k > 0"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else 0.0), dtype=np.float32)
    return x


def make_inputs(n, hyper, grad_scale, seed=0, live=None):
    """-> dict(p, g, m, v: f32 [n]; kind: int8 [n], the index into KINDS) for one call with the hyper-parameters `hyper` = (lr, b1,
    b2, eps, clip) and `grad_scale` (see the module text); all four arrays zero outside `live`"""
    rng = np.random.default_rng(seed)
    clip, s = np.float32(hyper[4]), np.float32(grad_scale)
    kind = ((np.arange(n) // CHUNK) % len(KINDS)).astype(np.int8)
    j = np.arange(n) % CHUNK
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    g = (rng.standard_normal(n) * 0.3).astype(np.float32)
    # moments as a run of Adam steps leaves them: v >= m^2
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (m.astype(np.float64) ** 2 + rng.random(n) * 1e-2).astype(np.float32)
    p = (rng.standard_normal(n) * 0.3).astype(np.float32)
    away = (sign * (P_FLOOR + np.abs(p))).astype(np.float32)      # |p| >= P_FLOOR
    at_clip = np.float32(clip / s)
    edge = np.array([_ulps(at_clip, k) for k in (0, 1, -1, 2, -2)] + [np.float32(at_clip * np.float32(1e6))], dtype=np.float32)
    edge = np.concatenate([edge, -edge])
    across = np.concatenate([clip * np.array([0.9, 1.5, 2.5, 6.0], dtype=np.float32),
                             (clip * np.array([0.9, 1.5], dtype=np.float32) / s).astype(np.float32)])
    across = np.concatenate([across, -across]).astype(np.float32)
    is_ = lambda name: kind == KINDS.index(name)
    g = np.where(is_("edge"), edge[j % len(edge)], g)
    g = np.where(is_("zero") | is_("decay"), np.float32(0), g)
    tiny = (sign * np.exp(rng.uniform(np.log(1e-12), np.log(1e-6), n))).astype(np.float32)
    g = np.where(is_("tiny"), tiny, g)
    g = np.where(is_("across0") | is_("across"), across[j % len(across)], g).astype(np.float32)
    zero_moments = is_("zero") | is_("tiny") | is_("plain0") | is_("across0")
    m = np.where(zero_moments, np.float32(0), m).astype(np.float32)
    v = np.where(zero_moments, np.float32(0), v).astype(np.float32)
    p = np.where(is_("plain0") | is_("across0") | is_("zero"), p, away).astype(np.float32)
    nz = g[g != 0]
    assert np.abs(nz).min() >= 1e-15 and np.abs(nz * s).min() >= 1e-13
    out = dict(p=p, g=g, m=m, v=v)
    if live is not None:
        out = {k: np.where(live, a, np.float32(0)).astype(np.float32) for k, a in out.items()}
    out["kind"] = kind
    return out


def restate_f32(p, g, m, v, t, lr, b1, b2, eps, clip, grad_scale, variant=None):
    """adam_kernel of csrc/elementwise.hip and kl_adam_step_scaled's lr_t in numpy f32 -> dict(p, m, v).  `variant`: one of
    VARIANTS, a mistake such a kernel could make."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    lr, b1, b2, eps, clip, s = (f(x) for x in (lr, b1, b2, eps, clip, grad_scale))
    assert variant is None or variant in VARIANTS, variant
    if variant == "default b2 hard-coded":
        b2 = f(0.999)
    tt = 1 if variant == "t frozen at 1" else t
    lr_t = f(lr) if variant == "no bias correction" else f(step_size(tt, lr, b1, b2))
    with np.errstate(all="ignore"):
        if variant == "clip before scale":
            gi = np.clip(g, -clip, clip) * s
        elif variant == "scale ignored":
            gi = np.clip(g, -clip, clip)
        elif variant == "clip by norm":
            gi = g * s
            norm = f(np.sqrt((gi.astype(np.float64) ** 2).sum()))
            gi = gi * min(f(1), clip / norm) if norm > 0 else gi
        else:
            gi = np.clip(g * s, -clip, clip)
        bm = b2 if variant == "m updated with b2" else b1
        mi = bm * m + (f(1) - bm) * gi
        vi = b2 * v + (f(1) - b2) * gi * gi
        if variant == "eps inside the root":
            den = np.sqrt(vi + eps)
        elif variant == "eps dropped":
            den = np.sqrt(vi)
        else:
            den = np.sqrt(vi) + eps
        pn = p - lr_t * mi / den
    return dict(p=pn.astype(f), m=mi.astype(f), v=vi.astype(f))
