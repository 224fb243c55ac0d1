"""The output-layer kernels of a training window, each through its own launcher (kl_test_softmax_ce, kl_test_logits_ce_ws,
kl_test_logits_ce_w128, kl_test_dh_ws) against tests/output_layer_ref.py (numpy, f64) on the same bf16 operands.

Every case carries random rows, padded targets (-1, 15 % anywhere plus a whole stream), two dummy streams (-2), both window
modes, an inv_count that is no power of two, two peaked rows (clipped on either side: no gradient, the clipped loss) and
three rows whose maximum is an exact tie between character 0 and a character of another 16-character tile (E[v2] = E[0]
bitwise: targets 0 = hit, v2 = no hit, -1 = hit).

Bounds (derived, not tuned): dlogits and a bf16 dH carry one bf16 rounding (eight significant bits: at most 2^-8 relative); the softmax is f32
with fast exponentials whose argument error at |z| <= 40 stays below 3e-6 relative; a contraction of K products summed in
f32 is off by at most K 2^-24 sum|a||b|.
  |dlogits - ref| <= 2^-8 |ref| + 2e-5 inv_count          |loss - ref| <= 1e-5 |ref| + 2e-5 inv_count
  bf16 dH from the device's own dlogits: 2^-8 |ref| + K 2^-24 sum|a||b|;  f32 dH (width 128): 2^-23 |ref| + K 2^-24 sum|a||b|
  dH from the REFERENCE's bf16 dlogits: the device's dlogits differ from those by the dlogits bound per element, so the
    bound above grows by sum_v (2^-8 |dl_v| + 2e-5 inv_count) |E_v|
  hit exact; pad columns of dlogits bitwise zero; rows beyond M untouched.
Left out, each from one comparison only and at most 1 % of the rows (asserted on the reference alone): rows whose two
largest reference logits are closer than 1e-3 without being equal (hit), rows whose reference p_t or 1 - p_t lies within
a factor 2 of 1e-7 (dlogits, dH from the reference's dlogits)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import lstm_oracle as O
from tests.output_layer_ref import dh_ref, logits_ref, softmax_ce_ref

pytestmark = pytest.mark.gpu

KL_ERR_SHAPE = 1
PAD = 8                       # rows behind the M the call is given: they keep their sentinel
SENT16 = 0x5A5A
SENT32 = np.float32(-12345.5)
_STATS = {}


def _bf16(x):
    return O.bf16_round(np.asarray(x, np.float32)).astype(np.float64)


def _bits(x):
    """bf16 values -> their 16 bits"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _vals(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _note(kernel, key, value):
    s = _STATS.setdefault(kernel, {})
    s[key] = max(s.get(key, 0.0), float(value))


def _report(kernel):
    print("%s: largest observed / bound and shares left out: %s" % (kernel, {k: round(v, 4) for k, v in sorted(_STATS.get(kernel, {}).items())}))


def _tie_partner(V):
    return 66 if V > 66 else 3      # another 16-character tile where the vocabulary has one; lane group 0 (characters 64 k + 0 .. 3)


def _near(r):
    """the rows the comparisons may leave out, from the reference alone"""
    band = lambda q: (q > 0.5e-7) & (q < 2e-7)
    return r["valid"] & (band(r["pt"]) | band(r["one_minus_pt"])), (r["gap"] < 1e-3) & (r["gap"] != 0)


@functools.lru_cache(maxsize=3)
def _inputs(W, V, Vp, B, T):
    """-> X [M][W], E [Vp][W] (bf16 values as f64; rows of E from V on are zero), tgt [B][T], the built rows.
    Drawn again (next seed) until the REFERENCE leaves out at most 1 % of the rows from either comparison -- at up to
    2000 rows: until it has no near-tie at all, so that sums of hits can be compared too.  The device plays no part."""
    base = zlib.crc32(repr((W, V, Vp, B, T)).encode())
    for attempt in range(16):
        drawn = _draw(np.random.default_rng([base, attempt]), W, V, Vp, B, T)
        r = softmax_ce_ref(logits_ref(drawn[0], drawn[1], V), drawn[2], 1.0)
        near_clip, near_tie = _near(r)
        if near_clip.mean() <= 0.01 and near_tie.mean() <= 0.01 and (B * T > 2000 or not near_tie.any()):
            return drawn
    raise AssertionError("no acceptable draw")


def _draw(rng, W, V, Vp, B, T):
    M = B * T
    assert B >= 16
    X = _bf16(rng.uniform(-1, 1, (M, W)))
    E = np.zeros((Vp, W))
    E[:V] = _bf16(rng.standard_normal((V, W)) * (2.5 / np.sqrt(W / 3.0)))      # logits: standard deviation 2.5
    v1, v2 = 0, _tie_partner(V)
    E[v2] = E[v1]
    v_peak = V - 1 if V - 1 != v2 else V - 2
    tgt = rng.integers(0, V, (B, T))
    tgt[rng.random((B, T)) < 0.15] = -1
    tgt[2] = -1                                  # a whole padded stream
    tgt[1] = tgt[B - 1] = -2                     # two dummy streams
    c = 1.0
    while True:                                  # the smallest power of two that peaks the row beyond the clip
        z = (c * E[v_peak]) @ E[:V].T
        e = np.exp(z - z.max())
        if z.argmax() == v_peak and (e.sum() - e[v_peak]) / e.sum() < 1e-9:
            break
        c *= 2
        assert c <= 64
    row = lambda b: (T - 1) * B + b              # (the last step: these rows count in both window modes)
    built = {"peak_hit": row(3), "peak_miss": row(4), "tie_v1": row(5), "tie_v2": row(6), "tie_pad": row(7)}
    X[row(3)] = c * E[v_peak]; tgt[3, T - 1] = v_peak
    X[row(4)] = c * E[v_peak]; tgt[4, T - 1] = 1
    X[row(5)] = E[v1]; tgt[5, T - 1] = v1
    X[row(6)] = 0.5 * E[v1]; tgt[6, T - 1] = v2
    X[row(7)] = E[v1]; tgt[7, T - 1] = -1
    for a in (X, E, tgt):
        a.setflags(write=False)
    return X, E, tgt, built, (v1, v2)


def _inv_count(M):
    return float(np.float32(1.0 / (M - 3)))      # (no power of two: what kl_set_loss_rows makes of a padded batch)


@functools.lru_cache(maxsize=4)
def _reference(W, V, Vp, B, T, last_only, ld_dl, f32_logits=False):
    X, E, tgt, built, (v1, v2) = _inputs(W, V, Vp, B, T)
    z = logits_ref(X, E, V)
    if f32_logits:                               # (the softmax kernels read f32 logits: the reference reads the same numbers)
        z = z.astype(np.float32).astype(np.float64)
    inv = _inv_count(B * T)
    r = softmax_ce_ref(z, tgt, inv, last_only, ld_dl)
    # the built rows are what they are meant to be, on the reference alone
    for k in ("peak_hit", "peak_miss"):
        assert not r["active"][built[k]] and (r["dlogits"][built[k]] == 0).all()
    assert r["one_minus_pt"][built["peak_hit"]] < 1e-9 and r["pt"][built["peak_miss"]] < 1e-9
    assert abs(r["loss"][built["peak_hit"]] - -np.log(1 - 1e-7) * inv) < 1e-20 and r["hit"][built["peak_hit"]] == inv
    assert abs(r["loss"][built["peak_miss"]] - -np.log(1e-7) * inv) < 1e-20 and r["hit"][built["peak_miss"]] == 0
    for k in ("tie_v1", "tie_v2", "tie_pad"):
        assert r["gap"][built[k]] == 0 and r["amax"][built[k]] == v1 and z[built[k], v1] == z[built[k], v2]
    assert r["hit"][built["tie_v1"]] == inv and r["hit"][built["tie_v2"]] == 0 and r["hit"][built["tie_pad"]] == inv
    r["near_clip"], r["near_tie"] = _near(r)
    assert r["near_clip"].mean() <= 0.01 and r["near_tie"].mean() <= 0.01, (r["near_clip"].sum(), r["near_tie"].sum())
    assert not r["near_clip"][list(built.values())].any() and not r["near_tie"][list(built.values())].any()
    r["z"] = z
    return r


class _Dev:
    def __init__(self):
        import torch
        from ocrd_keraslm_amd.lib import hipabi
        self.torch, self.lib = torch, hipabi.load()

    def up(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        return self.torch.from_numpy(a).cuda()

    def fill16(self, rows, cols):
        return self.torch.full((rows, cols), SENT16, dtype=self.torch.int16, device="cuda")

    def fill32(self, rows, cols):
        return self.torch.full((rows, cols), float(SENT32), dtype=self.torch.float32, device="cuda")

    def down16(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint16)

    def down32(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _untouched(*arrays16_then32):
    for a in arrays16_then32:
        if a.dtype == np.uint16:
            assert (a == SENT16).all()
        else:
            assert (a == SENT32).all()


def _check_ce(kernel, r, M, V, inv, dl_bits, rowstat):
    """dlogits (bits, [M + PAD][ld_dl]) and rowstat ([M + PAD][2]) of one call against the reference r"""
    _untouched(dl_bits[M:], rowstat[M:])
    assert (dl_bits[:M, V:] == 0).all(), "pad columns of dlogits"
    dl = _vals(dl_bits[:M])
    ref = r["dlogits"]
    keep = ~r["near_clip"]
    ratio = np.abs(dl - ref) / (2.0 ** -8 * np.abs(ref) + 2e-5 * inv)
    _note(kernel, "dlogits", ratio[keep].max())
    _note(kernel, "share near the clip", r["near_clip"].mean())
    _note(kernel, "share near a tie", r["near_tie"].mean())
    bad = np.argwhere(ratio[keep] > 1)
    assert bad.size == 0, ("dlogits", ratio[keep].max(), bad[:5])
    loss, hit = rowstat[:M, 0].astype(np.float64), rowstat[:M, 1]
    lratio = np.abs(loss - r["loss"]) / (1e-5 * np.abs(r["loss"]) + 2e-5 * inv)
    _note(kernel, "loss", lratio.max())
    assert lratio.max() <= 1, ("loss", lratio.max(), int(lratio.argmax()))
    assert np.isin(hit, (np.float32(0), np.float32(inv))).all()
    k2 = ~r["near_tie"]
    assert np.array_equal(hit[k2] != 0, r["hit"][k2] != 0), ("hit", np.flatnonzero((hit != 0) != (r["hit"] != 0))[:8])
    return dl


def _built_rows_have_no_gradient(W, V, Vp, B, T, dl_bits):
    built = _inputs(W, V, Vp, B, T)[3]
    for k in ("peak_hit", "peak_miss"):
        assert (_vals(dl_bits[built[k]]) == 0).all(), k


# ---------------------------------------------------------------- logits_ce_ws_kernel (width 512, V = 256)
@pytest.mark.parametrize("B,T", [(1024, 8), (256, 33)])      # 256 tiles on 256 workgroups / 264: eight take a second one, row % B crosses tiles
def test_logits_ce_ws(B, T):
    d = _Dev()
    W, V, M = 512, 256, B * T
    X, E, tgt, _built, _ = _inputs(W, V, V, B, T)
    inv = _inv_count(M)
    Xd, Ed, td = d.up(_bits(X)), d.up(_bits(E)), d.up(tgt.astype(np.int32))
    for last_only in (0, 1):
        r = _reference(W, V, V, B, T, last_only, V)
        dl, rs = d.fill16(M + PAD, V), d.fill32(M + PAD, 2)
        assert d.lib.kl_test_logits_ce_ws(_p(Xd), _p(Ed), _p(td), _p(dl), _p(rs), B, T, inv, last_only, None) == 0
        dlb = d.down16(dl)
        _check_ce("logits_ce_ws", r, M, V, inv, dlb, d.down32(rs))
        _built_rows_have_no_gradient(W, V, V, B, T, dlb)
    _report("logits_ce_ws")


@pytest.mark.parametrize("B,T", [(1020, 8), (1026, 8)])      # M = 8160: below the minimum; 8208 = 8192 + 16: no multiple of 32
def test_logits_ce_ws_refuses(B, T):
    d = _Dev()
    M = B * T
    Xd, Ed, td = d.up(np.zeros((M, 512), np.uint16)), d.up(np.zeros((256, 512), np.uint16)), d.up(np.zeros((B, T), np.int32))
    dl, rs = d.fill16(M, 256), d.fill32(M, 2)
    assert d.lib.kl_test_logits_ce_ws(_p(Xd), _p(Ed), _p(td), _p(dl), _p(rs), B, T, 0.01, 0, None) == KL_ERR_SHAPE
    _untouched(d.down16(dl), d.down32(rs))


# ---------------------------------------------------------------- dh_ws_kernel (width 512, Vp = 256)
@pytest.mark.parametrize("V", [256, 230])
@pytest.mark.parametrize("B,T", [(512, 8), (516, 8)])        # M = 4096: one tile per row group; 4128: one group takes a second
def test_dh_ws(B, T, V):
    d = _Dev()
    W, Vp, M = 512, 256, B * T
    _X, E, _tgt, _built, _ = _inputs(W, V, Vp, B, T)
    r = _reference(W, V, Vp, B, T, 0, Vp)
    dl = _bf16(r["dlogits"])                     # (pad columns zero, as are the rows of E from V on)
    assert (dl[:, V:] == 0).all() and (E[V:] == 0).all()
    out, dld, ETd = d.fill16(M + PAD, W), d.up(_bits(dl)), d.up(_bits(E.T))
    assert d.lib.kl_test_dh_ws(_p(dld), _p(ETd), _p(out), M, None) == 0
    ob = d.down16(out)
    _untouched(ob[M:])
    ref, mag = dh_ref(dl, E)
    ratio = np.abs(_vals(ob[:M]) - ref) / (2.0 ** -8 * np.abs(ref) + Vp * 2.0 ** -24 * mag + 1e-300)
    _note("dh_ws", "dH", ratio.max())
    assert ratio.max() <= 1, (ratio.max(), np.argwhere(ratio > 1)[:5])
    assert np.abs(ref).max() > 0
    _report("dh_ws")


def test_dh_ws_refuses():
    d = _Dev()
    M = 4064
    out, dld, ETd = d.fill16(M, 512), d.up(np.zeros((M, 256), np.uint16)), d.up(np.zeros((512, 256), np.uint16))
    assert d.lib.kl_test_dh_ws(_p(dld), _p(ETd), _p(out), M, None) == KL_ERR_SHAPE
    _untouched(d.down16(out))


# ---------------------------------------------------------------- logits_ce_w128_kernel (width 128, V <= Vp <= 256)
# M = 64: one tile; 69: a ragged tile; 4101: 65 tiles, the last ragged; 16455: 258 tiles -- more than the 256 workgroups the
# launcher starts at most (one per compute unit), so some take a second tile, the ragged last one among them
W128_SHAPES = [(64, 1), (16, 4), (69, 1), (23, 3), (4101, 1), (1367, 3)]


@pytest.mark.parametrize("V,Vp,B,T", [(V, Vp, B, T) for V, Vp in [(256, 256), (230, 256), (200, 224), (97, 128), (5, 32)] for B, T in W128_SHAPES]
                         + [(230, 256, 5485, 3)])
def test_logits_ce_w128(V, Vp, B, T):
    d = _Dev()
    W, M = 128, B * T
    X, E, tgt, _built, _ = _inputs(W, V, Vp, B, T)
    inv = _inv_count(M)
    Xd, Ed, ETd, td = d.up(_bits(X)), d.up(_bits(E)), d.up(_bits(E.T)), d.up(tgt.astype(np.int32))
    for last_only in (0, 1):
        r = _reference(W, V, Vp, B, T, last_only, Vp)
        dl, dh, rs = d.fill16(M + PAD, Vp), d.fill32(M + PAD, W), d.fill32(M + PAD, 2)
        assert d.lib.kl_test_logits_ce_w128(_p(Xd), _p(Ed), _p(ETd), _p(td), _p(dl), _p(dh), _p(rs), B, T, V, Vp, inv, last_only, None) == 0
        dlb, dhv = d.down16(dl), d.down32(dh)
        got_dl = _check_ce("logits_ce_w128", r, M, V, inv, dlb, d.down32(rs))
        _built_rows_have_no_gradient(W, V, Vp, B, T, dlb)
        _untouched(dhv[M:])
        got = dhv[:M].astype(np.float64)
        ref, mag = dh_ref(got_dl, E)             # the contraction alone: from the device's own dlogits
        ratio = np.abs(got - ref) / (2.0 ** -23 * np.abs(ref) + Vp * 2.0 ** -24 * mag + 1e-300)
        _note("logits_ce_w128", "dH (own dlogits)", ratio.max())
        assert ratio.max() <= 1, ("dH from the device's dlogits", ratio.max(), np.argwhere(ratio > 1)[:5])
        ref_dl = _bf16(r["dlogits"])             # softmax and contraction together: from the reference's bf16 dlogits
        ref2, mag2 = dh_ref(ref_dl, E)
        bound2 = 2.0 ** -23 * np.abs(ref2) + Vp * 2.0 ** -24 * mag2 + 2.0 ** -8 * mag2 + 2e-5 * inv * np.abs(E[:V]).sum(axis=0)[None, :]
        keep = ~r["near_clip"]
        ratio2 = (np.abs(got - ref2) / bound2)[keep]
        _note("logits_ce_w128", "dH (reference's dlogits)", ratio2.max())
        assert ratio2.max() <= 1, ("dH from the reference's dlogits", ratio2.max())
    _report("logits_ce_w128")


def test_logits_ce_w128_refuses():
    d = _Dev()
    B, T, V, Vp = 64, 1, 270, 288
    z16 = lambda r, c: d.up(np.zeros((r, c), np.uint16))
    dl, dh, rs = d.fill16(B, Vp), d.fill32(B, 128), d.fill32(B, 2)
    Xd, Ed, ETd, td = z16(B, 128), z16(Vp, 128), z16(128, Vp), d.up(np.zeros((B, T), np.int32))
    rc = d.lib.kl_test_logits_ce_w128(_p(Xd), _p(Ed), _p(ETd), _p(td), _p(dl), _p(dh), _p(rs), B, T, V, Vp, 0.01, 0, None)
    assert rc == KL_ERR_SHAPE
    _untouched(d.down16(dl), d.down32(dh), d.down32(rs))


# ---------------------------------------------------------------- softmax_ce_kernel / softmax_ce_v256_kernel (f32 logits)
SM_B, SM_T = 343, 3           # 1029 rows = 4 * 257 + 1: the last workgroup holds one row


def _softmax_call(d, V, ld_dl, last_only):
    W, M = 128, SM_B * SM_T
    _X, _E, tgt, _built, _ = _inputs(W, V, V, SM_B, SM_T)
    r = _reference(W, V, V, SM_B, SM_T, last_only, ld_dl, True)
    inv = _inv_count(M)
    zd, td = d.up(r["z"].astype(np.float32)), d.up(tgt.astype(np.int32))
    dl, rs = d.fill16(M + PAD, ld_dl), d.fill32(M + PAD, 2)
    acc = d.torch.zeros(4, dtype=d.torch.float32, device="cuda")
    assert d.lib.kl_test_softmax_ce(_p(zd), V, M, V, _p(td), SM_B, SM_T, inv, _p(dl), ld_dl, _p(rs), _p(acc), last_only, None) == 0
    assert np.array_equal(d.down32(zd), r["z"].astype(np.float32))      # (with dlogits asked for, the logits stay as they are)
    return r, inv, d.down16(dl), d.down32(rs), d.down32(acc)


@pytest.mark.parametrize("V,ld_dl,kernel", [(230, 256, "softmax_ce"), (300, 320, "softmax_ce"), (7, 32, "softmax_ce"),
                                            (200, 224, "softmax_ce_v256"), (256, 256, "softmax_ce_v256"), (4, 32, "softmax_ce_v256")])
def test_softmax_ce(V, ld_dl, kernel):
    d = _Dev()
    M = SM_B * SM_T
    one_pass = V <= 256 and V % 4 == 0 and ld_dl % 4 == 0 and ld_dl <= 256      # (the launcher's rule, with ld = V)
    assert one_pass == (kernel == "softmax_ce_v256")
    for last_only in (0, 1):
        r, inv, dlb, rs, acc = _softmax_call(d, V, ld_dl, last_only)
        _check_ce(kernel, r, M, V, inv, dlb, rs)
        _built_rows_have_no_gradient(128, V, V, SM_B, SM_T, dlb)
        # the reduction of the row statistics against the rows it read
        assert abs(acc[0] - rs[:M, 0].astype(np.float64).sum()) <= 1e-5 * rs[:M, 0].astype(np.float64).sum()
        assert abs(acc[1] - rs[:M, 1].astype(np.float64).sum()) <= 1e-5 * rs[:M, 1].astype(np.float64).sum()
        assert acc[2] == 0 and acc[3] == 0
    _report(kernel)


@pytest.mark.parametrize("V,ld_dl", [(230, 256), (200, 224)])
def test_softmax_ce_sums(V, ld_dl):
    """loss_acc after the call (softmax + rowstat reduction) against the reference's f64 sums over the 1029 rows"""
    d = _Dev()
    for last_only in (0, 1):
        r, _inv, _dlb, _rs, acc = _softmax_call(d, V, ld_dl, last_only)
        assert not (r["near_tie"] & r["counts"]).any()      # (no row whose hit the reference cannot call)
        loss, hits = r["loss"].sum(), r["hit"].sum()
        assert loss > 0 and hits > 0
        assert abs(acc[0] - loss) <= 1e-5 * loss, (acc[0], loss)
        assert abs(acc[1] - hits) <= 1e-5 * hits, (acc[1], hits)
