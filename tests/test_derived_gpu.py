"""Parameters to operands on the device (run with -m gpu on an MI355X): every array `kl_prepare`, `prepare_incremental`,
`prepare_big_step` and the comb-table build derive from the flat parameter vector, read back through `kl_test_derived_view`
and held to its definition in tests/derived_ref.py -- bit for bit where it is a conversion, a copy or a permutation, to the
thin GEMM's own bounds (array-wise AND row-wise) for EK, to the FMA chain's operation count for CtxK.  All cases go through
the C ABI (kl_create / kl_bind / kl_prepare) with parameters of order 0.1 - 1 and a derived buffer pre-filled with 0xA5 bytes,
so that a padding row nobody wrote, a plane left over from an earlier precision or a table not rebuilt after an update is
not accidentally right.  The lazy groups are built through `kl_test_prepare_lazy`; only what the view calls current is
compared.

The largest EK / CtxK ratios (difference over bound) per case and precision are printed and written to
profiles/derived_operands_error.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import derived_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "derived_operands_error.json")
KL_ERR_SHAPE = 1

# depth, width, V, n_ctx -- the smallest shapes that reach each edge
CASES = {
    "a": (2, 64, 50, 1),       # Vp = 64 > V: padding in E, ET, EF, Ecat; exactly one 64-tile per side
    "b": (3, 96, 30, 2),       # ragged 64 x 64 tiles (96, 384 = 6 x 64, Vp = 32); the second context variable's K0 rows; KF of two layers
    "c": (6, 32, 33, 1),       # 26 conversion jobs: the flush at 24 and the two after it; Vp = 64, V odd
    "d": (2, 512, 40, 1),      # the gate-interleaved set and comb (40 x 200 rows, 33 MB) in bf16 precision
    "e": (1, 128, 256, 0),     # no context tables; V == Vp
}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Bound:
    """a handle with its parameter vector and derived buffer, through the C ABI alone"""

    def __init__(self, sh):
        import torch
        from ocrd_keraslm_amd.lib import hipabi
        self.torch, self.hipabi, self.sh = torch, hipabi, sh
        self.lib = hipabi.load()
        self.cfg = hipabi.KlConfig(sh.depth, sh.width, sh.voc_size, sh.n_ctx, sh.ctx_vocab, sh.ctx_dim)
        self.handle = self.lib.kl_create(C.byref(self.cfg))
        assert self.handle
        self.n_params = D.layout(sh)[1]
        assert self.lib.kl_param_count(C.byref(self.cfg)) == self.n_params
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device="cuda")
        nbytes = self.lib.kl_derived_bytes(self.handle)
        self.derived = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        hipabi.check(self.lib.kl_bind(self.handle, _ptr(self.params), _ptr(self.derived), nbytes), "kl_bind")

    def close(self):
        self.torch.cuda.synchronize()
        self.lib.kl_destroy(self.handle)
        self.handle = None

    def set_params(self, p):
        self.params.copy_(self.torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)))

    def prepare(self, precision):
        self.hipabi.check(self.lib.kl_prepare(self.handle, precision, None), "kl_prepare")

    def lazy(self, mask):
        return self.lib.kl_test_prepare_lazy(self.handle, mask, None)

    def view(self):
        v = self.hipabi.KlDerivedView()
        self.hipabi.check(self.lib.kl_test_derived_view(self.handle, C.byref(v)), "kl_test_derived_view")
        return v

    def build_all(self):
        """every lazy group the shape has; returns the view"""
        self.hipabi.check(self.lazy(3), "kl_test_prepare_lazy")
        v = self.view()
        if v.has_comb and v.current & D.INTERLEAVED:
            self.hipabi.check(self.lazy(4), "kl_test_prepare_lazy")
        else:
            assert self.lazy(4) == KL_ERR_SHAPE      # comb not carved, or the interleaved tables it sums not current
        return self.view()

    def compare(self, params, view=None, where=""):
        view = view or self.view()
        self.torch.cuda.synchronize()
        sh, got = D.read_derived(view, self.derived.cpu().numpy())
        return D.compare(sh, params, view.precision, view.current, got, where=where), got


def _expected_names(sh, view):
    """what a full comparison must have looked at"""
    L, names = sh.depth, []
    for l in range(L):
        names += ["%s[%d]" % (n, l) for n in ("UT_hi", "KT_hi", "Un", "Kn", "UF", "WTcat", "WTperm")]
        if l > 0:
            names.append("KF[%d]" % l)
    names += ["E_hi", "ET", "EK", "EF", "Ecat"] + ["CtxK[%d]" % n for n in range(sh.n_ctx)]
    if view.precision == D.PREC_SPLIT:
        names += ["%s[%d]" % (n, l) for l in range(L) for n in ("UT_lo", "KT_lo")] + ["E_lo"]
    if view.current & D.INTERLEAVED:
        names += ["%s[%d]" % (n, l) for l in range(1, L) for n in ("KTp", "bp")] + ["EKp"] + ["CtxKp[%d]" % n for n in range(sh.n_ctx)]
    if view.current & D.COMB:
        names.append("comb")
    return set(names)


def _report(case, precision, stats):
    print("derived operands, case %s, precision %d: largest difference / bound -- EK array %.4f, EK row %.4f, CtxK %.4f"
          % (case, precision, stats.get("EK_array", 0.0), stats.get("EK_row", 0.0), stats.get("CtxK", 0.0)))
    try:
        data = json.load(open(REPORT))
    except (OSError, ValueError):
        data = {}
    data.setdefault("what", "largest |device - f64 reference| / bound of EK (thin GEMM: 3e-5 split, 1e-5 bf16, of the array's and of "
                            "each row's largest entry) and CtxK ((ctx_dim + 1) 2^-24 sum |a||k|), tests/test_derived_gpu.py")
    data.setdefault("cases", {})["%s/%s" % (case, "split" if precision == D.PREC_SPLIT else "bf16")] = {
        k: round(float(v), 6) for k, v in sorted(stats.items())}
    try:
        with open(REPORT, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:      # (a read-only checkout: the figures are printed above)
        pass


@pytest.mark.parametrize("case", sorted(CASES))
def test_derived_operands(case):
    """each case in both precisions, with DIFFERENT parameters for the second: whatever the second preparation does not
    rewrite is then wrong, not merely old"""
    sh = D.Shape(*CASES[case])
    m = Bound(sh)
    try:
        v0 = m.view()
        assert v0.current == 0 and v0.precision == 0 and v0.bytes == m.derived.numel()
        assert (v0.depth, v0.width, v0.voc_size, v0.Vp, v0.n_ctx, v0.ctx_vocab, v0.ctx_dim) == (
            sh.depth, sh.width, sh.voc_size, sh.Vp, sh.n_ctx, sh.ctx_vocab, sh.ctx_dim)
        assert m.lazy(3) == 3      # KL_ERR_STATE: nothing prepared
        for step, precision in enumerate((D.PREC_SPLIT, D.PREC_BF16)):
            params = D.random_params(sh, 100 * step + ord(case))
            m.set_params(params)
            m.prepare(precision)
            v = m.view()
            want = D.EAGER | (D.LO if precision == D.PREC_SPLIT else 0) | (D.INTERLEAVED if precision == D.PREC_BF16 and sh.width == 512 else 0)
            assert v.current == want and v.precision == precision, (v.current, want)
            v = m.build_all()
            want |= D.INC | D.BIG | (D.COMB if (want & D.INTERLEAVED) and v.has_comb else 0)
            assert v.current == want, (v.current, want)
            assert bool(v.has_comb) == (sh.width == 512 and sh.n_ctx == 1)
            out, _ = m.compare(params, v, where="case %s, precision %d" % (case, precision))
            assert set(out["checked"]) == _expected_names(sh, v), set(out["checked"]) ^ _expected_names(sh, v)
            _report(case, precision, out["stats"])
    finally:
        m.close()


def test_split_bf16_split_refreshes_every_lo_plane():
    """split, then bf16, then split with other parameters each time: every lo plane -- and every array built from one: the
    fragments' second plane, the third block of WTcat / WTperm / Ecat -- must be that of the LAST parameters"""
    sh = D.Shape(*CASES["b"])
    m = Bound(sh)
    try:
        for step, precision in enumerate((D.PREC_SPLIT, D.PREC_BF16, D.PREC_SPLIT)):
            params = D.random_params(sh, 40 + step)
            m.set_params(params)
            m.prepare(precision)
            v = m.build_all()
            assert bool(v.current & D.LO) == (precision == D.PREC_SPLIT)
            out, _ = m.compare(params, v, where="preparation %d, precision %d" % (step, precision))
        assert {"UT_lo[2]", "KT_lo[0]", "E_lo", "UF[0]", "KF[2]", "EF", "WTcat[1]", "Ecat"} <= set(out["checked"])
    finally:
        m.close()


def test_adam_step_rebuilds_the_eager_set_and_clears_the_lazy_flags():
    """kl_adam_step with a non-zero gradient: the eager set matches the UPDATED parameters bit for bit, the view reports the
    lazy groups as no longer current, and kl_step_batch / kl_test_prepare_lazy then build them from the updated parameters"""
    import torch
    sh = D.Shape(*CASES["a"])
    m = Bound(sh)
    try:
        p0 = D.random_params(sh, 7)
        m.set_params(p0)
        m.prepare(D.PREC_SPLIT)
        v = m.build_all()
        assert v.current & D.INC and v.current & D.BIG
        m.compare(p0, v, where="before the update")
        rng = np.random.default_rng(8)
        grads = torch.from_numpy(D.random_params(sh, 8)).cuda()      # (every entry 0.1 .. 1 in size: no entry's step is lost in eps)
        mom, var = torch.zeros_like(grads), torch.zeros_like(grads)
        m.hipabi.check(m.lib.kl_adam_step(m.handle, _ptr(grads), _ptr(mom), _ptr(var), 1, 0.05, 0.9, 0.999, 1e-7, 1.0, None), "kl_adam_step")
        torch.cuda.synchronize()
        p1 = m.params.cpu().numpy()
        assert np.abs(p1 - p0).min() > 0.01      # (Adam's first step moves every entry by about lr = 0.05: many bf16 ulps of 0.1 .. 1)
        v = m.view()
        assert v.current == D.EAGER | D.LO, v.current      # inc_ready / big_ready cleared
        out, _ = m.compare(p1, v, where="after kl_adam_step")
        assert "UF[0]" not in out["checked"] and "WTcat[0]" not in out["checked"] and "UT_lo[1]" in out["checked"]
        # one incremental step (24 hypotheses: step_small.hip's kernels) builds the fragment-major operands on its way
        n, L, W = 24, sh.depth, sh.width
        pool = torch.zeros((2 * n, 2 * L, W), dtype=torch.float32, device="cuda")
        idx = torch.from_numpy(rng.integers(0, sh.voc_size, n).astype(np.int32)).cuda()
        ctx = torch.from_numpy(rng.integers(0, sh.ctx_vocab, (n, 1)).astype(np.int32)).cuda()
        slot_in = torch.arange(n, dtype=torch.int32, device="cuda")
        slot_out = torch.arange(n, 2 * n, dtype=torch.int32, device="cuda")
        probs = torch.zeros((n, sh.voc_size), dtype=torch.float32, device="cuda")
        nws = m.lib.kl_step_workspace_bytes(m.handle, n)
        ws = torch.zeros(max(nws, 256), dtype=torch.uint8, device="cuda")
        m.hipabi.check(m.lib.kl_step_batch(m.handle, n, _ptr(idx), _ptr(ctx), _ptr(pool), _ptr(slot_in), _ptr(slot_out), _ptr(probs),
                                           _ptr(ws), ws.numel(), None), "kl_step_batch")
        torch.cuda.synchronize()
        assert abs(float(probs.sum().item()) - n) < 1e-3
        v = m.view()
        assert v.current == D.EAGER | D.LO | D.INC, v.current
        out, _ = m.compare(p1, v, where="after kl_step_batch")
        assert {"UF[0]", "UF[1]", "KF[1]", "EF"} <= set(out["checked"])
        # ... and the gather + GEMM path's operands through the hook
        m.hipabi.check(m.lazy(2), "kl_test_prepare_lazy")
        v = m.view()
        assert v.current == D.EAGER | D.LO | D.INC | D.BIG, v.current
        out, _ = m.compare(p1, v, where="after kl_test_prepare_lazy(2)")
        assert {"WTcat[0]", "WTcat[1]", "WTperm[1]", "Ecat"} <= set(out["checked"])
    finally:
        m.close()


def _pad_params(shp, W, w):
    """logical weights (Keras shapes at width W) -> the flat parameter vector at the padded width shp.width: hidden unit u of
    gate g sits in column g * Wp + u, the context rows of K0 behind the Wp embedding rows, zeros everywhere else"""
    Wp = shp.width
    flat = np.zeros(D.layout(shp)[1], dtype=np.float32)
    P = D.weights(shp, flat)      # views into flat
    P["E"][:, :W] = w["E"]
    for n in range(shp.n_ctx):
        P["Ctx%d" % n][:] = w["Ctx%d" % n]
    for l in range(shp.depth):
        for g in range(4):
            cols = slice(g * Wp, g * Wp + W)
            P["K%d" % l][:W, cols] = w["K%d" % l][:W, g * W:(g + 1) * W]
            if l == 0:
                P["K0"][Wp:, cols] = w["K0"][W:, g * W:(g + 1) * W]
            P["U%d" % l][:W, cols] = w["U%d" % l][:, g * W:(g + 1) * W]
            P["b%d" % l][0, cols] = w["b%d" % l].reshape(-1)[g * W:(g + 1) * W]
    return flat


def test_padded_width_units_are_exactly_zero():
    """the engine's padded widths (logical 80 on the kernels' 128): the rows and columns of the padded hidden units are
    exactly zero in every derived array, and the logical part is the reference of the unpadded weights"""
    from ocrd_keraslm_amd.lib import hipabi
    from ocrd_keraslm_amd.lib.engine import HipLM, physical_width
    L, W, V, n_ctx = 2, 80, 50, 1
    Wp = physical_width(W)
    assert Wp > W and Wp % 32 == 0
    lm = HipLM(L, W, V, n_ctx)
    lm.derived.fill_(0xA5)
    rng = np.random.default_rng(3)
    w = {name: (rng.uniform(0.1, 1.0, lm._logical_shape(name)) * rng.choice([-1.0, 1.0], lm._logical_shape(name))).astype(np.float32)
         for name, _o, _r, _c in lm.layout}
    lm.set_weights(w, hipabi.KL_PREC_SPLIT)
    lm.prepare_lazy(hipabi.KL_LAZY_INC | hipabi.KL_LAZY_BIG)
    view, derived = lm.derived_view()
    shp = D.Shape(L, Wp, V, n_ctx)
    params = _pad_params(shp, W, w)
    assert np.array_equal(lm.params.cpu().numpy(), params)      # the engine's padding against this file's own
    sh, got = D.read_derived(view, derived.cpu().numpy())
    assert (sh.width, view.current) == (Wp, D.EAGER | D.LO | D.INC | D.BIG)
    out = D.compare(sh, params, view.precision, view.current, got, where="width %d on %d" % (W, Wp))
    _report("padded-80", view.precision, out["stats"])
    # the padding itself, stated directly: unit u >= W of any gate, as a row or as a column
    unit = np.arange(4 * Wp) % Wp >= W
    for l in range(L):
        for name in ("UT_hi", "UT_lo", "KT_hi", "KT_lo"):
            a = got["%s[%d]" % (name, l)]
            assert not a[unit].any() and not a[:, W:].any(), (name, l)
        for name in ("Un", "Kn"):
            a = got["%s[%d]" % (name, l)]
            assert not a[W:].any() and not a[:, unit].any(), (name, l)
    assert not got["E_hi"][:, W:].any() and not got["E_lo"][:, W:].any() and not got["ET"][W:].any()
    assert not got["EK"][:, unit].any() and not got["CtxK[0]"][:, unit].any()


@pytest.mark.parametrize("tab", ["1", "0"])
def test_out_of_range_ids_read_clamped(monkeypatch, tab):
    """Layer 0 of the width-512 training forward reads ids clamped to their tables on every route (include/keraslm_hip.h, at
    kl_forward_window): a bf16 validation window whose context column holds ctx_vocab and -1 on some streams and whose
    characters hold V on others returns probabilities bitwise equal to the window with ctx_vocab - 1, 0 and V - 1 in their
    places.  tab = 1: the eight-wave scan gathering from the table of all (character, context value) sums, whose row
    numbers rows_tm_kernel computes; tab = 0: the 16-wave scan's table mode (ids_tm_kernel)."""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    from ocrd_keraslm_amd.lib.engine import CTX_VOCAB, HipLM
    from tests.gradcheck import cached_weights
    monkeypatch.setenv("KL_SCAN2_ROWS", "32")
    monkeypatch.setenv("KL_FWD8_TAB", tab)
    depth, width, V, B, T = 1, 512, 64, 2048, 3
    lm = HipLM(depth, width, V, 1)
    lm.set_weights(cached_weights(depth, width, V, 1, 4, 0.3), hipabi.KL_PREC_BF16)
    rng = np.random.default_rng(9)
    idx = rng.integers(0, V, (B, T))
    ctx = rng.integers(0, CTX_VOCAB, (B, 1, 1)).repeat(T, axis=1)
    bad_idx, bad_ctx = idx.copy(), ctx.copy()
    good_idx, good_ctx = idx.copy(), ctx.copy()
    bad_ctx[[3, 700, 2047]], good_ctx[[3, 700, 2047]] = CTX_VOCAB, CTX_VOCAB - 1
    bad_ctx[[16, 1029], 1:], good_ctx[[16, 1029], 1:] = -1, 0
    bad_idx[[5, 1500]], good_idx[[5, 1500]] = V, V - 1
    bad_idx[0, 2], good_idx[0, 2] = V + 7, V - 1
    # (row V - 1 with context 199 is the table's LAST row: one past it is beyond the table)
    bad_idx[2046], good_idx[2046], bad_ctx[2046], good_ctx[2046] = V - 1, V - 1, CTX_VOCAB, CTX_VOCAB - 1
    hipabi.check(lm.lib.kl_trace_enable(lm.handle, 1))
    lm.reset_states(B)
    want = lm.forward_window(good_idx, good_ctx).cpu().numpy()
    torch.cuda.synchronize()
    name = lm.lib.kl_trace_kernel_name(lm.handle, 0).decode()
    hipabi.check(lm.lib.kl_trace_enable(lm.handle, 0))
    assert name == ("lstm_scan_fwd8_kernel" if tab == "1" else "lstm_scan_fwd_wide2_kernel"), name
    lm.reset_states(B)
    got = lm.forward_window(bad_idx, bad_ctx).cpu().numpy()
    assert np.isfinite(want).all() and abs(float(want.sum()) - B * T) < 1e-2 * B * T
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:4]
    # ... and the clamped rows are not the rows the unclamped row number would name (the test would otherwise prove nothing)
    lm.reset_states(B)
    other_ctx = good_ctx.copy()
    other_ctx[[3, 700, 2047]] = 0      # idx * 200 + 200 = the NEXT character's row 0: context value 0
    other = lm.forward_window(good_idx, other_ctx).cpu().numpy()
    assert (other[[3, 700, 2047]] != want[[3, 700, 2047]]).any()
