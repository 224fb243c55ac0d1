"""Every operand array `kl_prepare` and its lazy companions derive from the parameters, stated in numpy from the flat
parameter vector, and the comparator that holds the arrays read back from the device to those statements.

No kernel on the hot path reads the parameters: they read the arrays `carve_derived` (csrc/api.hip) lays into the caller's
derived buffer, found here through `kl_test_derived_view`.  CPU only: used by tests/test_derived_ref.py (the comparator's own
sensitivity: one injected mistake at a time) and tests/test_derived_gpu.py (the kernels).

W = width, V = voc_size, Vp = V rounded up to 32, gate column order i, f, c, o; rne = round-to-nearest-even to bf16
(`f2bf`, csrc/kl_common.h); hi = rne(x), lo = rne(x - f32(hi)) (`split_bf16`).

BIT-EXACT (conversions, copies and permutations -- compared as uint16 / uint32 patterns, nothing to tolerate)
  UT_hi/lo[l], KT_hi/lo[l]  [4W][W]   hi / lo of U_l^T, K_l^T; layer 0: rows [0, W) of K0 only
  Un[l], Kn[l]              [W][4W]   hi of U_l, K_l (layer 0: rows [0, W) of K0)
  E_hi/lo [Vp][W], ET [W][Vp]          hi / lo of E, hi of E^T; rows / columns from V on exactly zero
  KTp[l], l >= 1            [4W][W]   row u*4+g = row g*W+u of KT_hi[l];  bp[l] f32 [4W] likewise from b_l
  EKp   f32 [V][W][4]                 EKp[v][u][g] = f32(EK[v][g*W+u] + b_0[g*W+u]) -- one f32 addition, so exact against EK AS READ BACK
  CtxKp[n] f32 [ctx_vocab][W][4]      the same permutation of CtxK[n] as read back
  comb  [V ctx_vocab][W][4]           comb[v ctx_vocab + c] = rne(f32(EKp[v] + CtxKp[0][c])), against those two as read back
  UF[l], KF[l] (l >= 1), EF           fragment-major [rows/16][K/32][planes][64][8] of UT, KT, E (the comment above frag_major_kernel,
                                      csrc/step_tile.hip): lane (c = lane % 16, q = lane / 16) of block (rt, kb) holds
                                      in[rt 16 + c][kb 32 + 8 q .. + 7]; one plane (hi) in bf16 precision, two (hi, lo) in split
  WTcat[l] [4W][3 K_l]                blocks [hi | hi | lo], K_0 = W (U^T), K_l = 2W (K^T then U^T); bf16 precision writes block 0 only
  WTperm[l]                           row (u/32) 128 + g 32 + u%32 = row g*W+u of WTcat[l] (kl_launch_permute_gate_rows, csrc/step_big.hip)
  Ecat [Vp][3W]                       [hi | hi | lo] of E (bf16 precision: block 0); rows from V on zero in all three blocks
A plane the current precision does not write is not asserted on; a group the view does not call current is not compared.

BOUNDED
  EK f32 [V][4W] = E . K0[:W] through the thin GEMM -- the two bounds tests/test_gpu_kernels.py::test_thin_gemm holds that
      kernel to: split precision EK_SPLIT = 3e-5 of the largest |entry| of the f64 product of the f32 operands, bf16 precision
      EK_BF16 = 1e-5 against the f64 product of the bf16-rounded operands.  Applied twice: against the ARRAY's largest
      entry, and per ROW against that row's own largest entry (same factors), so that the wrong row of a small-norm
      character cannot hide behind the array's maximum.  An entry whose terms are all zero (padded hidden units) must be zero.
  CtxK[n] f32 [ctx_vocab][4W] = Ctx_n . K0[W + n ctx_dim : W + (n+1) ctx_dim], a chain of ctx_dim f32 FMAs: per entry
      (ctx_dim + 1) 2^-24 sum_k |a_k| |k_k| against f64 -- from the operation count.

A failure names the array, the layer (or context variable), and the first offending (row, column) of the array as stored --
for the fragment-major arrays the (row, column) of the [rows][K] source it scrambles, with the plane.
"""
import numpy as np

from tests.test_gpu_kernels import bf16_bits, bits_to_f32

PREC_BF16, PREC_SPLIT = 1, 3
EAGER, LO, INTERLEAVED, INC, BIG, COMB = 1, 2, 4, 8, 16, 32      # kl_derived_view.current (include/keraslm_hip.h)
ALL_GROUPS = EAGER | LO | INTERLEAVED | INC | BIG | COMB
EK_SPLIT, EK_BF16 = 3e-5, 1e-5
U24 = 2.0 ** -24


class Shape:
    def __init__(self, depth, width, voc_size, n_ctx, ctx_vocab=200, ctx_dim=10):
        self.depth, self.width, self.voc_size, self.n_ctx = int(depth), int(width), int(voc_size), int(n_ctx)
        self.ctx_vocab, self.ctx_dim = int(ctx_vocab), int(ctx_dim)
        self.Vp = (self.voc_size + 31) // 32 * 32

    def __repr__(self):
        return "depth %d width %d V %d (Vp %d) n_ctx %d x [%d][%d]" % (self.depth, self.width, self.voc_size, self.Vp, self.n_ctx,
                                                                      self.ctx_vocab, self.ctx_dim)


def layout(sh):
    """name -> (offset, rows, cols) in the flat parameter vector (Keras weight order, include/keraslm_hip.h), and its length"""
    W, out, off = sh.width, {}, 0

    def put(name, rows, cols):
        nonlocal off
        out[name] = (off, rows, cols)
        off += rows * cols
    put("E", sh.voc_size, W)
    for n in range(sh.n_ctx):
        put("Ctx%d" % n, sh.ctx_vocab, sh.ctx_dim)
    for l in range(sh.depth):
        put("K%d" % l, W + sh.n_ctx * sh.ctx_dim if l == 0 else W, 4 * W)
        put("U%d" % l, W, 4 * W)
        put("b%d" % l, 1, 4 * W)
    return out, off


def weights(sh, params):
    lay, n = layout(sh)
    params = np.ascontiguousarray(params, dtype=np.float32)
    assert params.size == n, (params.size, n)
    return {k: params[o:o + r * c].reshape(r, c) for k, (o, r, c) in lay.items()}


def random_params(sh, seed):
    """non-trivial parameters: every entry of order 0.1 - 1 (not the tiny-variance embedding initialiser), so that a missing
    term, row or bias is many ulps"""
    rng = np.random.default_rng(seed)
    _, n = layout(sh)
    p = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)
    return p.astype(np.float32)


# ---------------------------------------------------------------- the definitions
def split(x):
    hi = bf16_bits(x)
    lo = bf16_bits(np.asarray(x, dtype=np.float32) - bits_to_f32(hi))
    return hi, lo


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def pad_rows(x, rows):
    out = np.zeros((rows,) + x.shape[1:], dtype=x.dtype)
    out[:x.shape[0]] = x
    return out


def interleave_rows(x, W):
    """out[u*4+g] = x[g*W+u]"""
    return x.reshape(4, W, -1).transpose(1, 0, 2).reshape(4 * W, -1)


def interleave_cols(x, W):
    """out[r][u*4+g] = x[r][g*W+u], as [R][4W]"""
    return x.reshape(x.shape[0], 4, W).transpose(0, 2, 1).reshape(x.shape[0], 4 * W)


def perm32_rows(x, W):
    """out[(u/32)*128 + g*32 + u%32] = x[g*W+u]"""
    return x.reshape(4, W // 32, 32, -1).transpose(1, 0, 2, 3).reshape(4 * W, -1)


def frag_major(planes):
    """planes: [npl][rows][K] uint16 -> [rows/16][K/32][npl][64][8]"""
    planes = np.asarray(planes)
    npl, rows, K = planes.shape
    a = planes.reshape(npl, rows // 16, 16, K // 32, 4, 8)          # (p, rt, c, kb, q, j)
    return np.ascontiguousarray(a.transpose(1, 3, 0, 4, 2, 5)).reshape(rows // 16, K // 32, npl, 64, 8)      # lane = q*16 + c


def unfrag(frag, rows, K):
    """the inverse: [rows/16][K/32][npl][64][8] -> [npl][rows][K]"""
    npl = frag.shape[2]
    a = frag.reshape(rows // 16, K // 32, npl, 4, 16, 8)            # (rt, kb, p, q, c, j)
    return np.ascontiguousarray(a.transpose(2, 0, 4, 1, 3, 5)).reshape(npl, rows, K)


def ek_reference(sh, w, precision):
    """(f64 reference, f64 sum of |terms|) of EK in the given precision"""
    W = sh.width
    E, K = w["E"], w["K0"][:W]
    if precision == PREC_BF16:
        E, K = bits_to_f32(bf16_bits(E)), bits_to_f32(bf16_bits(K))
    E, K = E.astype(np.float64), K.astype(np.float64)
    return E @ K, np.abs(E) @ np.abs(K)


def ctxk_reference(sh, w, n, k_rows_of=None):
    W, D = sh.width, sh.ctx_dim
    m = n if k_rows_of is None else k_rows_of
    A, K = w["Ctx%d" % n].astype(np.float64), w["K0"][W + m * D:W + (m + 1) * D].astype(np.float64)
    return A @ K, np.abs(A) @ np.abs(K)


def ekp_from(EK, b0, W):
    return interleave_cols((EK + b0.reshape(1, -1)).astype(np.float32), W)


def comb_from(EKp, CtxKp0):
    V, R = EKp.shape[0], CtxKp0.shape[0]
    return bf16_bits((EKp[:, None, :] + CtxKp0[None, :, :]).astype(np.float32)).reshape(V * R, -1)


def wtcat_from(sh, w, l, precision):
    """[4W][3 K_l] and the number of columns the precision writes"""
    W = sh.width
    uh, ul = split(w["U%d" % l].T)
    if l == 0:
        hi, lo = uh, ul
    else:
        kh, kl = split(w["K%d" % l].T)
        hi, lo = np.concatenate([kh, uh], axis=1), np.concatenate([kl, ul], axis=1)
    Kl = hi.shape[1]
    return np.concatenate([hi, hi, lo], axis=1), (3 * Kl if precision == PREC_SPLIT else Kl)


def build_exact(sh, params, precision, with_comb=True):
    """Every array as its definition gives it (EK and CtxK: the f64 products rounded to f32), whatever the device would carve
    or write at this shape: the comparator's clean input for tests/test_derived_ref.py."""
    W, V, Vp = sh.width, sh.voc_size, sh.Vp
    w = weights(sh, params)
    g = {}
    for l in range(sh.depth):
        K = w["K%d" % l][:W]
        g["UT_hi[%d]" % l], g["UT_lo[%d]" % l] = split(w["U%d" % l].T)
        g["KT_hi[%d]" % l], g["KT_lo[%d]" % l] = split(K.T)
        g["Un[%d]" % l], g["Kn[%d]" % l] = bf16_bits(w["U%d" % l]), bf16_bits(K)
        if l > 0:
            g["KTp[%d]" % l] = interleave_rows(g["KT_hi[%d]" % l], W)
            g["bp[%d]" % l] = interleave_cols(w["b%d" % l], W).reshape(-1).copy()
        planes = 2 if precision == PREC_SPLIT else 1
        g["UF[%d]" % l] = frag_major([g["UT_hi[%d]" % l], g["UT_lo[%d]" % l]][:planes])
        if l > 0:
            g["KF[%d]" % l] = frag_major([g["KT_hi[%d]" % l], g["KT_lo[%d]" % l]][:planes])
        g["WTcat[%d]" % l], _ = wtcat_from(sh, w, l, PREC_SPLIT)
        g["WTperm[%d]" % l] = perm32_rows(g["WTcat[%d]" % l], W)
    eh, el = split(w["E"])
    g["E_hi"], g["E_lo"] = pad_rows(eh, Vp), pad_rows(el, Vp)
    g["ET"] = np.ascontiguousarray(g["E_hi"].T)
    g["EF"] = frag_major([g["E_hi"], g["E_lo"]][:2 if precision == PREC_SPLIT else 1])
    g["Ecat"] = np.concatenate([g["E_hi"], g["E_hi"], g["E_lo"]], axis=1)
    g["EK"] = ek_reference(sh, w, precision)[0].astype(np.float32)
    g["EKp"] = ekp_from(g["EK"], w["b0"], W)
    for n in range(sh.n_ctx):
        g["CtxK[%d]" % n] = ctxk_reference(sh, w, n)[0].astype(np.float32)
        g["CtxKp[%d]" % n] = interleave_cols(g["CtxK[%d]" % n], W)
    if with_comb and sh.n_ctx > 0:
        g["comb"] = comb_from(g["EKp"], g["CtxKp[0]"])
    return g


# ---------------------------------------------------------------- the comparator
class DerivedMismatch(AssertionError):
    """`failures`: (array, layer, row, col, text) per failed check; `arrays`: the set of array names; `named`: (array, layer) pairs"""

    def __init__(self, failures, where=""):
        super().__init__("%s: %d derived arrays differ from their definition: %s"
                         % (where, len(failures), "; ".join("%s[%s] at (%s, %s): %s" % f for f in failures[:8])))
        self.failures = failures
        self.arrays = {f[0] for f in failures}
        self.named = {(f[0], f[1]) for f in failures}


def _first(bad):
    r, c = np.argwhere(bad)[0]
    return int(r), int(c)


class _Run:
    def __init__(self, got):
        self.got, self.fails, self.checked, self.stats = got, [], [], {}

    def have(self, key):
        return self.got.get(key) is not None

    def exact(self, name, layer, key, ref, cols=None, text="", bits=16):
        """got[key] == ref as bit patterns, on the first `cols` columns (None: all)"""
        got = self.got.get(key)
        if got is None:
            self.fails.append((name, layer, -1, -1, "not delivered"))
            return
        self.checked.append(key)
        dt = np.uint16 if bits == 16 else np.uint32
        got2 = np.ascontiguousarray(got).view(dt).reshape(ref.shape[0], -1)
        ref2 = np.ascontiguousarray(ref).view(dt).reshape(ref.shape[0], -1)
        if got2.shape != ref2.shape:
            self.fails.append((name, layer, -1, -1, "shape %s, expected %s" % (got2.shape, ref2.shape)))
            return
        if cols is not None:
            got2, ref2 = got2[:, :cols], ref2[:, :cols]
        bad = got2 != ref2
        if bad.any():
            r, c = _first(bad)
            self.fails.append((name, layer, r, c, "%s0x%x, expected 0x%x; %d entries differ" % (text, got2[r, c], ref2[r, c], int(bad.sum()))))

    def frag(self, name, layer, key, planes, rows, K):
        got = self.got.get(key)
        if got is None:
            self.fails.append((name, layer, -1, -1, "not delivered"))
            return
        self.checked.append(key)
        npl = len(planes)
        got = np.ascontiguousarray(got).view(np.uint16).reshape(-1)
        if got.size < npl * rows * K:
            self.fails.append((name, layer, -1, -1, "%d elements, expected %d" % (got.size, npl * rows * K)))
            return
        src = unfrag(got[:npl * rows * K].reshape(rows // 16, K // 32, npl, 64, 8), rows, K)
        for p in range(npl):
            bad = src[p] != planes[p]
            if bad.any():
                r, c = _first(bad)
                self.fails.append((name, layer, r, c, "plane %d (source row, column): 0x%x, expected 0x%x; %d entries differ"
                                   % (p, src[p][r, c], planes[p][r, c], int(bad.sum()))))
                return

    def bounded(self, name, layer, key, ref, bound, text):
        """|got - ref| <= bound elementwise (f64 arrays); returns the largest ratio"""
        got = np.asarray(self.got[key], dtype=np.float64).reshape(ref.shape)
        d = np.abs(got - ref)
        if not np.isfinite(got).all():
            r, c = _first(~np.isfinite(got))
            self.fails.append((name, layer, r, c, "not finite"))
            return float("inf")
        bad = d > bound
        ratio = float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))))
        if bad.any():
            r, c = _first(bad)
            self.fails.append((name, layer, r, c, "%s: %.9g, expected %.9g, |difference| %.3g beyond %.3g (worst ratio %.3g)"
                               % (text, got[r, c], ref[r, c], d[r, c], float(np.broadcast_to(bound, d.shape)[r, c]), ratio)))
        return ratio


def compare(sh, params, precision, current, got, where="", raise_on_failure=True):
    """Hold `got` (name -> array as read back; see `read_derived`) to the definitions, for the groups in `current` (KL_DV_* bits)
    at `precision`.  Returns dict(checked=[names], stats={"EK_array", "EK_row", "CtxK"}: the largest ratios of difference to
    bound); raises DerivedMismatch (or with raise_on_failure=False returns the failures under "failures")."""
    W, V, Vp, L = sh.width, sh.voc_size, sh.Vp, sh.depth
    w = weights(sh, params)
    run = _Run(got)
    splitp = precision == PREC_SPLIT
    hi_of, lo_of = {}, {}
    for l in range(L):
        K = w["K%d" % l][:W]
        hi_of["UT", l], lo_of["UT", l] = split(w["U%d" % l].T)
        hi_of["KT", l], lo_of["KT", l] = split(K.T)
    eh, el = split(w["E"])
    eh, el = pad_rows(eh, Vp), pad_rows(el, Vp)
    if current & EAGER:
        for l in range(L):
            run.exact("UT_hi", l, "UT_hi[%d]" % l, hi_of["UT", l])
            run.exact("KT_hi", l, "KT_hi[%d]" % l, hi_of["KT", l])
            run.exact("Un", l, "Un[%d]" % l, bf16_bits(w["U%d" % l]))
            run.exact("Kn", l, "Kn[%d]" % l, bf16_bits(w["K%d" % l][:W]))
        run.exact("E_hi", 0, "E_hi", eh)
        run.exact("ET", 0, "ET", np.ascontiguousarray(eh.T))
        # EK: the thin GEMM's two bounds, on the array and per row
        if run.have("EK"):
            run.checked.append("EK")
            ref, mag = ek_reference(sh, w, precision)
            tol = EK_SPLIT if splitp else EK_BF16
            n0 = len(run.fails)
            run.stats["EK_array"] = run.bounded("EK", 0, "EK", ref, np.full(ref.shape, tol * np.abs(ref).max()), "array bound")
            if len(run.fails) == n0:
                run.stats["EK_row"] = run.bounded("EK", 0, "EK", ref, np.broadcast_to(tol * np.abs(ref).max(axis=1, keepdims=True), ref.shape),
                                                  "row bound")
            zero = (mag == 0) & (np.asarray(got["EK"], dtype=np.float64).reshape(ref.shape) != 0)
            if zero.any():
                r, c = _first(zero)
                run.fails.append(("EK", 0, r, c, "every term is zero, the entry is not"))
        else:
            run.fails.append(("EK", 0, -1, -1, "not delivered"))
        for n in range(sh.n_ctx):
            key = "CtxK[%d]" % n
            if not run.have(key):
                run.fails.append(("CtxK", n, -1, -1, "not delivered"))
                continue
            run.checked.append(key)
            ref, mag = ctxk_reference(sh, w, n)
            r = run.bounded("CtxK", n, key, ref, (sh.ctx_dim + 1) * U24 * mag, "FMA-chain bound")
            run.stats["CtxK"] = max(run.stats.get("CtxK", 0.0), r)
    if current & LO:
        for l in range(L):
            run.exact("UT_lo", l, "UT_lo[%d]" % l, lo_of["UT", l])
            run.exact("KT_lo", l, "KT_lo[%d]" % l, lo_of["KT", l])
        run.exact("E_lo", 0, "E_lo", el)
    if current & INTERLEAVED:
        for l in range(1, L):
            run.exact("KTp", l, "KTp[%d]" % l, interleave_rows(hi_of["KT", l], W))
            run.exact("bp", l, "bp[%d]" % l, f32_bits(interleave_cols(w["b%d" % l], W)).reshape(1, -1), bits=32)
        if run.have("EK"):
            run.exact("EKp", 0, "EKp", f32_bits(ekp_from(np.asarray(got["EK"], dtype=np.float32).reshape(V, 4 * W), w["b0"], W)), bits=32)
        for n in range(sh.n_ctx):
            if run.have("CtxK[%d]" % n):
                run.exact("CtxKp", n, "CtxKp[%d]" % n,
                          f32_bits(interleave_cols(np.asarray(got["CtxK[%d]" % n], dtype=np.float32).reshape(sh.ctx_vocab, 4 * W), W)), bits=32)
    if current & COMB and run.have("EKp") and run.have("CtxKp[0]"):
        run.exact("comb", 0, "comb", comb_from(np.asarray(got["EKp"], dtype=np.float32).reshape(V, 4 * W),
                                               np.asarray(got["CtxKp[0]"], dtype=np.float32).reshape(sh.ctx_vocab, 4 * W)))
    if current & INC:
        for l in range(L):
            run.frag("UF", l, "UF[%d]" % l, [hi_of["UT", l], lo_of["UT", l]][:2 if splitp else 1], 4 * W, W)
            if l > 0:
                run.frag("KF", l, "KF[%d]" % l, [hi_of["KT", l], lo_of["KT", l]][:2 if splitp else 1], 4 * W, W)
        run.frag("EF", 0, "EF", [eh, el][:2 if splitp else 1], Vp, W)
    if current & BIG:
        for l in range(L):
            ref, cols = wtcat_from(sh, w, l, precision)
            run.exact("WTcat", l, "WTcat[%d]" % l, ref, cols=cols)
            run.exact("WTperm", l, "WTperm[%d]" % l, perm32_rows(ref, W), cols=cols)
        ecat = np.concatenate([eh, eh, el], axis=1)
        run.exact("Ecat", 0, "Ecat", ecat, cols=3 * W if splitp else W)
        if run.have("Ecat") and np.ascontiguousarray(got["Ecat"]).view(np.uint16).size == Vp * 3 * W:
            tail = np.ascontiguousarray(got["Ecat"]).view(np.uint16).reshape(Vp, 3 * W)[V:] != 0
            if tail.any():
                r, c = _first(tail)
                run.fails.append(("Ecat", 0, V + r, c, "padding row not zero"))
    out = dict(checked=run.checked, stats=run.stats, failures=run.fails)
    if run.fails and raise_on_failure:
        raise DerivedMismatch(run.fails, where or repr(sh))
    return out


# ---------------------------------------------------------------- reading the device's arrays
def read_derived(view, buf):
    """view: a kl_derived_view (ctypes structure or any object with its fields); buf: the derived buffer as a numpy uint8
    array.  Returns (Shape, got): every CARVED array in the shape its definition has, as uint16 / float32 views of buf."""
    sh = Shape(view.depth, view.width, view.voc_size, view.n_ctx, view.ctx_vocab, view.ctx_dim)
    assert sh.Vp == view.Vp, (sh.Vp, view.Vp)
    assert buf.dtype == np.uint8 and buf.size >= view.bytes, (buf.size, view.bytes)
    W, V, Vp, R = sh.width, sh.voc_size, sh.Vp, sh.ctx_vocab

    def take(off, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert off + n <= view.bytes, ("array beyond the derived buffer", off, n, view.bytes)
        return buf[off:off + n].view(dtype).reshape(shape)
    g = {}
    for l in range(sh.depth):
        Kl = W if l == 0 else 2 * W
        for name in ("UT_hi", "UT_lo", "KT_hi", "KT_lo"):
            g["%s[%d]" % (name, l)] = take(getattr(view, "off_" + name)[l], np.uint16, 4 * W, W)
        for name in ("Un", "Kn"):
            g["%s[%d]" % (name, l)] = take(getattr(view, "off_" + name)[l], np.uint16, W, 4 * W)
        if (view.mask_il >> l) & 1:
            g["KTp[%d]" % l] = take(view.off_KTp[l], np.uint16, 4 * W, W)
            g["bp[%d]" % l] = take(view.off_bp[l], np.float32, 4 * W)
        g["UF[%d]" % l] = take(view.off_UF[l], np.uint16, 2 * 4 * W * W)
        if (view.mask_KF >> l) & 1:
            g["KF[%d]" % l] = take(view.off_KF[l], np.uint16, 2 * 4 * W * W)
        g["WTcat[%d]" % l] = take(view.off_WTcat[l], np.uint16, 4 * W, 3 * Kl)
        g["WTperm[%d]" % l] = take(view.off_WTperm[l], np.uint16, 4 * W, 3 * Kl)
    g["E_hi"], g["E_lo"] = take(view.off_E_hi, np.uint16, Vp, W), take(view.off_E_lo, np.uint16, Vp, W)
    g["ET"] = take(view.off_ET, np.uint16, W, Vp)
    g["EK"], g["EKp"] = take(view.off_EK, np.float32, V, 4 * W), take(view.off_EKp, np.float32, V, 4 * W)
    g["EF"] = take(view.off_EF, np.uint16, 2 * Vp * W)
    g["Ecat"] = take(view.off_Ecat, np.uint16, Vp, 3 * W)
    for n in range(sh.n_ctx):
        g["CtxK[%d]" % n] = take(view.off_CtxK[n], np.float32, R, 4 * W)
        g["CtxKp[%d]" % n] = take(view.off_CtxKp[n], np.float32, R, 4 * W)
    if view.has_comb:
        g["comb"] = take(view.off_comb, np.uint16, V * R, 4 * W)
    return sh, g
