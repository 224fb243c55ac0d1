"""The contract of the GEMM launchers (gemm.hip: kl_launch_gemm_tn, kl_launch_gemm_an / _an2; lstm_step.hip:
kl_launch_thin_gemm), as buffers that show when it is broken, a reference, a checker and the case tables.  numpy only:
tests/test_gemm_contract_ref.py turns the checker on a numpy model with planted faults, tests/test_gemm_contract_gpu.py
on the kernels.

What a call may touch:
  * it reads rows [0, rows) x columns [0, K) of a row-major operand with row stride ld (K-major: rows [0, K) x columns
    [0, M)) and nothing it reads beyond that may reach C.  Everything else of an operand's allocation -- the ld - K
    padding columns of every row and 64 whole rows behind the last -- holds the bf16 quiet NaN 0x7fc0 (f32 operands:
    0x7fc00000), so a ragged edge masked on one fragment only shows as 0 * NaN in the valid region of C;
  * it writes rows [0, M) x columns [0, N) of C with row stride ldc (transposed: [0, N) x [0, M)).  C lies inside a
    larger allocation whose other elements hold a marker (f32 0x7fc0beef, bf16 0x7fc1): 64 elements and the alignment
    shift in front, the ldc - N padding columns of every row, 64 rows behind;
  * out_mode 0 / 1 and the thin kernel store, out_mode 2 and every K-major product add to what C holds: the valid
    region starts from C0 = 0 for the storing modes and from a seeded draw, uniform in +- 1/4 max |ref|, for the adding
    ones, and an adding case may be called twice;
  * the bias is added once per call, whatever the K split.

reference(): C0 + calls * (f64 product of the operands as given + bias).  check(): the promises in the order
guard-front, guard-pad, guard-rows (bit for bit), nan (no NaN / Inf in the valid region), value.  The value bound of an
f32 output is the one the direct tests have always used, max |got - ref| <= 1e-5 max |product| (the thin kernel: 3e-5
with the split weights, 1e-5 without); C0 is at most a quarter of that scale, so each of its f32 roundings is below
1e-7 of it, and the tables keep every accumulating case at 16 splits or fewer.  A bf16 output is held element by
element, |got - ref| <= 2^-8 |ref| + 1e-5 max |ref|: the final rounding to bf16 plus the f32 bound (1e-2 of the
maximum would pass an element that is 100 % wrong wherever |ref| is small).  Where the valid region holds a NaN the
value bound is not consulted: "nan" is the finding."""
import functools
from dataclasses import dataclass

import numpy as np

NAN_BF16 = 0x7FC0
NAN_F32 = 0x7FC00000
MARK_F32 = 0x7FC0BEEF
MARK_BF16 = 0x7FC1
GUARD = 64          # elements in front of C, rows behind C and behind every operand
PROMISES = ("guard-front", "guard-pad", "guard-rows", "nan", "value")

TN_ROUTES = {0: "KL_ERR_SHAPE", 1: "long split-K", 2: "persistent", 3: "long, one tile per workgroup", 4: "64x128 long",
             5: "gemm_tn_kernel<64>", 6: "gemm_tn_kernel<128>"}
AN_ROUTES = {0: "not applicable", 1: "256x128", 2: "wide"}
THIN_ROUTES = {0: "bf16 A", 1: "bf16 A, lo", 2: "f32 A", 3: "f32 A, lo"}


def bf16_bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_to_f32(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


@dataclass(frozen=True)
class Case:
    kind: str               # "tn", "an", "thin"
    route: int              # the route the case must take with no KL_GEMM_* switch set (thin: the instantiation)
    M: int
    N: int
    K: int
    lda: int = 0            # 0 = natural (packed)
    ldb: int = 0
    ldc: int = 0
    mode: int = 0           # tn: out_mode; an: 2; thin: 0
    splits: int = 1         # tn: requested K splits; thin: 1 or 3 (hi + lo weights)
    bias: bool = False
    calls: int = 1
    c_off: int = 0          # bytes C is shifted off 16-byte alignment
    # an
    N2: int = 0
    c_t: int = 0
    b_km: int = 0
    # thin
    a_f32: int = 1
    gather: bool = False

    @property
    def accumulates(self):
        return self.kind == "an" or (self.kind == "tn" and self.mode == 2)

    @property
    def out_bf16(self):
        return self.kind == "tn" and self.mode == 1

    @property
    def name(self):
        s = "%s-%dx%dx%d" % (self.kind, self.M, self.N, self.K)
        if self.kind == "an":
            s += "+%d-ct%d-km%d" % (self.N2, self.c_t, self.b_km)
        if self.kind == "thin":
            s += "-%s-split%d%s" % ("f32" if self.a_f32 else "bf16", self.splits, "-gather" if self.gather else "")
        else:
            s += "-mode%d" % self.mode
        if self.kind == "tn" and self.mode == 2:
            s += "-splits%d" % self.splits
        s += "-ld%d.%d.%d" % (self.lda, self.ldb, self.ldc)
        if self.bias:
            s += "-bias"
        if self.calls > 1:
            s += "-calls%d" % self.calls
        if self.c_off:
            s += "-off%d" % self.c_off
        return s

    @property
    def route_name(self):
        return {"tn": TN_ROUTES, "an": AN_ROUTES, "thin": THIN_ROUTES}[self.kind].get(self.route, str(self.route))


# ---------------------------------------------------------------- buffers
def padded_operand(data, ld, fill):
    """data [rows][cols] laid out with row stride ld, the padding columns and GUARD rows behind filled with `fill`"""
    rows, cols = data.shape
    assert ld >= cols
    buf = np.full((rows + GUARD, ld), fill, dtype=data.dtype)
    buf[:rows, :cols] = data
    return buf.reshape(-1)


@dataclass
class Output:
    """C as the kernel stores it: [rows][ld] with cols valid columns, `front` elements in front of it"""
    rows: int
    cols: int
    ld: int
    bf16: bool
    front: int
    c0: np.ndarray          # [rows][cols], f64 (exactly representable in the output type)
    transposed: bool = False

    @property
    def dtype(self):
        return np.uint16 if self.bf16 else np.uint32

    @property
    def marker(self):
        return MARK_BF16 if self.bf16 else MARK_F32

    @property
    def esz(self):
        return 2 if self.bf16 else 4

    def initial(self):
        """the whole allocation, as bits"""
        buf = np.full(self.front + (self.rows + GUARD) * self.ld, self.marker, dtype=self.dtype)
        body = buf[self.front:].reshape(self.rows + GUARD, self.ld)
        if self.bf16:
            body[:self.rows, :self.cols] = bf16_bits(self.c0)
        else:
            body[:self.rows, :self.cols] = self.c0.astype(np.float32).view(np.uint32)
        return buf

    def body(self, buf):
        return buf[self.front:].reshape(self.rows + GUARD, self.ld)

    def values(self, buf):
        """the valid region as f32, in the stored orientation"""
        v = self.body(buf)[:self.rows, :self.cols]
        return bits_to_f32(v) if self.bf16 else np.ascontiguousarray(v).view(np.float32)


def make_output(rows, cols, ld, bf16, c_off, c0, transposed=False):
    esz = 2 if bf16 else 4
    assert c_off % esz == 0 and ld >= cols
    return Output(rows, cols, ld, bf16, GUARD + c_off // esz, c0, transposed)


def draw_c0(seed, ref_single, accumulates):
    if not accumulates:
        return np.zeros_like(ref_single)
    rng = np.random.default_rng(seed)
    amp = 0.25 * np.abs(ref_single).max()
    c0 = rng.uniform(-amp, amp, ref_single.shape).astype(np.float32)
    return c0.astype(np.float64)


# ---------------------------------------------------------------- problems
@dataclass
class Problem:
    case: Case
    a: np.ndarray               # flat operand buffers (bits, or float32 for the thin kernel's f32 A)
    b: list                     # one per product (thin: [hi, lo or None])
    lda: int
    ldb: list
    bias: object                # float32 [N] or None
    row_index: object           # int32 [M] or None
    products: list              # f64 [M][N] per product, without bias
    outputs: list               # Output per product
    tol: float                  # the f32 value bound, relative to max |product|

    def reference(self, i=0):
        """what the valid region of output i must hold after case.calls calls, in the stored orientation"""
        single = self.products[i] + (self.bias.astype(np.float64) if self.bias is not None else 0.0)
        out = self.outputs[i]
        if out.transposed:
            single = single.T
        if self.case.accumulates:
            return out.c0 + self.case.calls * single
        return single


def _natural(v, natural):
    return v if v else natural


@functools.lru_cache(maxsize=3)
def _tn_operands(M, N, K, lda, ldb):
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A = bf16_bits(rng.standard_normal((M, K), dtype=np.float32))
    B = bf16_bits(rng.standard_normal((N, K), dtype=np.float32) * (1 + np.arange(N, dtype=np.float32)[:, None] % 5))
    bias = rng.standard_normal(N).astype(np.float32)
    prod = bits_to_f32(A).astype(np.float64) @ bits_to_f32(B).astype(np.float64).T
    return padded_operand(A, lda, NAN_BF16), padded_operand(B, ldb, NAN_BF16), bias, prod


@functools.lru_cache(maxsize=3)
def _an_operands(M, N, N2, K, lda, ldb, ldb2, b_km):
    rng = np.random.default_rng(M + 3 * N + 5 * N2 + K)
    A = bf16_bits(rng.standard_normal((K, M), dtype=np.float32) * (1 + np.arange(M, dtype=np.float32)[None, :] % 3))
    At = bits_to_f32(A).astype(np.float64).T
    bs, prods = [], []
    for n, ld in ((N, ldb), (N2, ldb2)):
        if n == 0:
            continue
        if b_km:
            Bm = bf16_bits(rng.standard_normal((K, n), dtype=np.float32) * (1 + np.arange(n, dtype=np.float32)[None, :] % 5))
            prods.append(At @ bits_to_f32(Bm).astype(np.float64))
        else:
            Bm = bf16_bits(rng.standard_normal((n, K), dtype=np.float32) * (1 + np.arange(n, dtype=np.float32)[:, None] % 5))
            prods.append(At @ bits_to_f32(Bm).astype(np.float64).T)
        bs.append(padded_operand(Bm, ld, NAN_BF16))
    return padded_operand(A, lda, NAN_BF16), bs, prods


def an_ldb(case, n):
    """row stride of a B operand of n columns: 40 wider than natural K-major (as test_gemm_wide_gpu.py), 8 wider row-major"""
    return n + 40 if case.b_km else case.K + 8


@functools.lru_cache(maxsize=4)
def build(case):
    c = case
    if c.kind == "tn":
        lda, ldb, ldc = _natural(c.lda, c.K), _natural(c.ldb, c.K), _natural(c.ldc, c.N)
        a, b, bias, prod = _tn_operands(c.M, c.N, c.K, lda, ldb)
        bias = bias if c.bias else None
        single = prod + (bias.astype(np.float64) if c.bias else 0.0)
        c0 = draw_c0(c.M + c.N, single, c.accumulates)
        out = make_output(c.M, c.N, ldc, c.out_bf16, c.c_off, c0)
        return Problem(c, a, [b], lda, [ldb], bias, None, [prod], [out], 1e-5)
    if c.kind == "an":
        lda = _natural(c.lda, c.M)
        ldb, ldb2 = an_ldb(c, c.N), (an_ldb(c, c.N2) if c.N2 else 0)
        a, bs, prods = _an_operands(c.M, c.N, c.N2, c.K, lda, ldb, ldb2, c.b_km)
        outs = []
        for i, (n, prod) in enumerate(zip((c.N, c.N2), prods)):
            ct = c.c_t if i == 0 else 1 - c.c_t          # the second product: the other orientation
            single = prod.T if ct else prod
            rows, cols = single.shape
            ld = cols + (8 if i == 0 else 16)            # ... and another ldc
            outs.append(make_output(rows, cols, _natural(c.ldc if i == 0 else 0, ld), False, c.c_off,
                                    draw_c0(c.M + n + i, single, True), transposed=bool(ct)))
        return Problem(c, a, bs, lda, [ldb, ldb2][:len(bs)], None, None, prods, outs, 1e-5)
    assert c.kind == "thin"
    lda, ldw, ldc = _natural(c.lda, c.K + 8), _natural(c.ldb, c.K + 8), _natural(c.ldc, c.N + 8)
    rng = np.random.default_rng(c.M + c.N + c.K)
    A = rng.standard_normal((c.M, c.K)).astype(np.float32)
    Wt = (rng.standard_normal((c.N, c.K)) * (1 + np.arange(c.N)[:, None] % 3)).astype(np.float32)
    bias = rng.standard_normal(c.N).astype(np.float32) if c.bias else None
    row_index = rng.integers(0, c.M, c.M).astype(np.int32) if c.gather else None      # (a draw with repeats)
    hi = bf16_bits(Wt)
    lo = bf16_bits(Wt - bits_to_f32(hi))
    if c.a_f32:
        a = padded_operand(A.view(np.uint32), lda, NAN_F32).view(np.float32)
        # (one weight part: the kernel rounds A to bf16; with the lo part it splits A into hi + lo, 16 bits of mantissa)
        A_eff = A if c.splits == 3 else bits_to_f32(bf16_bits(A))
    else:
        a = padded_operand(bf16_bits(A), lda, NAN_BF16)
        A_eff = bits_to_f32(bf16_bits(A))
    W_eff = bits_to_f32(hi).astype(np.float64) + (bits_to_f32(lo).astype(np.float64) if c.splits == 3 else 0.0)
    A_eff = A_eff.astype(np.float64)
    if c.gather:
        A_eff = A_eff[row_index]
    prod = A_eff @ W_eff.T
    out = make_output(c.M, c.N, ldc, False, c.c_off, np.zeros_like(prod))
    return Problem(c, a, [padded_operand(hi, ldw, NAN_BF16), padded_operand(lo, ldw, NAN_BF16) if c.splits == 3 else None],
                   lda, [ldw], bias, row_index, [prod], [out], 3e-5 if c.splits == 3 else 1e-5)


# ---------------------------------------------------------------- checker
def check_output(out, buf, ref, scale, tol):
    """the broken promises of one output, [(promise, detail)]; ratio: the value bound's use, max err / bound"""
    broken = []
    mark = out.marker
    front = buf[:out.front]
    if (front != mark).any():
        i = int(np.flatnonzero(front != mark)[0])
        broken.append(("guard-front", "element %d in front of C holds 0x%x" % (out.front - i, int(front[i]))))
    body = out.body(buf)
    pad = body[:out.rows, out.cols:]
    if (pad != mark).any():
        r, cc = np.argwhere(pad != mark)[0]
        broken.append(("guard-pad", "row %d, padding column %d holds 0x%x" % (r, out.cols + cc, int(pad[r, cc]))))
    tail = body[out.rows:]
    if (tail != mark).any():
        r, cc = np.argwhere(tail != mark)[0]
        broken.append(("guard-rows", "row %d (past the last, %d), column %d holds 0x%x" % (out.rows + r, out.rows - 1, cc, int(tail[r, cc]))))
    got = out.values(buf).astype(np.float64)
    ratio = float("nan")
    if not np.isfinite(got).all():
        r, cc = np.argwhere(~np.isfinite(got))[0]
        broken.append(("nan", "%d non-finite elements in the valid region, first at [%d][%d]" % (int((~np.isfinite(got)).sum()), r, cc)))
    else:
        err = np.abs(got - ref)
        if out.bf16:
            bound = 2.0 ** -8 * np.abs(ref) + 1e-5 * np.abs(ref).max()
        else:
            bound = np.full_like(ref, tol * scale)
        q = err / bound
        ratio = float(q.max())
        if ratio > 1.0:
            r, cc = np.unravel_index(int(q.argmax()), q.shape)
            broken.append(("value", "[%d][%d]: got %r, ref %r, |diff| %.3e > bound %.3e" % (r, cc, got[r, cc], ref[r, cc], err[r, cc], bound[r, cc])))
    return broken, ratio


def check(problem, bufs, route=None):
    """bufs: the allocation of every output after the calls.  Returns ([(promise, message)], largest value-bound ratio)"""
    c = problem.case
    broken, worst = [], 0.0
    for i, (out, buf) in enumerate(zip(problem.outputs, bufs)):
        ref = problem.reference(i)
        scale = np.abs(problem.products[i]).max()
        b, ratio = check_output(out, buf, ref, scale, problem.tol)
        where = "case %s, route %s%s" % (c.name, c.route_name if route is None else route, ", second product" if i else "")
        broken += [(p, "%s: %s broken: %s" % (where, p, d)) for p, d in b]
        worst = max(worst, ratio) if ratio == ratio else worst
    return broken, worst


def untouched(problem, bufs):
    """every output still as it was handed over (a refused call)"""
    return all((out.initial() == buf).all() for out, buf in zip(problem.outputs, bufs))


# ---------------------------------------------------------------- a numpy model of a kernel, with faults to plant
FAULTS = {
    # fault: (the promise it breaks, what a case needs for it to show)
    "store-not-add": "value", "bias-per-split": "value", "pad-write": "guard-pad", "row-past-m": "guard-rows",
    "front-write": "guard-front", "ktail-one-operand": "nan", "bf16-two-ulps": "value", "ld-as-k": "nan",
}


def _logical(buf, ld, rows, K, kmajor, ktile=0, take_ld=None):
    """the [rows][K'] matrix a kernel sees: element (r, k) at r * ld + k (K-major: k * ld + r), K' = K rounded up to
    ktile (reads past K: whatever lies there)"""
    Kr = K if not ktile else -(-K // ktile) * ktile
    if Kr == K and take_ld is None:
        m = buf.reshape(-1, ld)[:K, :rows].T if kmajor else buf.reshape(-1, ld)[:rows, :K]
        return (m if m.dtype == np.float32 else bits_to_f32(m)).astype(np.float64)
    ld = take_ld or ld
    flat = buf if buf.dtype == np.float32 else bits_to_f32(buf)
    r, k = np.arange(rows)[:, None], np.arange(Kr)[None, :]
    idx = k * ld + r if kmajor else r * ld + k
    return flat[np.minimum(idx, flat.size - 1)].astype(np.float64)


def model_run(problem, splits=1, fault=None):
    """the buffers a correct kernel leaves (fault None), or one with the named fault; `splits`: K ranges added one by one"""
    c = problem.case
    bufs = [out.initial() for out in problem.outputs]
    for _ in range(c.calls):
        for i, out in enumerate(problem.outputs):
            n = (c.N, c.N2)[i]
            akm = c.kind == "an"
            bkm = c.kind == "an" and bool(c.b_km)
            ktile = 64 if fault == "ktail-one-operand" else 0
            if c.kind == "thin":
                A = _logical(problem.a, problem.lda, c.M, c.K, False, ktile, c.K if fault == "ld-as-k" else None)
                if c.a_f32 and c.splits != 3:
                    A = bits_to_f32(bf16_bits(A.astype(np.float32))).astype(np.float64)
                if problem.row_index is not None:
                    A = A[problem.row_index]
                Bm = _logical(problem.b[0], problem.ldb[0], n, c.K, False)
                if problem.b[1] is not None:
                    Bm = Bm + _logical(problem.b[1], problem.ldb[0], n, c.K, False)
            else:
                A = _logical(problem.a, problem.lda, c.M, c.K, akm, ktile, c.K if fault == "ld-as-k" and not akm else None)
                Bm = _logical(problem.b[i], problem.ldb[i], n, c.K, bkm)
            if ktile:       # the tail masked on B only: zeros against whatever A holds past K
                Bm = np.concatenate([Bm, np.zeros((n, A.shape[1] - Bm.shape[1]))], axis=1)
            bias = problem.bias.astype(np.float64) if problem.bias is not None else None
            body = out.body(bufs[i])
            acc = out.values(bufs[i]).astype(np.float64) if c.accumulates else None
            edges = np.linspace(0, A.shape[1], splits + 1).astype(int)
            total = None
            with np.errstate(invalid="ignore"):
                for s in range(splits):
                    part = A[:, edges[s]:edges[s + 1]] @ Bm[:, edges[s]:edges[s + 1]].T
                    if bias is not None and (s == 0 or fault == "bias-per-split"):
                        part = part + bias
                    if out.transposed:
                        part = part.T
                    if fault == "store-not-add":
                        total = part
                    else:
                        total = part if total is None else total + part
            res = total if (acc is None or fault == "store-not-add") else acc + total
            bits = bf16_bits(res) if out.bf16 else res.astype(np.float32).view(np.uint32)
            if fault == "bf16-two-ulps":
                assert out.bf16
                r, cc = np.unravel_index(int(np.abs(res).argmax()), res.shape)
                bits[r, cc] += 2
            body[:out.rows, :out.cols] = bits
            if fault == "pad-write":
                assert out.ld > out.cols
                body[0, out.cols] = bits[0, 0]
            if fault == "row-past-m":
                body[out.rows, :out.cols] = bits[0]
            if fault == "front-write":
                bufs[i][out.front - 1] = bits[0, 0]
    return bufs


# ---------------------------------------------------------------- case tables
def _tn(route, M, N, K, modes, lda=0, ldb=0, ldc=0, splits=1, c_off=0, biases=(False, True)):
    out = []
    for mode in modes:
        for bias in biases:
            for calls in ((1, 2) if mode == 2 else (1,)):
                out.append(Case("tn", route, M, N, K, lda, ldb, ldc, mode, splits if mode == 2 else 1, bias, calls, c_off))
    return out


TN_CASES = (
    # ---- routes 5 / 6: gemm_tn_kernel
    _tn(6, 1, 16, 8, (0, 1, 2))
    + _tn(5, 130, 70, 200, (2,), 208, 216, 75, splits=3) + _tn(5, 130, 70, 200, (1,), 208, 216, 75)
    + _tn(5, 200, 136, 72, (0, 1, 2), lda=80, ldc=140)
    + _tn(6, 64, 2048, 512, (1,), ldc=2056)
    # ---- route 1: the long split-K kernel (accumulating only; every case starts from a non-zero C0)
    + _tn(1, 300, 200, 8192, (2,), 8200, 8256, 203, splits=4)
    + _tn(1, 256, 128, 8256, (2,), splits=1)
    # ---- route 2: persistent workgroups (ragged row tile; ragged column tile and a bias row longer than 512)
    + _tn(2, 66000, 256, 448, (0, 1), ldc=260)
    + _tn(2, 33000, 520, 384, (0, 1), ldc=524)
    # ---- route 3: the same family pushed off the persistent route by each of its conditions in turn
    + _tn(3, 66000, 230, 448, (0, 1, 2), ldc=230)                   # N & 3, ldc & 3: the per-element epilogue
    + _tn(3, 66000, 256, 448, (0,), ldc=260, c_off=4)               # C off 16-byte alignment: per element
    + _tn(3, 66000, 256, 256, (0, 1), ldc=260)                      # K below the persistent range: whole-row epilogues
    + _tn(3, 66000, 256, 448, (1,), ldc=260, c_off=8)               # bf16: 8-byte aligned rows still go whole
    + _tn(3, 66000, 256, 448, (1,), ldc=260, c_off=2)               # ... 2-byte aligned ones per element
    # ---- route 4: 64 x 128 tiles; the incremental step's K = 2 Kl of ld = 3 Kl
    + _tn(4, 1030, 2048, 1024, (0, 1, 2), 1536, 1536)
    + _tn(4, 600, 3072, 576, (0, 1, 2), 1728, 1728, 3080)
    # ---- route 0: refused (K no multiple of 8), C stays as it was
    + _tn(0, 16, 16, 12, (0, 2), lda=16, ldb=16, biases=(False,))
)

# the shapes of tests/test_gpu_kernels.py::test_gemm_tn by the comment that promises their kernel (packed operands, bias)
TN_LEGACY_GROUPS = {
    1: [(512, 256, 16384, 2, 8), (300, 200, 8192, 2, 4), (256, 128, 8256, 2, 1), (100, 520, 12352, 2, 2)],     # "long-K kernel"
    3: [(65536, 128, 256, 0, 1), (33000, 256, 320, 0, 1), (32768, 384, 256, 1, 1)],                            # "... with plain stores"
    2: [(131072, 128, 512, 0, 1), (66000, 256, 448, 0, 1), (140000, 200, 384, 0, 1), (70000, 512, 64 * 9, 0, 1)],   # "persistent workgroups"
    4: [(1024, 2048, 1536, 0, 1), (600, 3072, 576, 0, 1), (1024, 3072, 512, 1, 1)],                            # "64 x 128 tile variant"
}


def _an(route, M, N, N2, K, lda, b_km):
    return [Case("an", route, M, N, K, lda=lda, mode=2, calls=calls, N2=N2, c_t=c_t, b_km=b_km)
            for c_t in (0, 1) for calls in (1, 2)]


AN_CASES = (
    # the cases of test_gemm_wide_gpu.py that reach K splits (the pairs: second product in the other orientation, other ldc)
    _an(2, 512, 512, 0, 4096, 640, 1) + _an(2, 512, 512, 0, 4160, 512, 1)
    + _an(2, 256, 256, 256, 2048, 256, 1) + _an(2, 512, 512, 256, 4096, 640, 1)
    + _an(1, 256, 384, 0, 2048, 256, 1)
    # two narrow ones
    + _an(1, 256, 128, 0, 1024, 256, 0) + _an(1, 512, 200, 0, 4160, 512, 1)
    # K = 160: whole 32-deep stages only -- without the wide form the call is refused and C stays as it was
    + [Case("an", 2, 256, 256, 160, lda=256, mode=2, c_t=1, b_km=1)]
    # refused whatever the switches say: M no multiple of 256; K no multiple of 64 with a row-major B
    + [Case("an", 0, 200, 128, 1024, lda=200, mode=2), Case("an", 0, 256, 128, 96, lda=256, mode=2, c_t=1)]
)

THIN_SHAPES = [(5, 20, 64), (33, 256, 512), (256, 100, 128), (64, 2048, 512)]
THIN_CASES = [Case("thin", 2 * a_f32 + (split == 3), M, N, K, splits=split, bias=bias, a_f32=a_f32, gather=gather)
              for (M, N, K) in THIN_SHAPES for a_f32 in (1, 0) for split in (1, 3) for gather in (False, True)
              for bias in (False, True)]

ALL_CASES = TN_CASES + AN_CASES + THIN_CASES
MAX_SPLITS = 16


def tn_args(c):
    """(M, N, K, lda, ldb, ldc, out_mode, splits) of a tn case with the natural strides filled in"""
    return (c.M, c.N, c.K, _natural(c.lda, c.K), _natural(c.ldb, c.K), _natural(c.ldc, c.N), c.mode, c.splits)


def an_args(c):
    """(M, N, N2, K, lda, ldb, ldb2, b_km) of an an case"""
    return (c.M, c.N, c.N2, c.K, _natural(c.lda, c.M), an_ldb(c, c.N), an_ldb(c, c.N2) if c.N2 else 0, c.b_km)


def c_address_offset(case):
    """bytes from the start of the (first) output's allocation to C"""
    return GUARD * (2 if case.out_bf16 else 4) + case.c_off
