"""The GEMM contract's checker and case tables (tests/gemm_contract.py), without a GPU.

Sensitivity: a numpy model of a kernel runs the cases; planted with one fault at a time -- a store where the contract
says add, the bias once per K split, an element written into a padding column, a row past M, an element in front of C,
the k-tail masked on one operand only, a bf16 element two ulps off, a row stride taken for K -- the checker has to
answer with exactly the promise that fault breaks, and the unplanted model has to pass every case of every table.

Routes: kl_test_gemm_tn_route / kl_test_gemm_an_route are the launchers' own decision, host only.  Every case has to
land on the route its row names, every route has to be reached by two cases or more, no accumulating case may run
with more than 16 K splits (the value bound counts on that), and the shapes tests/test_gpu_kernels.py::test_gemm_tn
lists under "long-K kernel", "plain stores", "persistent workgroups" and "64 x 128 tile variant" still have to reach
those kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gemm_contract as G  # noqa: E402

C_BASE = 1 << 20          # a 16-byte aligned address for the allocation C lies in


def _lib():
    from ocrd_keraslm_amd.lib import hipabi
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return hipabi.load()


def route_of(lib, case):
    """(route, effective K splits) of a case by the launchers' own rule"""
    out = C.c_int(0)
    if case.kind == "tn":
        M, N, K, lda, ldb, ldc, mode, splits = G.tn_args(case)
        r = lib.kl_test_gemm_tn_route(M, N, K, lda, ldb, ldc, mode, splits, C_BASE + G.c_address_offset(case), int(case.bias), C.byref(out))
        return r, out.value
    if case.kind == "an":
        M, N, N2, K, lda, ldb, ldb2, b_km = G.an_args(case)
        r = lib.kl_test_gemm_an_route(M, N, N2, K, lda, ldb, ldb2, b_km, C.byref(out))
        return r, (-(-K // out.value) if out.value else 0)
    return case.route, 1


def find(kind, **kw):
    for c in G.ALL_CASES:
        if c.kind == kind and all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError((kind, kw))


# ---------------------------------------------------------------- the tables themselves
def test_case_names_are_unique():
    names = [c.name for c in G.ALL_CASES]
    assert len(set(names)) == len(names)


def test_tables_hold_what_they_must():
    tn = G.TN_CASES
    for route in (1, 2, 3, 4):
        modes = {c.mode for c in tn if c.route == route}
        assert modes == ({2} if route == 1 else {0, 1} if route == 2 else {0, 1, 2}), (route, modes)
    assert {c.mode for c in tn if c.route in (5, 6)} == {0, 1, 2}
    for c in tn:       # with and without bias; accumulating cases once and twice
        twin = [d for d in tn if (d.M, d.N, d.K, d.mode, d.c_off, d.ldc) == (c.M, c.N, c.K, c.mode, c.c_off, c.ldc)]
        if c.route:
            assert {d.bias for d in twin} == {False, True}, c.name
        assert {d.calls for d in twin} == ({1, 2} if c.accumulates else {1}), c.name
    assert {c.c_off for c in tn if c.route == 3 and c.mode == 0} == {0, 4}
    assert {c.c_off for c in tn if c.route == 3 and c.mode == 1} == {0, 2, 8}
    for c in G.AN_CASES:
        p = G.build(c)
        for out in p.outputs:
            assert out.ld >= out.cols + 8 and np.abs(out.c0).max() > 0
        if c.N2:
            assert p.outputs[0].transposed != p.outputs[1].transposed and p.outputs[0].ld - p.outputs[0].cols != p.outputs[1].ld - p.outputs[1].cols
    assert len(G.THIN_CASES) == 64 and {c.route for c in G.THIN_CASES} == {0, 1, 2, 3}


def test_buffers_are_poisoned_and_guarded():
    p = G.build(find("tn", M=130, mode=1, bias=True))
    a = p.a.reshape(-1, p.lda)
    assert (a[:130, 200:] == G.NAN_BF16).all() and (a[130:] == G.NAN_BF16).all() and a.shape[0] == 130 + 64
    assert np.isfinite(G.bits_to_f32(a[:130, :200])).all()
    out = p.outputs[0]
    buf = out.initial()
    assert out.front == 64 and (buf[:64] == G.MARK_BF16).all() and np.isnan(G.bits_to_f32(buf[:1]))[0]
    body = out.body(buf)
    assert (body[:130, 70:] == G.MARK_BF16).all() and (body[130:] == G.MARK_BF16).all() and body.shape == (130 + 64, 75)
    # K-major operands: the columns past M and 64 rows behind row K - 1
    p = G.build(find("an", M=512, N=200, calls=1, c_t=0))
    a = p.a.reshape(-1, p.lda)
    assert a.shape == (4160 + 64, 512) and (a[4160:] == G.NAN_BF16).all()
    b = p.b[0].reshape(-1, p.ldb[0])
    assert (b[:4160, 200:] == G.NAN_BF16).all() and (b[4160:] == G.NAN_BF16).all()
    # an f32 output shifted by 4 bytes: one more marker in front
    p = G.build(find("tn", route=3, c_off=4, bias=False))
    assert p.outputs[0].front == 65 and G.c_address_offset(p.case) == 65 * 4
    assert np.isnan(np.array([G.MARK_F32], dtype=np.uint32).view(np.float32))[0]


# ---------------------------------------------------------------- the checker's sensitivity
def small(case):
    return case.M * case.N * case.K <= 1 << 28


@pytest.mark.parametrize("case", G.ALL_CASES, ids=lambda c: c.name)
def test_faultless_model_passes(case):
    p = G.build(case)
    splits = 3 if small(case) else 1
    broken, ratio = G.check(p, G.model_run(p, splits=splits))
    assert broken == [], broken
    assert ratio <= 1.0


PLANTED = [
    ("store-not-add", find("tn", M=200, mode=2, bias=True, calls=1)),
    ("store-not-add", find("tn", M=130, mode=2, bias=False, calls=2)),
    ("store-not-add", find("an", M=256, N=128, calls=1, c_t=1)),
    ("bias-per-split", find("tn", M=130, mode=2, bias=True, calls=1)),
    ("bias-per-split", find("tn", M=1, mode=2, bias=True, calls=2)),
    ("pad-write", find("tn", M=200, mode=0, bias=False)),
    ("pad-write", find("tn", M=130, mode=1, bias=False)),
    ("pad-write", find("thin", M=5, a_f32=0, splits=1, gather=False, bias=False)),
    ("row-past-m", find("tn", M=200, mode=0, bias=True)),
    ("row-past-m", find("an", M=256, N=128, calls=1, c_t=0)),
    ("front-write", find("tn", M=200, mode=1, bias=False)),
    ("front-write", find("tn", M=1, mode=2, bias=False, calls=1)),
    ("ktail-one-operand", find("tn", M=130, mode=1, bias=False)),
    ("ktail-one-operand", find("tn", M=200, mode=0, bias=False)),
    ("bf16-two-ulps", find("tn", M=130, mode=1, bias=True)),
    ("bf16-two-ulps", find("tn", M=200, mode=1, bias=False)),
    ("ld-as-k", find("tn", M=130, mode=2, bias=False, calls=1)),
    ("ld-as-k", find("thin", M=33, a_f32=1, splits=3, gather=False, bias=False)),
]


@pytest.mark.parametrize("fault,case", PLANTED, ids=["%s/%s" % (f, c.name) for f, c in PLANTED])
def test_planted_fault_breaks_exactly_its_promise(fault, case):
    p = G.build(case)
    broken, _ = G.check(p, G.model_run(p, splits=3, fault=fault))
    assert [b[0] for b in broken] == [G.FAULTS[fault]], (fault, broken)
    msg = broken[0][1]
    assert case.name in msg and case.route_name in msg and G.FAULTS[fault] + " broken" in msg, msg


def test_every_fault_and_promise_is_planted():
    assert {f for f, _ in PLANTED} == set(G.FAULTS)
    assert {G.FAULTS[f] for f, _ in PLANTED} == set(G.PROMISES)


def test_bf16_bound_sees_a_small_element_that_is_all_wrong():
    """the bound of the direct test, 1e-2 of the maximum, passes this; the element-wise one does not"""
    case = find("tn", M=200, mode=1, bias=False)
    p = G.build(case)
    bufs = G.model_run(p)
    ref = p.reference()
    big = np.abs(ref).max()
    r, c = np.argwhere((np.abs(ref) > 1e-3 * big) & (np.abs(ref) < 5e-3 * big))[0]
    p.outputs[0].body(bufs[0])[r, c] = 0                     # 100 % wrong
    assert abs(ref[r, c]) <= 1e-2 * big
    broken, _ = G.check(p, bufs)
    assert [b[0] for b in broken] == ["value"] and "[%d][%d]" % (r, c) in broken[0][1]


def test_untouched_tells_a_refused_call_from_a_run():
    p = G.build(find("tn", route=0, mode=2))
    bufs = [out.initial() for out in p.outputs]
    assert G.untouched(p, bufs)
    bufs[0][p.outputs[0].front] ^= 1
    assert not G.untouched(p, bufs)


# ---------------------------------------------------------------- routes, by the launchers' own rule
def test_every_case_lands_on_its_route():
    lib = _lib()
    wrong = [(c.name, c.route, route_of(lib, c)[0]) for c in G.TN_CASES + G.AN_CASES if route_of(lib, c)[0] != c.route]
    assert wrong == [], wrong


def test_every_route_is_reached_twice():
    lib = _lib()
    for cases, n_routes in ((G.TN_CASES, 7), (G.AN_CASES, 3)):
        reached = [route_of(lib, c)[0] for c in cases]
        for route in range(n_routes):
            assert reached.count(route) >= 2, (cases[0].kind, route, reached.count(route))


def test_accumulating_cases_stay_within_16_splits():
    lib = _lib()
    split = {c.name: route_of(lib, c)[1] for c in G.TN_CASES + G.AN_CASES if c.accumulates and c.route}
    assert split and max(split.values()) <= G.MAX_SPLITS, split
    assert max(split.values()) > 1          # ... and some do split
    assert route_of(lib, find("tn", M=300, calls=1, bias=True)) == (1, 8)
    assert route_of(lib, find("tn", M=130, mode=2, calls=1, bias=True)) == (5, 2)       # (K = 200: two 128-deep splits)


def test_legacy_shapes_still_reach_their_kernels():
    """the comment groups of test_gpu_kernels.py::test_gemm_tn (packed operands, a bias, an aligned C)"""
    lib = _lib()
    for route, shapes in G.TN_LEGACY_GROUPS.items():
        for (M, N, K, mode, splits) in shapes:
            got = lib.kl_test_gemm_tn_route(M, N, K, K, K, N, mode, splits, C_BASE, 1, None)
            assert got == route, ((M, N, K, mode, splits), got, route)


def test_route_query_reads_what_the_launch_reads():
    """each condition of the persistent route on its own, the address of C and the bias among them"""
    lib = _lib()

    def q(M=66000, N=256, K=448, ldc=260, mode=0, addr=C_BASE, bias=1):
        return lib.kl_test_gemm_tn_route(M, N, K, K, K, ldc, mode, 1, addr, bias, None)
    assert q() == 2 and q(mode=1) == 2
    assert q(addr=C_BASE + 4) == 3 and q(addr=C_BASE + 8) == 3 and q(ldc=262) == 3 and q(N=230, ldc=232) == 3
    assert q(K=320) == 3 and q(K=1088) == 3 and q(mode=2) == 3 and q(M=60000) == 3
    assert q(N=2560, ldc=2560) == 3 and q(N=2560, ldc=2560, bias=0) == 2
    assert q(K=12) == 0 and q(M=0) == 7
    rows = C.c_int(-1)
    assert lib.kl_test_gemm_an_route(0, 128, 0, 64, 256, 64, 0, 0, C.byref(rows)) == 3
    assert lib.kl_test_gemm_an_route(256, 256, 0, 4096, 256, 296, 0, 1, C.byref(rows)) == 2 and rows.value == 512
    assert lib.kl_test_gemm_an_route(256, 256, 0, 4096, 256, 4096, 0, 0, C.byref(rows)) == 1 and rows.value == 1024
