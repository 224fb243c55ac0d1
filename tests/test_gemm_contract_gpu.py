"""Every GEMM route held to its contract at the edges of C, A and B (tests/gemm_contract.py: what is read, what is
written, store or add, the bias once), on the kernels.

Each case of the tables goes through kl_test_gemm_tn, kl_test_gemm_an / kl_test_gemm_an2 or kl_test_thin_gemm_ex with
operands whose padding columns and tail rows hold NaN and an output inside guards that hold a marker, and is handed to
the checker: guards bit for bit, no NaN / Inf in the valid region, the value bound against the f64 product (+ bias
once, + C0, twice for two calls).  The route is asked of kl_test_gemm_tn_route / kl_test_gemm_an_route with the
address C really has; with no switch set it has to be the one the case's row names.  A call the route query refuses has
to answer KL_ERR_SHAPE and leave C and its guards as they were.

The whole table runs again under KL_GEMM_LONG=0 (gemm_tn_kernel takes every shape), KL_GEMM_PERS=0, KL_GEMM_WIDE=0 and
KL_GEMM_WIDE_RING=4, each in one fresh child process that runs this file as a script (the switches are read once per
process), one child after the other.

Largest use of the value bound (max over the cases of max err / bound) per route on an MI355X, no switch set:

    route                                   output  cases  largest ratio
    tn 1  long split-K                      f32         8  0.063
    tn 2  persistent                        f32         4  0.039
    tn 2  persistent                        bf16        4  0.991
    tn 3  long, one tile per workgroup      f32        10  0.073
    tn 3  long, one tile per workgroup      bf16        8  0.991
    tn 4  64 x 128 long                     f32        12  0.088
    tn 4  64 x 128 long                     bf16        4  0.990
    tn 5  gemm_tn_kernel<64>                f32        10  0.026
    tn 5  gemm_tn_kernel<64>                bf16        4  0.977
    tn 6  gemm_tn_kernel<128>               f32         6  0.007
    tn 6  gemm_tn_kernel<128>               bf16        4  0.987
    an 1  256 x 128                         f32        12  0.062
    an 2  wide (256 x 256)                  f32        17  0.052
    thin  bf16 A / bf16 A, lo               f32   16 / 16  0.014 / 0.007
    thin  f32 A / f32 A, lo                 f32   16 / 16  0.014 / 0.135

(one run; the split-K sums vary in the last digits with the order of the atomics.  A bf16 output's bound is its own final
rounding, 2^-8 |ref|, plus the f32 bound: a ratio just below 1 is an element that fell half an ulp from its reference, as
a correctly rounded result does somewhere among 10^5 elements or more; the three refused tn cases and the two refused an
cases launch nothing.)
"""
import collections
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gemm_contract as G  # noqa: E402

pytestmark = pytest.mark.gpu

KL_ERR_SHAPE = 1
CASES = G.ALL_CASES
IDS = [c.name for c in CASES]
KNOBS = [("KL_GEMM_LONG", "0"), ("KL_GEMM_PERS", "0"), ("KL_GEMM_WIDE", "0"), ("KL_GEMM_WIDE_RING", "4")]

_on_device = collections.OrderedDict()      # id(host array) -> (host array, device tensor): the big operands go up once


def dev(a, keep=True):
    import torch
    hit = _on_device.get(id(a))
    if hit is not None and hit[0] is a:
        return hit[1]
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    t = torch.from_numpy(a.view(signed) if signed else a).cuda()
    if keep:
        _on_device[id(a)] = (a, t)
        while len(_on_device) > 8:
            _on_device.popitem(last=False)
    return t


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def run_case(case):
    """{route, rc, broken: [[promise, message]], ratio, untouched} of one case on the device"""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    c = case
    p = G.build(c)
    a = dev(p.a)
    bs = [dev(b) if b is not None else None for b in p.b]
    bias = dev(p.bias, keep=False) if p.bias is not None else None
    rix = dev(p.row_index, keep=False) if p.row_index is not None else None
    cd = [dev(out.initial(), keep=False) for out in p.outputs]
    cp = []
    for out, t in zip(p.outputs, cd):
        assert t.data_ptr() % 16 == 0
        cp.append(ptr(t, out.front * out.esz))
    if c.kind == "tn":
        M, N, K, lda, ldb, ldc, mode, splits = G.tn_args(c)
        route = lib.kl_test_gemm_tn_route(M, N, K, lda, ldb, ldc, mode, splits, cp[0].value, int(c.bias), None)
        name = G.TN_ROUTES[route]

        def call():
            return lib.kl_test_gemm_tn(ptr(a), ptr(bs[0]), cp[0], ptr(bias), M, N, K, lda, ldb, ldc, mode, splits, None)
    elif c.kind == "an":
        M, N, N2, K, lda, ldb, ldb2, b_km = G.an_args(c)
        route = lib.kl_test_gemm_an_route(M, N, N2, K, lda, ldb, ldb2, b_km, None)
        name = G.AN_ROUTES[route]
        o = p.outputs

        def call():
            if N2 == 0:
                return lib.kl_test_gemm_an(ptr(a), ptr(bs[0]), cp[0], M, N, K, lda, ldb, o[0].ld, int(o[0].transposed), b_km, None)
            return lib.kl_test_gemm_an2(ptr(a), ptr(bs[0]), cp[0], M, N, K, lda, ldb, o[0].ld, int(o[0].transposed),
                                        ptr(bs[1]), cp[1], N2, ldb2, o[1].ld, int(o[1].transposed), b_km, None)
    else:
        route, name = c.route, c.route_name

        def call():
            return lib.kl_test_thin_gemm_ex(ptr(a), p.lda, c.a_f32, ptr(rix), ptr(bs[0]), ptr(bs[1]), p.ldb[0], c.M, c.N, c.K,
                                            cp[0], p.outputs[0].ld, ptr(bias), c.splits, None)
    rc = 0
    for _ in range(c.calls):
        rc = call()
        if rc != 0:
            break
    torch.cuda.synchronize()
    bufs = [t.cpu().numpy().view(out.dtype) for out, t in zip(p.outputs, cd)]
    res = {"route": route, "rc": rc, "broken": [], "ratio": 0.0, "untouched": G.untouched(p, bufs)}
    if rc == 0:
        broken, ratio = G.check(p, bufs, route=name)
        res["broken"] = [list(b) for b in broken]
        res["ratio"] = ratio
    return res


def verdict(case, res, knob=None):
    print(case.name, res)
    if res["route"] == 0 and case.kind != "thin":
        assert res["rc"] == KL_ERR_SHAPE and res["untouched"], (case.name, res)
        return
    assert res["rc"] == 0, (case.name, res)
    assert res["broken"] == [], "\n".join(b[1] for b in res["broken"])
    assert not res["untouched"]
    if knob is None:
        assert res["route"] == case.route, (case.name, res["route"], case.route)
    elif case.kind == "tn":
        assert res["route"] in {"KL_GEMM_LONG": (5, 6), "KL_GEMM_PERS": (1, 3, 4, 5, 6)}.get(knob, range(1, 7)), (case.name, res)
    elif case.kind == "an" and knob == "KL_GEMM_WIDE":
        assert res["route"] == 1, (case.name, res)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gemm_contract(case):
    verdict(case, run_case(case))


@functools.lru_cache(maxsize=None)
def child_results(knob, value):
    env = dict(os.environ)
    env[knob] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("knob,value", KNOBS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gemm_contract_knobs(case, knob, value):
    """the same cases with one switch moved: other kernels take the shapes, the contract stays"""
    verdict(case, child_results(knob, value)[case.name], knob)


if __name__ == "__main__":
    print(json.dumps({c.name: run_case(c) for c in CASES}))
