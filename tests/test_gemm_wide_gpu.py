"""The weight-gradient contraction's wide form: 256 x 256 tiles on sixteen waves, 32-deep stages in a ring of 4 or 5
(gemm.hip, kl_launch_gemm_an2 with both operands K-major and every width a multiple of 256).

Every case goes through kl_test_gemm_an / kl_test_gemm_an2 with b_km = 1 and is held to the f64 product of the same
bf16 operands with the bound of test_gpu_kernels.py::test_gemm_an, max |got - ref| <= 1e-5 * max |ref| (K <= 16384).
The shapes are the smallest at which the loop can go wrong: one tile with fewer k-steps than the ring, as many, and one
more (for either ring depth: K = 64, 128, 160, 192); several tiles and K splits with padded rows, both output
orientations, splits with odd k-step counts (K = 4160: 17 and 11), the paired launch, and a width the rule refuses.
Every case runs again with KL_GEMM_WIDE=0 (the 256 x 128 kernel) and with KL_GEMM_WIDE_RING=4 (the four-stage ring),
each set in one fresh child process that runs this file as a script.  K = 160 is no multiple of the 256 x 128 kernel's
64-deep stage: with KL_GEMM_WIDE=0 the call has to answer KL_ERR_SHAPE there (its caller's sign to transpose), as it
does for every such K without the wide form."""
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

pytestmark = pytest.mark.gpu

# (M, N, N2, K, lda, c_transposed): N2 > 0 = the paired launch (second product: its own operand, other orientation)
CASES = [
    (256, 256, 0, 64, 256, 0), (256, 256, 0, 128, 256, 0), (256, 256, 0, 160, 256, 1), (256, 256, 0, 192, 256, 0),
    (512, 512, 0, 4096, 640, 0), (512, 512, 0, 4096, 640, 1), (512, 512, 0, 4160, 512, 1),
    (256, 256, 256, 2048, 256, 0), (512, 512, 256, 4096, 640, 1),
    (256, 384, 0, 2048, 256, 0),
]
IDS = ["%dx%d+%dx%d-lda%d-ct%d" % c for c in CASES]
BOUND = 1e-5
KL_ERR_SHAPE = 1


def bf16_bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=None)
def operands(case):
    """A_km [K][lda], B_km [K][N + 40] (and B2_km [K][N2 + 40]) as bf16 bits, and the f64 products"""
    M, N, N2, K, lda, _ = case
    rng = np.random.default_rng(M + 3 * N + 5 * N2 + K)
    A = bf16_bits(rng.standard_normal((K, lda)).astype(np.float32) * (1 + np.arange(lda)[None, :] % 3))
    At = bits_to_f32(A)[:, :M].astype(np.float64).T
    Bs, refs = [], []
    for n in (N, N2):
        if n == 0:
            continue
        B = bf16_bits(rng.standard_normal((K, n + 40)).astype(np.float32) * (1 + np.arange(n + 40)[None, :] % 5))
        Bs.append(B)
        refs.append(At @ bits_to_f32(B)[:, :n].astype(np.float64))
    return A, Bs, refs


def run_case(case):
    """[(max |got - ref|, max |ref|)] per product; for a pair also each product launched singly and its distance from the
    paired result; None: the call answered KL_ERR_SHAPE"""
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    M, N, N2, K, lda, c_t = case
    A, Bs, refs = operands(case)

    def dev(a):
        return torch.from_numpy(a.view(np.int16)).cuda()

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def out(n, ct):
        return torch.zeros((n, M) if ct else (M, n), dtype=torch.float32, device="cuda")

    def host(t, ct):
        a = t.cpu().numpy().astype(np.float64)
        return a.T if ct else a

    Ad, Bd = dev(A), [dev(b) for b in Bs]
    res = []
    if N2 == 0:
        Cd = out(N, c_t)
        rc = lib.kl_test_gemm_an(ptr(Ad), ptr(Bd[0]), ptr(Cd), M, N, K, lda, N + 40, M if c_t else N, c_t, 1, None)
        if rc == KL_ERR_SHAPE:
            return None
        hipabi.check(rc)
        torch.cuda.synchronize()
        res.append((float(np.abs(host(Cd, c_t) - refs[0]).max()), float(np.abs(refs[0]).max())))
        return res
    ct2 = 1 - c_t
    C1, C2 = out(N, c_t), out(N2, ct2)
    hipabi.check(lib.kl_test_gemm_an2(ptr(Ad), ptr(Bd[0]), ptr(C1), M, N, K, lda, N + 40, M if c_t else N, c_t,
                                      ptr(Bd[1]), ptr(C2), N2, N2 + 40, M if ct2 else N2, ct2, 1, None))
    torch.cuda.synchronize()
    for Cp, Bq, n, ct, ref in ((C1, Bd[0], N, c_t, refs[0]), (C2, Bd[1], N2, ct2, refs[1])):
        got = host(Cp, ct)
        Cs = out(n, ct)
        hipabi.check(lib.kl_test_gemm_an(ptr(Ad), ptr(Bq), ptr(Cs), M, n, K, lda, n + 40, M if ct else n, ct, 1, None))
        torch.cuda.synchronize()
        single = host(Cs, ct)
        scale = float(np.abs(ref).max())
        res.append((float(np.abs(got - ref).max()), scale))
        res.append((float(np.abs(single - ref).max()), scale))
        res.append((float(np.abs(got - single).max()), scale))
    return res


def check(case, res):
    print(case, res)
    assert res is not None and len(res) == (6 if case[2] else 1)
    for err, scale in res:
        assert err <= BOUND * scale, (case, err, scale)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gemm_wide(case):
    check(case, run_case(case))


@functools.lru_cache(maxsize=None)
def child_results(knob, value):
    env = dict(os.environ)
    env[knob] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("knob,value", [("KL_GEMM_WIDE", "0"), ("KL_GEMM_WIDE_RING", "4")])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gemm_wide_knobs(case, knob, value):
    """the same cases through the 256 x 128 kernel (KL_GEMM_WIDE=0) and through the four-stage ring"""
    res = child_results(knob, value)[IDS[CASES.index(case)]]
    if knob == "KL_GEMM_WIDE" and case[3] % 64:
        assert res is None, (case, res)
        return
    check(case, res and [tuple(x) for x in res])


if __name__ == "__main__":
    print(json.dumps({i: run_case(c) for i, c in zip(IDS, CASES)}))
