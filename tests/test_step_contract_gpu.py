"""One incremental step per case of tests/step_contract.py through the C ABI (kl_step_batch; the host cases through
kl_step_batch_host), in split and in bf16 precision, held to the step contract: nothing but the slots of slot_out and
the n rows of probs changes, everything written is a number, padded hidden units stay zero, the new states and the
probabilities agree with the model reference within 8 E32, and in split precision with the f64 oracle within the
project's standing bounds.  Before the call the test asserts the route kl_test_step_route reports against the case's
table entry, so every kernel family of the step -- inc_tile_kernel on 64- and 128-row tiles, inc_cell_kernel /
inc_cell_hx_kernel with one and two row tiles and both widths classes, the fused and the plain gather + GEMM, the thin
kernel, the three output routes -- runs here in both of its instantiations, at the row counts on either side of every
threshold of the plan.

Layer 0's tables (EK, CtxK) are read back from the device through kl_test_derived_view: tests/test_derived_gpu.py holds
them to their definitions.  Every case prints its figures (got / E32 for states and probabilities, the distance to the
oracle); DESIGN.md records them per route and precision."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import step_contract as S  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = (S.PREC_SPLIT, S.PREC_BF16)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Harness:
    """a handle for one model with one set of switches, bound to its own parameter and derived buffers"""

    def __init__(self, model, env):
        import torch
        from ocrd_keraslm_amd.lib import hipabi
        self.torch, self.hipabi, self.lib = torch, hipabi, hipabi.load()
        self.model, self.env = model, env
        self.dev = torch.device("cuda:0")
        self.cfg = hipabi.KlConfig(model.depth, model.pwidth, model.V, model.n_ctx, S.CTX_VOCAB, S.CTX_DIM)
        self.handle = self.lib.kl_create(C.byref(self.cfg))
        assert self.handle
        self.w = S.logical_weights(model)
        self.flat = S.physical_params(model, self.w)
        assert self.flat.size == self.lib.kl_param_count(C.byref(self.cfg))
        self.params = torch.from_numpy(self.flat).to(self.dev)
        nbytes = self.lib.kl_derived_bytes(self.handle)
        self.derived = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        with S.switches(env):
            hipabi.check(self.lib.kl_bind(self.handle, _ptr(self.params), _ptr(self.derived), nbytes), "kl_bind")
        self.prec, self.op = 0, None
        self.host_ws = []           # (kept alive: the ticket counter at the head of a host workspace must stay this handle's)
        self.true = {}

    def close(self):
        self.torch.cuda.synchronize()
        if self.handle:
            self.lib.kl_destroy(self.handle)
            self.handle = None

    def prepare(self, prec):
        if prec == self.prec:
            return
        torch, hipabi = self.torch, self.hipabi
        hipabi.check(self.lib.kl_prepare(self.handle, prec, None), "kl_prepare")
        torch.cuda.synchronize()
        view = hipabi.KlDerivedView()
        hipabi.check(self.lib.kl_test_derived_view(self.handle, C.byref(view)), "kl_test_derived_view")
        m = self.model
        rows = 4 * m.pwidth

        def table(off, n_rows):
            return self.derived[off:off + n_rows * rows * 4].cpu().numpy().view(np.float32).reshape(n_rows, rows).copy()
        EK = table(view.off_EK, m.V)
        CtxK = [table(view.off_CtxK[k], S.CTX_VOCAB) for k in range(m.n_ctx)]
        self.op = S.operands(m, self.flat, EK, CtxK)
        self.prec = prec

    def route(self, case):
        view = self.hipabi.KlStepRoute()
        rc = self.lib.kl_test_step_route(self.handle, case.n, int(case.ws), int(case.host), C.byref(view))
        return rc, S.route_of(view, self.model.depth), view

    def references(self, buf):
        """the oracle's part is the same in both precisions: computed once per case"""
        refs = S.references(buf, self.w, self.op, self.prec) if buf.case not in self.true else None
        if refs is None:
            n = buf.case.n
            h_in, c_in = buf.states_in()
            es, ep = S.e32(self.op, self.prec, buf.idx[:n], buf.ctx[:n], h_in, c_in, S._sample(n, S.SAMPLE_ROWS))
            refs = S.Refs(self.op, self.prec, *self.true[buf.case], es, ep)
        self.true = {buf.case: (refs.true_probs, refs.true_H, refs.true_C)}
        return refs

    def _device(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(self.dev)

    def step(self, buf):
        torch, case, m = self.torch, buf.case, self.model
        n = case.n
        pool, probs = self._device(buf.pool), self._device(buf.probs)
        idx, si, so = self._device(buf.idx), self._device(buf.slot_in), self._device(buf.slot_out)
        ctx = self._device(buf.ctx) if m.n_ctx else None
        ws, nws = None, 0
        if case.ws:
            nws = int(self.lib.kl_step_workspace_bytes(self.handle, n))
            ws = torch.empty(nws, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()
        self.hipabi.check(self.lib.kl_step_batch(self.handle, n, _ptr(idx), _ptr(ctx), _ptr(pool), _ptr(si), _ptr(so), _ptr(probs),
                                                 _ptr(ws), nws, None), "kl_step_batch")
        torch.cuda.synchronize()
        return pool.cpu().numpy().view(np.uint32), probs.cpu().numpy().view(np.uint32)

    def step_host(self, buf):
        torch, lib, case, m = self.torch, self.lib, buf.case, self.model
        n, k, Wp = case.n, case.head_k, m.pwidth
        pool = self._device(buf.pool)
        nws = int(lib.kl_step_host_workspace_bytes(self.handle, n))
        if not self.host_ws or self.host_ws[-1].numel() < nws:
            self.host_ws.append(torch.zeros(nws, dtype=torch.uint8, device=self.dev))
        ws = self.host_ws[-1]
        sizes = {"probs": buf.probs.size * 4, "heads": max(1, n * k * Wp) * 4, "done": 64}
        ptr = {name: lib.kl_host_alloc(b) for name, b in sizes.items()}
        try:
            assert all(ptr.values())
            arr = {name: np.ctypeslib.as_array(C.cast(ptr[name], C.POINTER(C.c_uint32)), shape=(sizes[name] // 4,)) for name in sizes}
            arr["probs"][:] = S.MARK_F32
            arr["heads"][:] = S.MARK_F32
            idx = np.ascontiguousarray(buf.idx[:n])
            ctx = np.ascontiguousarray(buf.ctx[:n]) if m.n_ctx else None
            si, so = np.ascontiguousarray(buf.slot_in[:n]), np.ascontiguousarray(buf.slot_out[:n])
            tg = np.ascontiguousarray(buf.target) if case.by_target else None
            torch.cuda.synchronize()
            self.hipabi.check(lib.kl_step_batch_host(
                self.handle, n, idx.ctypes.data, ctx.ctypes.data if ctx is not None else None, si.ctypes.data, so.ctypes.data,
                tg.ctypes.data if tg is not None else None, _ptr(pool), k, ptr["probs"], ptr["heads"] if k else None, ptr["done"], 7,
                _ptr(ws), ws.numel(), None), "kl_step_batch_host")
            self.hipabi.check(lib.kl_step_wait(ptr["done"], 7, 20.0), "kl_step_wait")
            torch.cuda.synchronize()
            probs = arr["probs"].copy().reshape(buf.probs.shape)
            heads = arr["heads"][:n * k * Wp].copy().view(np.float32).reshape(n, k * Wp) if k else None
            return pool.cpu().numpy().view(np.uint32), probs, heads
        finally:
            torch.cuda.synchronize()
            for p in ptr.values():
                if p:
                    lib.kl_host_free(p)


@pytest.fixture(scope="module")
def harness():
    """one handle at a time: the cases come grouped by model and switches"""
    held = {}

    def get(model, env):
        key = (model, env)
        if key not in held:
            for h in held.values():
                h.close()
            held.clear()
            held[key] = Harness(model, env)
        return held[key]
    yield get
    for h in held.values():
        h.close()


CASES = sorted(S.ALL_CASES, key=lambda c: (S.ALL_MODELS.index(c.model), c.env, c.host, c.n))


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: "split" if p == S.PREC_SPLIT else "bf16")
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_step_contract(harness, case, prec, capsys):
    hs = harness(case.model, case.env)
    hs.prepare(prec)
    rc, got, view = hs.route(case)
    assert rc == 0
    assert got == S.route_fields(case), (case.route_name, got)
    assert view.lo == int(prec == S.PREC_SPLIT)
    buf = S.build(case)
    refs = hs.references(buf)
    if case.host:
        pool, probs, heads = hs.step_host(buf)
    else:
        (pool, probs), heads = hs.step(buf), None
    m = None
    try:
        m = S.check(buf, refs, pool, probs, heads)
    except S.ContractFailure as e:
        m = e.metrics
        raise
    finally:
        if m:
            with capsys.disabled():
                print("\n  STEP-CONTRACT %s | %s | %s | states %.3g = %.2f E32 (%.3g) | probs %.3g = %.2f E32 (%.3g) | true: states %.3g probs %.3g"
                      % (case.name, "split" if prec == S.PREC_SPLIT else "bf16", case.route_name, m["state"], m["state_ratio"], m["e32_state"],
                         m["prob_rel"], m["prob_ratio"], m["e32_prob"], m.get("true_state", float("nan")), m.get("true_prob", float("nan"))))
