"""Segment streams on the GPU: `kl_assemble_windows` (csrc/assemble.hip) through the C ABI against the host assembly and
the torch assembly it replaces, `Rater.train` on the HIP engine with more streams than files, and the CLI switch."""
import ctypes as C
import os
import random
import tempfile

import numpy as np
import pytest

from ocrd_keraslm_amd.lib import Rater, streams
from tests.test_rater_plumbing import hip_factory, synth_files
from tests.test_segment_streams import CHARS, MemFile, random_text

pytestmark = pytest.mark.gpu


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def random_plan(rng, bat, B, T, n_ctx):
    """B plan rows as `StreamBatcher.next_plan` makes them, drawn at random, the corner cases in the first rows"""
    total = bat._total                       # ids of text; T + 1 zeros follow
    vlen = rng.integers(1, T + 1, B).astype(np.int64)
    vlen[rng.uniform(size=B) < 0.5] = T
    start = rng.integers(0, total - T, B).astype(np.int64)
    zero_col = np.where(rng.uniform(size=B) < 0.3, rng.integers(0, T, B), -1).astype(np.int64)
    zero_ctx = np.where(rng.uniform(size=B) < 0.3, rng.integers(0, max(n_ctx, 1), B), -1).astype(np.int64)
    if not n_ctx:
        zero_ctx[:] = -1
    ctx = rng.integers(0, 200, (B, n_ctx)).astype(np.int32)
    corners = [
        # (start, vlen, zero_col, zero_ctx)
        (total - T, T, -1, -1),              # the last target is the first padding zero behind the text
        (total, T, 0, n_ctx - 1),            # the window's last target is the LAST id of the corpus array
        (total - 1, 1, 0, -1),               # one character: the tail of a file of T * k + 2 characters
        (0, T, T - 1, n_ctx - 1),
        (3, 1, -1, -1),
    ]
    for b, (s, v, zc, zx) in enumerate(corners[:B]):
        start[b], vlen[b], zero_col[b], zero_ctx[b] = s, v, zc, (zx if n_ctx else -1)
    return start, vlen, zero_col, zero_ctx, ctx, []


@pytest.fixture(scope="module")
def batcher():
    import torch
    rng = np.random.default_rng(3)
    files = [MemFile("a_b%d_%d.txt" % (k, 1750 + k), random_text(rng, size)) for k, size in enumerate((5000, 1, 12345, 4097))]
    c_i = {c: i + 1 for i, c in enumerate(sorted(set(CHARS)))}
    return lambda T: streams.StreamBatcher([[f] for f in files], T, c_i, device=torch.device("cuda:0"))


@pytest.mark.parametrize("n_ctx", [0, 1, 2, 3])
@pytest.mark.parametrize("T", [7, 64, 256, 1000])
@pytest.mark.parametrize("B", [1, 5, 64, 3072])
def test_assemble_windows_equals_host_and_torch_assembly(batcher, B, T, n_ctx):
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    bat = batcher(T)
    bat.prepare()
    bat.n_ctx = n_ctx                        # (the plan carries the contexts: any number of them goes through the same assembly)
    rng = np.random.default_rng(1000 * B + 10 * T + n_ctx)
    plan = random_plan(rng, bat, B, T, n_ctx)
    want = bat.assemble_host(plan)
    witness = [t.cpu().numpy() for t in bat.assemble_device_torch(plan)]
    for w, h in zip(witness, want):
        assert w.dtype == np.int32 and np.array_equal(w, h)
    corpus = bat._corpus_dev
    assert corpus.dtype == torch.int32 and corpus.numel() == bat._total + T + 1
    p = bat._plan_to_device(plan)
    for n_corpus in (corpus.numel(), bat._total):      # (the second: the padding zeros come from the bounds rule instead of memory)
        idx = torch.full((B, T), 77, dtype=torch.int32, device=corpus.device)
        tgt = torch.full((B, T), 77, dtype=torch.int32, device=corpus.device)
        ctx = torch.full((B, T, n_ctx), 77, dtype=torch.int32, device=corpus.device)
        torch.cuda.synchronize()
        code = lib.kl_assemble_windows(ptr(corpus), n_corpus, ptr(p), B, T, n_ctx, ptr(idx), ptr(ctx) if n_ctx else None,
                                       ptr(tgt), None)
        assert code == 0, lib.kl_error_string(code)
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), want[0])
        assert np.array_equal(ctx.cpu().numpy(), want[1])
        assert np.array_equal(tgt.cpu().numpy(), want[2])


def test_assemble_windows_rejects_bad_arguments():
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    lib = hipabi.load()
    corpus = torch.zeros(100, dtype=torch.int32, device="cuda:0")
    plan = torch.zeros((2, 5), dtype=torch.int64, device="cuda:0")
    out = [torch.zeros((2, 8, 1), dtype=torch.int32, device="cuda:0") for _ in range(3)]
    call = lambda c, p, B, T, n, i, z, y: lib.kl_assemble_windows(ptr(c), 100, ptr(p), B, T, n, ptr(i), ptr(z), ptr(y), None)
    assert call(corpus, plan, 2, 8, 1, *out) == 0
    assert call(None, plan, 2, 8, 1, *out) == 5
    assert call(corpus, None, 2, 8, 1, *out) == 5
    assert call(corpus, plan, 0, 8, 1, *out) == 5
    assert call(corpus, plan, 2, 0, 1, *out) == 5
    assert call(corpus, plan, 2, 1025, 1, *out) == 5
    assert call(corpus, plan, 2, 8, 9, *out) == 5
    assert call(corpus, plan, 2, 8, -1, *out) == 5
    assert call(corpus, plan, 2, 8, 1, out[0], None, out[2]) == 5
    torch.cuda.synchronize()


def test_engine_assembler_is_what_the_batcher_uses():
    """a device batcher with the engine's `assemble_windows` gives the batches of a host batcher"""
    import torch
    lm = hip_factory(1, 64, 30, 1)
    rng = np.random.default_rng(9)
    T = 16
    files = [MemFile("a_b%d_%d.txt" % (k, 1750 + 10 * k), random_text(rng, size)) for k, size in enumerate((333, 17, 1000))]
    c_i = {c: i + 1 for i, c in enumerate(sorted(set(CHARS)))}
    per_stream = [[files[0]], [files[1], files[2]], [files[2]]]
    host = streams.StreamBatcher(per_stream, T, c_i, train=True, rng=np.random.default_rng(2), char_degradation=0.3,
                                 context_degradation=0.4)
    devb = streams.StreamBatcher(per_stream, T, c_i, train=True, rng=np.random.default_rng(2), char_degradation=0.3,
                                 context_degradation=0.4, device=lm.device, assembler=lm.assemble_windows)
    for step in range(60):
        (x, z, y), rows = host.next_batch()
        (xd, zd, yd), rows_d = devb.next_batch()
        assert xd.dtype == torch.int32 and xd.is_cuda
        assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(zd.cpu().numpy(), z) and np.array_equal(yd.cpu().numpy(), y)
        assert rows == rows_d


def test_rater_trains_more_streams_than_files_on_the_hip_engine():
    """3 files (2 for training, 1 for validation after the split) at 16 streams; batched path (kernel assembly) against the
    generator path within the tolerances tests/test_rater_plumbing.py uses for the HIP engine (f32 atomics in the
    weight-gradient products)"""
    length, n_streams = 32, 16
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        names = synth_files(tmp, n=3, size=40 * length + 7, seed=4)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            for batched in (True, False):
                random.seed(3)
                r = Rater(engine_factory=hip_factory)
                r.width, r.depth, r.length = 128, 2, length
                r.max_epochs = 2
                r.seed = 5
                r.streams = n_streams
                r.batched_streams = batched
                r.device_dropout_masks = False
                r.segment_streams = True
                r.configure()
                r.train([open(n) for n in names])
                assert r.status == 2
                for key in ("loss", "accuracy", "val_loss", "val_accuracy"):
                    assert len(r.history[key]) == 2 and np.all(np.isfinite(r.history[key])), (key, r.history)
                runs.append((r.history, r.model.get_weights()))
        finally:
            os.chdir(cwd)
    for key in ("loss", "accuracy", "val_loss", "val_accuracy"):
        assert np.allclose(runs[0][0][key], runs[1][0][key], rtol=2e-3, atol=1e-4), (key, runs[0][0], runs[1][0])
    for k, v in runs[0][1].items():
        assert np.abs(v - runs[1][1][k]).max() <= 1e-4 + 1e-2 * np.abs(v).max(), k


def test_cli_train_with_segment_streams():
    from click.testing import CliRunner
    from ocrd_keraslm_amd.scripts.run import cli
    runner = CliRunner()
    with tempfile.TemporaryDirectory() as tmp:
        names = synth_files(tmp, n=4, size=1200)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            model = os.path.join(tmp, "model_segments.h5")
            orig = Rater.__init__

            def short(self, *a, **k):      # one epoch is enough for plumbing
                orig(self, *a, **k)
                self.max_epochs = 1
            Rater.__init__ = short
            try:
                res = runner.invoke(cli, ["train", "-m", model, "-w", "64", "-d", "2", "-l", "32", "--streams", "8",
                                          "--segment-streams"] + names[:3] + ["-v", names[3]])
            finally:
                Rater.__init__ = orig
            assert res.exit_code == 0, res.output + repr(res.exception)
            assert os.path.exists(model)
            res = runner.invoke(cli, ["test", "-m", model, names[3]])
            assert res.exit_code == 0, res.output
            assert 1.0 < float(res.output.strip().splitlines()[-1]) < 100
        finally:
            os.chdir(cwd)
