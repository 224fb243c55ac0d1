"""bench.py: a plain run reports only the timed steps, and --dump-outputs writes what the last of them computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_BLOCKS = ("roofline", "cpu_baseline", "cpu_baseline_torch", "incremental", "beam_step_latency", "rating_window",
               "small_batch", "cfg5", "reference_models", "other_stream_counts", "end_to_end")


def _cfg2_weights():
    rng = np.random.default_rng(0)
    shapes = {"E": (bench.VOC, bench.WIDTH), "Ctx0": (200, 10)}
    for l in range(bench.DEPTH):
        shapes["K%d" % l] = (bench.WIDTH + 10 if l == 0 else bench.WIDTH, 4 * bench.WIDTH)
        shapes["U%d" % l] = (bench.WIDTH, 4 * bench.WIDTH)
        shapes["b%d" % l] = (4 * bench.WIDTH,)
    return {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}


@pytest.mark.parametrize("B", [3072, 8192])
def test_dump_outputs_dtypes_cap_and_sample(tmp_path, B):
    w = _cfg2_weights()
    states = np.broadcast_to(np.arange(B, dtype=np.float32)[:, None, None], (B, 2 * bench.DEPTH, bench.WIDTH))
    bench.dump_outputs(str(tmp_path), w, states, (4.5, 0.25, 0.125))
    files = {p.name: p for p in tmp_path.iterdir()}
    assert sorted(files) == sorted([k + ".npy" for k in w] + ["loss.npy", "states.npy"])
    assert sum(p.stat().st_size for p in files.values()) <= 64e6
    for k, v in w.items():
        a = np.load(files[k + ".npy"])
        assert a.dtype == np.float32 and np.array_equal(a, v), k
    loss = np.load(files["loss.npy"])
    assert loss.dtype == np.float64 and loss.tolist() == [4.5, 0.25, 0.125]
    s = np.load(files["states.npy"])
    assert s.dtype == np.float32 and s.shape[1:] == states.shape[1:]
    rows = s[:, 0, 0].astype(np.int64)
    assert np.array_equal(s, states[rows])
    if B == 3072:                                   # (the default stream count fits: every stream is written)
        assert np.array_equal(rows, np.arange(B))
    else:                                           # a seeded sample, in stream order, the same every time
        assert 0 < len(rows) < B and np.all(np.diff(rows) > 0)
        bench.dump_outputs(str(tmp_path), w, states, (4.5, 0.25, 0.125))
        assert np.array_equal(np.load(files["states.npy"]), s)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--streams", "64", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "chars/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - 64 * bench.LENGTH / (line["ms_per_step"] / 1e3)) < 1e-6 * line["value"]
    assert all(line[k] is None for k in FULL_BLOCKS)
    states = np.load(out / "states.npy")
    assert states.dtype == np.float32 and states.shape == (64, 2 * bench.DEPTH, bench.WIDTH)
    assert np.isfinite(states).all() and np.abs(states).max() > 0
    k0 = np.load(out / "K0.npy")
    assert k0.dtype == np.float32 and k0.shape == (bench.WIDTH + 10, 4 * bench.WIDTH) and np.isfinite(k0).all()
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == (3,) and np.isfinite(loss).all() and loss[0] > 0
