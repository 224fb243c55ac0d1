#!/usr/bin/env python3
"""Training more stateful streams than there are files: `Rater.train` with `segment_streams` on FOUR files.

  python tools/bench_segment_streams.py [--out profiles/segment_streams.json] [--streams 3072] [--parent-json FILE]

The workload of bench.py's `end_to_end_leg` (cfg2: depth 2, width 512, length 256; one epoch + validation through the
drop-in API) with the same number of characters -- `streams` x 201 windows for training, `streams` / 8 x 201 windows for
validation --, but held by four training files and one validation file instead of one file per stream.  The files
are cut into `streams` segments (lib/segments.py); the batches are assembled by kl_assemble_windows.

Reported: chars/s of the whole train() call (`value`) and of its training-step phase (`train_steps_only`), the
phases of `Rater.timings`, and the steps the epoch ran.  Characters are counted as steps x streams x length with the
steps the epoch really ran.  (bench.py's leg credits `windows_per_file - 1` = 200 steps where its epoch runs 201;
`--parent-json`, the JSON line of `bench.py --full` from a checkout of the parent commit run in the same job, is
compared after that correction, and both readings are written down.)

`--assembly-steps N` adds the per-step cost of the batch assembly alone: N steps of a device StreamBatcher at the
benchmark's shape, once through the kernel and once through the torch operations it replaced, host clock around a
device synchronise (for the kernels' own time run this tool under rocprofv3 --kernel-trace --stats with
`--assembly-only --assembly-form kl_assemble_windows`, then `... torch`).  One JSON line on stdout, also written to --out.  Needs the GPU: there is no fallback."""
import argparse
import json
import logging
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOWS_PER_STREAM = 201
N_TRAINING_FILES = 4


def write_file(name, rng, p, voc, size):
    ids = rng.choice(voc - 1, size=size, p=p)
    with open(name, "w", encoding="utf-8") as f:      # (code points U+0100 ..: one character per id, as bench.py writes them)
        f.write((ids.astype('<u4') + 0x100).tobytes().decode('utf-32-le'))


def make_files(tmp, streams, length, voc):
    rng = np.random.default_rng(5)
    p = 1.0 / (np.arange(1, voc) + 1.0)
    p /= p.sum()
    per_stream = WINDOWS_PER_STREAM * length + 1
    total = streams * per_stream
    names = []
    for i in range(N_TRAINING_FILES):
        size = total // N_TRAINING_FILES + (1 if i < total % N_TRAINING_FILES else 0)
        names.append(os.path.join(tmp, "a_b%d_%d.txt" % (i, 1700 + i * 10)))
        write_file(names[-1], rng, p, voc, size)
    val = os.path.join(tmp, "a_val_1800.txt")
    write_file(val, rng, p, voc, max(1, streams // 8) * per_stream)
    return names, val, total


def train_leg(streams):
    import bench
    from math import ceil
    from ocrd_keraslm_amd.lib import Rater
    with tempfile.TemporaryDirectory() as tmp:
        names, val_name, total = make_files(tmp, streams, bench.LENGTH, bench.VOC)
        r = Rater(logger=logging.getLogger("bench.segments"))
        r.width, r.depth, r.length = bench.WIDTH, bench.DEPTH, bench.LENGTH
        r.stateful = True
        r.streams = streams
        r.segment_streams = True
        r.max_epochs = 1
        r.seed = 1
        r.configure()
        files = [open(n, encoding="utf-8") for n in names]
        val = [open(val_name, encoding="utf-8")]
        sizes = [os.path.getsize(n) for n in names]
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            t0 = time.perf_counter()
            r.train(files, val_data=val)
            el = time.perf_counter() - t0
        finally:
            os.chdir(cwd)
            for f in files + val:
                f.close()
        assert r.status == 2, "training failed"
        # the epoch's steps by Rater.train's own formula (rating.py:342 per file, over the streams)
        per_file = [total // N_TRAINING_FILES + (1 if i < total % N_TRAINING_FILES else 0) for i in range(N_TRAINING_FILES)]
        steps = max(1, ceil(sum(ceil((s - bench.LENGTH) / bench.LENGTH) for s in per_file) / streams))
        chars = steps * streams * bench.LENGTH
        t = {k: round(v, 3) for k, v in r.timings.items()}
        return {"value": chars / el, "unit": "chars/s", "seconds": el, "train_steps": steps, "streams": streams,
                "training_files": N_TRAINING_FILES, "validation_files": 1, "training_chars": total, "file_bytes": sizes,
                "phases_s": t, "train_steps_only": chars / t["train_steps"] if t.get("train_steps") else None,
                "loss": r.history["loss"], "val_loss": r.history["val_loss"]}


def assembly_leg(streams, steps, forms=("kl_assemble_windows", "torch")):
    """the batch assembly alone at the benchmark's shape: `steps` batches through kl_assemble_windows, then through torch"""
    import bench
    import io
    import torch
    from ocrd_keraslm_amd.lib import segments, streams as streams_mod
    from ocrd_keraslm_amd.lib.engine import HipLM

    class Mem(io.StringIO):
        name = "a_b_1750.txt"
    T = bench.LENGTH
    rng = np.random.default_rng(1)
    size = streams * (40 * T) + 1
    text = (rng.integers(0, 200, size).astype('<u4') + 0x100).tobytes().decode('utf-32-le')
    c_i = {chr(0x100 + k): k + 1 for k in range(200)}
    f = Mem(text)
    items = [(f, lo, hi) for _, lo, hi in segments.char_plan([size], T, streams)]
    lm = HipLM(1, 64, 201, 1)
    out = {}
    for name, assembler in (("kl_assemble_windows", lm.assemble_windows), ("torch", None)):
        if name not in forms:
            continue
        bat = streams_mod.StreamBatcher(segments.deal(items, 0, streams, streams), T, c_i, train=True,
                                        rng=np.random.default_rng(2), device=lm.device, assembler=assembler)
        bat.prepare()
        for _ in range(3):
            bat.next_batch()
        torch.cuda.synchronize()
        host = 0.0
        t0 = time.perf_counter()
        for _ in range(steps):
            h0 = time.perf_counter()
            plan = bat.next_plan()
            host += time.perf_counter() - h0
            bat.assemble_device(plan)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        out[name] = {"ms_per_step": 1e3 * el / steps, "of_which_host_plan_ms": 1e3 * host / steps, "steps": steps}
    return out


def git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_streams.json"))
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--parent-json", help="JSON line of `bench.py --full` from the parent commit, run in the same job")
    ap.add_argument("--assembly-steps", type=int, default=0)
    ap.add_argument("--assembly-only", action="store_true")
    ap.add_argument("--assembly-form", choices=("both", "kl_assemble_windows", "torch"), default="both",
                    help="the assembly leg in one form only (one form per rocprofv3 run keeps its kernels apart)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_segment_streams: no GPU visible (the rater has no CPU path)")
    result = {"tool": "bench_segment_streams", "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
              "head": git_head()}
    if not args.assembly_only:
        result["segment_streams"] = train_leg(args.streams)
    if args.assembly_steps:
        forms = ("kl_assemble_windows", "torch") if args.assembly_form == "both" else (args.assembly_form,)
        result["assembly"] = assembly_leg(args.streams, args.assembly_steps, forms)
    if args.parent_json and not args.assembly_only:
        lines = [l for l in open(args.parent_json).read().splitlines() if l.startswith("{")]
        e2e = json.loads(lines[-1]).get("end_to_end") or {}
        steps_run = e2e.get("train_steps", 0) + 1      # (its epoch runs one step more than the leg credits)
        as_run = e2e["train_steps_only"] * steps_run / e2e["train_steps"] if e2e.get("train_steps_only") else None
        mine = result["segment_streams"]["train_steps_only"]
        result["parent_many_files"] = {"value": e2e.get("value"), "train_steps_only": e2e.get("train_steps_only"),
                                       "train_steps_only_as_run": as_run, "phases_s": e2e.get("phases_s"),
                                       "streams": e2e.get("streams")}
        result["ratio_train_steps_only"] = mine / e2e["train_steps_only"] if e2e.get("train_steps_only") else None
        result["ratio_train_steps_only_as_run"] = mine / as_run if as_run else None
        result["expectation"] = "ratio_train_steps_only_as_run >= 0.95"
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
