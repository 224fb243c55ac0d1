#!/usr/bin/env python3
"""Lattice decoding: `Rater.rate_best_batch` (many lattices in lockstep, beams kept on the device) against a loop of
`Rater.rate_best(edge_walk=True)` over the same lattices.

  python tools/bench_lattice_batch.py [--out profiles/lattice_batch.json] [--repeats 5] [--sizes 1,16,256]

N random lattices of 30 edges (tests/edge_walk_cases.random_segments, seeds 300 .., no unmapped characters, no empty
alternative: 1-6 alternatives of 1-10 characters), beam width 10, without and with history clustering (distance 5); two models
-- depth 2 at width 512 and at width 128 -- over the character set of the golden fixtures.  Both legs decode the SAME
lattices in the same process, alternated loop, batch, loop, batch, ... `--repeats` times each after one warm-up of both; the
graphs are built outside the clock, the garbage collector runs between the repetitions and is held off inside them; host
clock around the whole leg (both end with their results on the host).  Reported per model, setting and N: the median ms per
edge of both legs with their spreads (max - min) / median, the ratio, whether the batch is faster by more than the loop's
spread, whether both legs chose the same paths, and the split of the batch's time per round (median repetition): building
the host arrays, enqueueing the walk, the decode launch with the round's one wait (the walk's GPU time is inside it), and
the construction of the survivors' `Node`s.  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = {"w512": dict(depth=2, width=512), "w128": dict(depth=2, width=128)}
EDGES = 30


def make_rater(depth, width, chars):
    from ocrd_keraslm_amd.lib import Rater
    r = Rater()
    r.width, r.depth, r.length = width, depth, 256
    r.stateful, r.incremental = False, True
    r.mapping = (dict((c, i) for i, c in enumerate(chars, 1)), dict((i, c) for i, c in enumerate(chars, 1)))
    r.voc_size = len(chars) + 1
    r.seed = 3
    r.configure()
    r.model.init_weights(seed=3, emb_std=0.5)      # (the default 0.001 gives a uniform model: every hypothesis would tie)
    r.model.prepare(3)
    r.status = 2
    r.batch_size = 128
    return r


def timed(fn):
    import torch
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out
    finally:
        gc.enable()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_batch.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--models", default="w512,w128")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lattice_batch: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import lattice_batch
    from tests.edge_walk_cases import CHARS, random_segments
    from tests.test_rater_golden import lattice
    sizes = [int(n) for n in args.sizes.split(",")]
    segments = [random_segments(300 + k, n_edges=EDGES, unmapped=False, empty=False) for k in range(max(sizes))]
    result = {"tool": "bench_lattice_batch", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "edges_per_lattice": EDGES,
              "beam_width": 10, "models": {}}
    for model in args.models.split(","):
        rater = make_rater(chars=CHARS, **MODELS[model])
        rows = {}
        for name, dist in (("plain", 0), ("clustering", 5)):
            for n in sizes:
                def graphs():
                    built = [lattice(segs) for segs in segments[:n]]
                    return [b[0] for b in built], [b[1] for b in built], [b[2] for b in built]

                def loop(gs, ss, es):
                    return [rater.rate_best(g, s, e, context=[17], lm_weight=0.5, beam_width=10, beam_clustering_dist=dist,
                                            edge_walk=True) for g, s, e in zip(gs, ss, es)]

                def batch(gs, ss, es, split=None):
                    return lattice_batch.decode_lattices(rater, gs, ss, es, None, [17], 0.5, 10, dist, None, timings=split)

                def paths(results):
                    return [[(el.id, alt.index) for el, alt, _ in path] for path, _, _ in results]

                same = paths(loop(*graphs())) == paths(batch(*graphs()))      # (also the warm-up of both legs)
                times = {"loop": [], "batch": []}
                splits = []
                for _ in range(args.repeats):
                    g = graphs()
                    times["loop"].append(timed(lambda: loop(*g))[0] / (n * EDGES))
                    g = graphs()
                    split = {}
                    times["batch"].append(timed(lambda: batch(*g, split=split))[0] / (n * EDGES))
                    splits.append(split)
                loop_ms, batch_ms = statistics.median(times["loop"]), statistics.median(times["batch"])
                spread = (max(times["loop"]) - min(times["loop"])) / loop_ms
                mid = splits[sorted(range(len(splits)), key=times["batch"].__getitem__)[len(splits) // 2]]
                rows["%s-n%d" % (name, n)] = {
                    "lattices": n, "clustering_dist": dist, "loop_ms_per_edge": loop_ms, "batch_ms_per_edge": batch_ms,
                    "ratio": loop_ms / batch_ms, "loop_spread": spread,
                    "batch_spread": (max(times["batch"]) - min(times["batch"])) / batch_ms,
                    "faster_beyond_spread": bool(batch_ms < loop_ms * (1.0 - spread)), "same_paths": bool(same),
                    "round_ms": dict((k + "_ms", v * 1e3 / EDGES) for k, v in mid.items())}
                print("%-5s %-10s N=%-4d loop %.4f ms/edge  batch %.4f ms/edge  (%.2fx, loop spread %.1f %%)  same paths: %s  round: %s" % (
                    model, name, n, loop_ms, batch_ms, loop_ms / batch_ms, 100 * spread, same,
                    ", ".join("%s %.3f ms" % (k, v * 1e3 / EDGES) for k, v in mid.items())), file=sys.stderr)
        result["models"][model] = dict(MODELS[model], voc_size=len(CHARS) + 1, settings=rows)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
