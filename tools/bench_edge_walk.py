#!/usr/bin/env python3
"""Lattice decoding: `Rater.rate_best` stepwise (one engine call per character) against `edge_walk=True` (one per edge).

  python tools/bench_edge_walk.py [--out profiles/edge_walk_rate_best.json] [--repeats 5]

Synthetic pages from a seeded generator: 100 tokens of 1-8 alternatives of 1-12 characters, each followed by a space edge
(about 200 edges).  Beam width 10, without and with history clustering; two models -- cfg2 size (depth 2, width 512) and the
published size (depth 2, width 128).  Both legs decode the SAME lattices in the same process, alternated stepwise, walk,
stepwise, walk, ... `--repeats` times each after one warm-up; host clock around a whole `rate_best` call (it ends with the
results on the host).  Reported per model and setting: the median ms per edge of both legs, the spread (max - min) / median
of the stepwise repetitions (the garbage collector runs between the repetitions, not inside them), their ratio, whether the walk is faster by more than that spread, whether both legs chose the
same path, mean engine steps per edge of the stepwise leg and mean tracks per edge.  One JSON line on stdout, also written to
--out.  The stepwise leg is the decoder as it was before the walk existed: the comparison inside one run is the acceptance.

Needs the GPU: there is no fallback.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALPHABET = [chr(c) for c in range(33, 127)] + [chr(c) for c in range(0xA1, 0xA1 + 160)]      # 254 characters + the space: V = 256
MODELS = {"cfg2": dict(depth=2, width=512), "published": dict(depth=2, width=128)}


class Alt(object):
    def __init__(self, text, conf, index):
        self.Unicode, self.conf, self.index = text, conf, index


class Elem(object):
    def __init__(self, id_):
        self.id = id_


def make_rater(depth, width):
    from ocrd_keraslm_amd.lib import Rater
    chars = [" "] + ALPHABET
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


def page(seed, tokens=100):
    """[[(text, conf)]] per edge: `tokens` word edges, each followed by a space edge"""
    rng = np.random.default_rng(seed)
    segs = []
    for _ in range(tokens):
        alts = []
        for _ in range(int(rng.integers(1, 9))):
            text = "".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), int(rng.integers(1, 13))))
            alts.append((text, float(rng.uniform(0.3, 1.0))))
        segs.append(alts)
        segs.append([(" ", 1.0)])
    return segs


def lattice(segs):
    import networkx as nx
    g = nx.DiGraph()
    for i, alts in enumerate(segs):
        g.add_edge(i, i + 1, element=Elem("e%d" % i), alternatives=[Alt(t, c, k) for k, (t, c) in enumerate(alts)])
    return g, 0, len(segs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_walk_rate_best.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pages", type=int, default=2)
    ap.add_argument("--models", default="cfg2,published")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_edge_walk: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import lattice_beam
    pages = [page(2025 + k) for k in range(args.pages)]
    edges = sum(len(p) for p in pages)
    result = {"tool": "bench_edge_walk", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "pages": len(pages),
              "edges": edges, "beam_width": 10, "models": {}}
    for model in args.models.split(","):
        rater = make_rater(**MODELS[model])
        rows = {}
        for name, dist in (("plain", 0), ("clustering", 5)):
            def decode(walk):
                traceback, paths = None, []
                for segs in pages:
                    g, s, e = lattice(segs)
                    path, _entropy, traceback = rater.rate_best(g, s, e, start_traceback=traceback, context=[17], lm_weight=0.5,
                                                                beam_width=10, beam_clustering_dist=dist, edge_walk=walk)
                    paths.append([(el.id, alt.index) for el, alt, _ in path])
                return paths

            # what the stepwise leg asks of the engine: steps (batches) and tracks per edge, counted once outside the timing
            stats = {"steps": 0, "tracks": 0}
            real_decode, real_step = lattice_beam.decode_edge, rater.model.step_host

            def counting_decode(tracks, *a, **k):
                stats["tracks"] += len(tracks)
                return real_decode(tracks, *a, **k)

            def counting_step(*a, **k):
                stats["steps"] += 1
                return real_step(*a, **k)

            lattice_beam.decode_edge, rater.model.step_host = counting_decode, counting_step
            try:
                same = decode(False) == decode(True)      # (also the warm-up of both legs)
            finally:
                lattice_beam.decode_edge = real_decode
                del rater.model.step_host
            stats["tracks"] //= 2
            times = {False: [], True: []}
            for _ in range(args.repeats):
                for walk in (False, True):
                    # (the decoder builds thousands of small objects per page: a collection of the oldest generation inside one
                    #  repetition doubled its time -- collected here, outside the clock, and held off inside it)
                    gc.collect()
                    gc.disable()
                    try:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        decode(walk)
                        times[walk].append((time.perf_counter() - t0) * 1e3 / edges)
                    finally:
                        gc.enable()
            step_ms, walk_ms = statistics.median(times[False]), statistics.median(times[True])
            spread = (max(times[False]) - min(times[False])) / step_ms
            rows[name] = {"stepwise_ms_per_edge": step_ms, "edge_walk_ms_per_edge": walk_ms, "ratio": step_ms / walk_ms,
                          "stepwise_spread": spread, "edge_walk_spread": (max(times[True]) - min(times[True])) / walk_ms,
                          "faster_beyond_spread": bool(walk_ms < step_ms * (1.0 - spread)), "same_paths": bool(same),
                          "steps_per_edge": stats["steps"] / edges, "tracks_per_edge": stats["tracks"] / edges}
            print("%-9s %-10s stepwise %.4f ms/edge  edge walk %.4f ms/edge  (%.2fx, stepwise spread %.1f %%)  %.1f steps, %.1f tracks per edge" % (
                model, name, step_ms, walk_ms, step_ms / walk_ms, 100 * spread, rows[name]["steps_per_edge"],
                rows[name]["tracks_per_edge"]), file=sys.stderr)
        result["models"][model] = dict(MODELS[model], voc_size=len(ALPHABET) + 2, settings=rows)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
