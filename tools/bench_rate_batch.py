#!/usr/bin/env python3
"""Rating many independent texts: `Rater.rate_batch` against the loop `reset_states(1); rate(text)`.

  python tools/bench_rate_batch.py [--out profiles/rate_batch.json] [--streams 64] [--repeats 3]

Synthetic documents from a seeded generator; two models -- cfg2 size (depth 2, width 512, length 256) and the
published size (depth 2, width 128, length 256) --; document sets of 1, 16, 64 and 256 documents of 4096 characters
and one of mixed lengths.  Per set three legs: (a) the loop, (b) rate_batch, (c) rate_batch(want_probs=False).
Host clock around work that ends in a device synchronise; every leg is warmed up once (its graphs captured, its
buffers allocated), then the legs are alternated a, b, c, a, b, c, ... in the same process, `--repeats` times each;
a leg is repeated inside one timing until it lasts at least `--min-seconds`.  Reported: the median chars/s of each
leg and the spread (max - min) / median of its repeats.  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALPHABET = [chr(c) for c in range(32, 127)] + [chr(c) for c in range(0xA1, 0xA1 + 160)]      # 255 characters: V = 256
MODELS = {"cfg2": dict(depth=2, width=512, length=256), "published": dict(depth=2, width=128, length=256)}


def make_rater(depth, width, length):
    from ocrd_keraslm_amd.lib import Rater
    r = Rater()
    r.width, r.depth, r.length = width, depth, length
    r.stateful = True
    r.mapping = (dict((c, i) for i, c in enumerate(ALPHABET, 1)), dict((i, c) for i, c in enumerate(ALPHABET, 1)))
    r.voc_size = len(ALPHABET) + 1
    r.seed = 3
    r.configure()
    r.status = 2
    return r


def documents(rng, sizes):
    return ["".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), int(s))) for s in sizes]


def document_sets():
    rng = np.random.default_rng(2024)
    sets = [("%dx4096" % n, documents(rng, [4096] * n)) for n in (1, 16, 64, 256)]
    mixed = np.exp(rng.uniform(np.log(64), np.log(16384), 96)).astype(int)
    sets.append(("mixed96", documents(rng, mixed)))
    return sets


def timed(fn, sync, inner):
    sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    sync()
    return (time.perf_counter() - t0) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_batch.json"))
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--models", default="cfg2,published")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rate_batch: no GPU visible (the rater has no CPU path)")
    sync = torch.cuda.synchronize
    sets = document_sets()
    result = {"tool": "bench_rate_batch", "device": torch.cuda.get_device_name(0), "streams": args.streams,
              "repeats": args.repeats, "models": {}}
    for model in args.models.split(","):
        rater = make_rater(**MODELS[model])
        context = [17]
        rows = {}
        for name, docs in sets:
            chars = sum(len(d) for d in docs)

            def loop():
                for d in docs:
                    rater.model.reset_states(1)
                    rater.rate(d, context)

            legs = {"loop": loop,
                    "rate_batch": lambda: rater.rate_batch(docs, context, streams=args.streams),
                    "rate_batch_bits": lambda: rater.rate_batch(docs, context, streams=args.streams, want_probs=False)}
            inner = {}
            for leg, fn in legs.items():       # warm-up, and how often a leg runs inside one timing
                fn()
                inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
            times = dict((leg, []) for leg in legs)
            for _ in range(args.repeats):
                for leg, fn in legs.items():
                    times[leg].append(timed(fn, sync, inner[leg]))
            row = {"documents": len(docs), "chars": chars}
            for leg, ts in times.items():
                med = statistics.median(ts)
                row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                            "runs_per_timing": inner[leg]}
            row["speedup"] = row["rate_batch"]["chars_per_s"] / row["loop"]["chars_per_s"]
            row["speedup_bits"] = row["rate_batch_bits"]["chars_per_s"] / row["loop"]["chars_per_s"]
            rows[name] = row
            print("%-9s %-8s loop %9.0f  rate_batch %10.0f (%.1fx)  bits only %10.0f (%.1fx) chars/s" % (
                model, name, row["loop"]["chars_per_s"], row["rate_batch"]["chars_per_s"], row["speedup"],
                row["rate_batch_bits"]["chars_per_s"], row["speedup_bits"]), file=sys.stderr)
        result["models"][model] = dict(MODELS[model], voc_size=len(ALPHABET) + 1, sets=rows)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
