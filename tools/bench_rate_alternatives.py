#!/usr/bin/env python3
"""Rating with alternatives: `Rater.rate_alternatives` against the whole-softmax route, beside plain `rate_batch`.

  python tools/bench_rate_alternatives.py [--out profiles/rate_alternatives.json] [--k 3] [--streams 64] [--repeats 3]

64 synthetic documents of 4096 characters from a seeded generator (the 64x4096 set of bench_rate_batch.py), two models
-- cfg2 size (depth 2, width 512, length 256) and the published size (depth 2, width 128, length 256).  Three legs:
(a) `softmax_loop`, the only route without the device selection: per text `reset_states(1)`, then window by window
`forward_window(want_probs=True)` -- 4 V bytes per character to the host -- and `ratebatch.alternatives_of` there;
(b) `rate_alternatives`; (c) `rate_batch`, which delivers the target's probability alone: the floor.
Host clock around work that ends in a device synchronise; every leg is warmed up once, then the legs are alternated
a, b, c, a, b, c, ... in the same process, `--repeats` times each; a leg is repeated inside one timing until it lasts at
least `--min-seconds`.  Reported: the median chars/s of each leg, the spread (max - min) / median of its repeats and the
ratios.  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_rate_batch import ALPHABET, MODELS, documents, make_rater, timed      # noqa: E402


def softmax_loop(rater, docs, context, k):
    """what a caller did for alternatives before rate_alternatives: the whole softmax of every window, sorted on the host"""
    from ocrd_keraslm_amd.lib import ratebatch, windows
    out = []
    for d in docs:
        rater.model.reset_states(1)
        parts = []
        for x, z, y in windows.stateful_windows(windows.normalize(d), context, rater.length, rater.mapping[0]):
            full = rater.model.forward_window(x[None], z[None], want_probs=True).cpu().numpy()
            parts.append(ratebatch.alternatives_of(full, y[None], k))
        out.append(parts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_alternatives.json"))
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--documents", type=int, default=64)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--models", default="cfg2,published")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rate_alternatives: no GPU visible (the rater has no CPU path)")
    sync = torch.cuda.synchronize
    docs = documents(np.random.default_rng(2024), [4096] * args.documents)
    chars = sum(len(d) for d in docs)
    result = {"tool": "bench_rate_alternatives", "device": torch.cuda.get_device_name(0), "k": args.k, "streams": args.streams,
              "repeats": args.repeats, "documents": len(docs), "chars": chars, "models": {}}
    for model in args.models.split(","):
        rater = make_rater(**MODELS[model])
        context = [17]
        legs = {"softmax_loop": lambda: softmax_loop(rater, docs, context, args.k),
                "rate_alternatives": lambda: rater.rate_alternatives(docs, context, k=args.k, streams=args.streams),
                "rate_batch": lambda: rater.rate_batch(docs, context, streams=args.streams)}
        inner = {}
        for leg, fn in legs.items():       # warm-up, and how often a leg runs inside one timing
            fn()
            inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        times = dict((leg, []) for leg in legs)
        for _ in range(args.repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, inner[leg]))
        row = dict(MODELS[model], voc_size=len(ALPHABET) + 1)
        for leg, ts in times.items():
            med = statistics.median(ts)
            row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                        "runs_per_timing": inner[leg]}
        row["speedup_over_softmax_loop"] = row["rate_alternatives"]["chars_per_s"] / row["softmax_loop"]["chars_per_s"]
        row["share_of_rate_batch"] = row["rate_alternatives"]["chars_per_s"] / row["rate_batch"]["chars_per_s"]
        result["models"][model] = row
        print("%-9s softmax loop %9.0f  rate_alternatives %10.0f (%.1fx)  rate_batch %10.0f chars/s" % (
            model, row["softmax_loop"]["chars_per_s"], row["rate_alternatives"]["chars_per_s"],
            row["speedup_over_softmax_loop"], row["rate_batch"]["chars_per_s"]), file=sys.stderr)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
