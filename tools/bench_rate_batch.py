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

  python tools/bench_rate_batch.py --bulk [--out profiles/rate_bulk.json] [--repeats 5]

--bulk compares the two precisions of `rate_batch` on corpus-sized inputs, cfg2 size only: 1024 documents of 2048
characters at 256, 1024 and 3072 streams, and 20 000 lines of 30 to 90 characters at 1024 streams.  Legs: "split"
(rate_batch as ever), "bf16" (precision="bf16": bulk rating on the training forward) and both with want_probs=False;
warmed up, alternated, median of --repeats (at least 5) timings; also the largest |p_bf16 - p_split| over all characters.

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


def bulk_sets():
    rng = np.random.default_rng(2025)
    docs = documents(rng, [2048] * 1024)
    lines = documents(rng, rng.integers(30, 91, 20000))
    return [("1024x2048@256", docs, 256), ("1024x2048@1024", docs, 1024), ("1024x2048@3072", docs, 3072),
            ("20000lines@1024", lines, 1024)]


def bulk(args, sync):
    """split against bf16 on the same texts"""
    import torch
    repeats = max(5, args.repeats)
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)      # (embeddings large enough for peaked distributions: |dp| means something)
    context = [17]
    result = {"tool": "bench_rate_batch --bulk", "device": torch.cuda.get_device_name(0), "repeats": repeats,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "sets": {}}
    for name, docs, streams in bulk_sets():
        chars = sum(len(d) for d in docs)
        legs = {}
        for prec in ("split", "bf16"):
            legs[prec] = lambda prec=prec: rater.rate_batch(docs, context, streams=streams, precision=prec)
            legs[prec + "_bits"] = lambda prec=prec: rater.rate_batch(docs, context, streams=streams, want_probs=False,
                                                                      precision=prec)
        p_split, _ = legs["split"]()
        p_bf16, _ = legs["bf16"]()
        gap = max(float(np.abs(a - b).max()) for a, b in zip(p_split, p_bf16) if len(a))
        inner = {}
        for leg, fn in legs.items():
            fn()
            inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        times = dict((leg, []) for leg in legs)
        for _ in range(repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, inner[leg]))
        row = {"documents": len(docs), "chars": chars, "streams": streams, "max_abs_dp": gap}
        for leg, ts in times.items():
            med = statistics.median(ts)
            row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                        "runs_per_timing": inner[leg]}
        row["speedup"] = row["bf16"]["chars_per_s"] / row["split"]["chars_per_s"]
        row["speedup_bits"] = row["bf16_bits"]["chars_per_s"] / row["split_bits"]["chars_per_s"]
        result["sets"][name] = row
        print("%-16s split %10.0f  bf16 %10.0f (%.2fx)  bits only %10.0f / %10.0f (%.2fx) chars/s  max |dp| %.3g" % (
            name, row["split"]["chars_per_s"], row["bf16"]["chars_per_s"], row["speedup"], row["split_bits"]["chars_per_s"],
            row["bf16_bits"]["chars_per_s"], row["speedup_bits"], gap), file=sys.stderr)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/rate_batch.json, with --bulk profiles/rate_bulk.json")
    ap.add_argument("--bulk", action="store_true", help="split against bf16 precision on corpus-sized inputs")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--models", default="cfg2,published")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rate_batch: no GPU visible (the rater has no CPU path)")
    sync = torch.cuda.synchronize
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rate_bulk.json" if args.bulk else "rate_batch.json")
    if args.bulk:
        return emit(bulk(args, sync), args.out)
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
    emit(result, args.out)


def emit(result, out):
    line = json.dumps(result)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
