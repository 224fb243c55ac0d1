#!/usr/bin/env python3
"""Suspect characters of a corpus: `Rater.suspects(precision="bf16")` against `rate_alternatives` in split precision
followed by a filter on the host.

  python tools/bench_suspects.py [--out profiles/rate_suspects.json] [--repeats 5] [-k 3] [--max-prob 0.01] [--min-rank 1]

The corpus-sized inputs of `bench_rate_batch.py --bulk`, cfg2 size (depth 2, width 512, length 256): 1024 documents of 2048
characters and 20 000 lines of 30 to 90 characters, both at 1024 streams.  Legs:
  "suspects"   Rater.suspects(precision="bf16"): bulk rating with alternatives, results kept in corpus order on the device,
               the suspects picked out there (kl_rate_select); count * (8k + 16) bytes plus the bits leave the device;
  "parent"     Rater.rate_alternatives(precision="split") -- (8k + 8) bytes per character leave the device -- and the same
               rule applied per text in numpy;
  "selection"  the selection alone on the device arrays of one bf16 run: counting call, read of the count, writing call,
               transfer of the records and the split per text -- its share of the "suspects" leg is reported.
Host clock around work that ends in a device synchronise; every leg is warmed up once, then the legs are alternated in the
same process; a leg is repeated inside one timing until it lasts at least --min-seconds; the median of --repeats (at least
5) timings and the spread (max - min) / median.  The two legs rate in different precisions, so their suspect counts differ
slightly; both are reported.  One JSON line on stdout, also written to --out.

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

from tools.bench_rate_batch import ALPHABET, MODELS, documents, emit, make_rater, timed      # noqa: E402


def corpus_sets():
    """the documents and lines of bench_rate_batch.bulk_sets, at 1024 streams"""
    rng = np.random.default_rng(2025)
    docs = documents(rng, [2048] * 1024)
    lines = documents(rng, rng.integers(30, 91, 20000))
    return [("1024x2048@1024", docs, 1024), ("20000lines@1024", lines, 1024)]


def host_filter(rated, max_prob, min_rank):
    limit = np.float32(max_prob)
    out = []
    for one in rated:
        keep = np.nonzero((one.rank >= min_rank) & (one.probs <= limit))[0]
        out.append((keep, one.probs[keep], one.rank[keep], one.alt_ids[keep], one.alt_probs[keep]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_suspects.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--max-prob", type=float, default=0.01)
    ap.add_argument("--min-rank", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_suspects: no GPU visible (the rater has no CPU path)")
    sync = torch.cuda.synchronize
    repeats = max(5, args.repeats)
    k = args.k
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)      # (as bench_rate_batch --bulk: peaked distributions)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_suspects", "device": torch.cuda.get_device_name(0), "repeats": repeats, "k": k,
              "max_prob": args.max_prob, "min_rank": args.min_rank, "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1),
              "sets": {}}
    for name, docs, streams in corpus_sets():
        chars = sum(len(d) for d in docs)
        held = {}

        def suspects():
            return rater.suspects(docs, context, k=k, streams=streams, max_prob=args.max_prob, min_rank=args.min_rank,
                                  precision="bf16")

        def parent():
            rated, bits = rater.rate_alternatives(docs, context, k=k, streams=streams, precision="split")
            return host_filter(rated, args.max_prob, args.min_rank), bits

        def selection():
            plan, arrays = held["plan"], held["arrays"]
            sel = [t.cpu().numpy() for t in lm.rate_select(*arrays, max_prob=args.max_prob, min_rank=args.min_rank)]
            lo = np.searchsorted(sel[0], plan.offsets[:-1], side="left")
            hi = np.searchsorted(sel[0], plan.offsets[1:], side="left")
            return [[f[a:b].copy() for f in sel] for a, b in zip(lo, hi)]

        found, _ = suspects()
        count = sum(len(f) for f in found)
        count_parent = sum(len(f[0]) for f in parent()[0])
        plan, arrays, _ = rater._rate_in_corpus_order(docs, [context] * len(docs), k, streams, "bf16")
        held.update(plan=plan, arrays=arrays)
        legs = {"suspects": suspects, "parent": parent, "selection": selection}
        inner = {}
        for leg, fn in legs.items():
            fn()
            inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        times = dict((leg, []) for leg in legs)
        for _ in range(repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, inner[leg]))
        held.clear()
        row = {"documents": len(docs), "chars": chars, "streams": streams, "suspects_found": count,
               "suspects_found_parent": count_parent,
               "bytes_from_device": count * (8 * k + 16) + 8 * len(docs),
               "bytes_from_device_parent": chars * (8 * k + 8) + 8 * len(docs),
               "device_bytes_corpus_order": chars * (8 * k + 8)}
        for leg, ts in times.items():
            med = statistics.median(ts)
            row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                        "runs_per_timing": inner[leg]}
        row["speedup"] = row["suspects"]["chars_per_s"] / row["parent"]["chars_per_s"]
        row["selection_share"] = row["selection"]["seconds"] / row["suspects"]["seconds"]
        result["sets"][name] = row
        print("%-16s suspects %10.0f  parent %10.0f chars/s (%.2fx)  %d / %d found  %d / %d bytes  selection %.1f %%" % (
            name, row["suspects"]["chars_per_s"], row["parent"]["chars_per_s"], row["speedup"], count, count_parent,
            row["bytes_from_device"], row["bytes_from_device_parent"], 100.0 * row["selection_share"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
