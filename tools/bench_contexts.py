#!/usr/bin/env python3
"""Rating under candidate contexts over a corpus: `Rater.rate_contexts(precision="bf16")` against the loop a caller writes on
the parent commit's interface -- one `Rater.rate_batch(precision="bf16")` per candidate, then `ratebulk.context_mix_host` over
the probabilities it returned.

  python tools/bench_contexts.py [--out profiles/rate_contexts.json] [--repeats 5] [--candidates 20] [--streams 1024]

cfg2 size (depth 2, width 512, length 256), 20 candidates (the decades 1700 .. 1890 of a one-variable model), three corpora:
64 documents of 2048 characters -- the small job whose 64 rows become 1280 --, 1024 documents of 2048 characters and 20 000
lines of 30 to 90 characters (bench_rate_batch's bulk sets).  Legs:
  "contexts"   Rater.rate_contexts(want_probs=True): one upload of the ids, one bulk plan over texts x candidates, the planes
               and the mix on the device (kl_rate_scatter_planes, kl_context_mix);
  "loop"       per candidate rate_batch(texts, candidate, precision="bf16") at the same `streams`, the C lists of probabilities
               laid out as planes on the host, context_mix_host.
Both legs must name the same `best` for every text (the run fails otherwise, after writing what it measured); the largest
difference of their bits is reported -- the two legs run other batch compositions through the bf16 forward, so it need not
be zero.  Also reported: the share
of the "contexts" call spent in kl_context_mix and in kl_rate_scatter_planes (device time between events around the engine
calls, in one extra run) and the bytes that leave the device on either leg.
Host clock around work that ends in a device synchronise; every leg is warmed up once, then the legs are alternated in the
same process; the median of --repeats (at least 5) timings and the spread (max - min) / median.  One JSON line on stdout,
also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_rate_batch import ALPHABET, MODELS, documents, emit, make_rater, timed      # noqa: E402


def corpus_sets():
    rng = np.random.default_rng(2025)
    docs = documents(rng, [2048] * 1024)
    lines = documents(rng, rng.integers(30, 91, 20000))
    return [("64x2048", docs[:64]), ("1024x2048", docs), ("20000lines", lines)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_contexts.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--streams", type=int, default=1024)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_contexts: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk
    sync = torch.cuda.synchronize
    repeats = max(5, args.repeats)
    streams = args.streams
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)      # (as bench_rate_batch --bulk: peaked distributions)
    lm = rater.model
    candidates = [[171 + c] for c in range(args.candidates)]
    C = len(candidates)
    result = {"tool": "bench_contexts", "device": torch.cuda.get_device_name(0), "repeats": repeats, "candidates": C,
              "streams": streams, "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "sets": {}}
    for name, docs in corpus_sets():
        chars = sum(len(d) for d in docs)

        def contexts():
            return rater.rate_contexts(docs, candidates, streams=streams, precision="bf16")

        def loop():
            per = [rater.rate_batch(docs, c, streams=streams, precision="bf16")[0] for c in candidates]
            offsets = np.concatenate([[0], np.cumsum([len(p) for p in per[0]])]).astype(np.int64)
            planes = np.stack([np.concatenate(p) for p in per])
            mix = np.ones(planes.shape[1], dtype=np.float32)
            return ratebulk.context_mix_host(planes, offsets, None, mix), mix

        # one run of each outside the timings: the two legs agree
        found = contexts()
        (cand_bits, mix_bits, post, best, margin), _ = loop()
        differ = np.nonzero(np.asarray([f.best for f in found]) != best)[0]
        bits = np.stack([f.bits for f in found])
        # one more run with events around the two new engine calls
        spans = {"context_mix": [], "rate_scatter_planes": []}

        def watched(call, into):
            def run(*a, **k):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out = call(*a, **k)
                t1.record()
                into.append((t0, t1))
                return out
            return run
        lm.context_mix, lm.rate_scatter_planes = watched(lm.context_mix, spans["context_mix"]), watched(lm.rate_scatter_planes,
                                                                                                  spans["rate_scatter_planes"])
        try:
            watched_seconds = timed(contexts, sync, 1)
        finally:
            del lm.context_mix, lm.rate_scatter_planes      # (the instance attributes: the methods are back)
        device_seconds = dict((k, sum(a.elapsed_time(b) for a, b in v) * 1e-3) for k, v in spans.items())
        legs = {"contexts": contexts, "loop": loop}
        times = dict((leg, []) for leg in legs)
        for _ in range(repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, 1))
        plan_calls = len(ratebulk.plan_candidates([len(d) for d in docs], candidates, rater.length, streams)[0].calls)
        loop_calls = C * len(ratebulk.plan([len(d) for d in docs], [candidates[0]] * len(docs), rater.length, streams).calls)
        row = {"documents": len(docs), "chars": chars, "rows": len(docs) * C, "window_calls": plan_calls, "window_calls_loop": loop_calls,
               "best_identical": not len(differ), "best_differs": int(len(differ)),
               "largest_margin_where_best_differs": float(margin[differ].max()) if len(differ) else 0.0,
               "max_abs_bits_difference": float(np.abs(bits - cand_bits).max()),
               "max_rel_bits_difference": float((np.abs(bits - cand_bits) / np.maximum(1.0, cand_bits)).max()),
               "least_margin_bits": float(margin.min()),
               "bytes_from_device": {"contexts": chars * 4 + len(docs) * (16 * C + 20), "contexts_without_probs": len(docs) * (16 * C + 20),
                                     "loop": C * (chars * 4 + len(docs) * 8)},
               "watched_run_seconds": watched_seconds}
        for leg, ts in times.items():
            med = statistics.median(ts)
            row[leg] = {"chars_times_candidates_per_s": chars * C / med, "seconds": med, "spread": (max(ts) - min(ts)) / med}
        row["speedup"] = row["loop"]["seconds"] / row["contexts"]["seconds"]
        for k, v in device_seconds.items():
            row[k + "_device_seconds"] = v
            row[k + "_share"] = v / watched_seconds
        result["sets"][name] = row
        print("%-12s contexts %.3f s  loop %.3f s (%.2fx)  mix %.2f %%  scatter %.2f %%  calls %d vs %d  |dbits| %.3g"
              % (name, row["contexts"]["seconds"], row["loop"]["seconds"], row["speedup"], 100.0 * row["context_mix_share"],
                 100.0 * row["rate_scatter_planes_share"], plan_calls, loop_calls, row["max_abs_bits_difference"]), file=sys.stderr)
    emit(result, args.out)
    if not all(row["best_identical"] for row in result["sets"].values()):
        sys.exit("bench_contexts: the two legs disagree about `best` (see best_differs)")


if __name__ == "__main__":
    main()
