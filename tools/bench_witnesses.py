#!/usr/bin/env python3
"""Two witnesses: the alignment of a second reading on the device (kl_align_pairs, `Rater.align`) against the numpy statement
of the same commit (`ratebulk.align_pairs_host`) -- the parent commit has no alignment at all, and no edit-distance library is
at hand, so a banded DP in numpy is what a caller would write --, and what `Rater.merge_witnesses` spends where.

  python tools/bench_witnesses.py [--out profiles/witnesses.json] [--repeats 5] [--host-repeats 3] [--host-documents 64]
                                  [--host-lines 5000] [--merge-documents 1024] [--merge-lines 20000]

The corpora are bench_words.py's (cfg2 size: depth 2, width 512, length 256; 1024 documents of 2048 characters and 20 000 lines
of 30 to 90 characters).  Every text has ONE witness: the text with 2 % of its characters substituted, 0.5 % dropped and 0.5 %
inserted (--substituted, --dropped, --inserted; seed 2028).  max_dist is 128 for the documents and 32 for the lines.  Legs:
  (a) "align": `Rater.align(texts, witnesses, max_dist)` on the whole set -- normalising, encoding, one upload per side, the
      kernel, the compaction, one download, the `Alignment`s; "kernel": `HipLM.align_pairs` alone on inputs that lie on the
      device, with cell updates per second (cells: the (n + 1) * (2 * max_dist + 1) of a pair, half of them a lane's turn);
      "numpy": `align_pairs_host` on the first --host-documents / --host-lines pairs, "align_subset" the device on the same
      pairs.  All three outputs of the two are asserted identical on that subset.
  (b) "merge": `Rater.merge_witnesses` on the first --merge-documents / --merge-lines texts, alternated with the same chain
      called by hand with a clock between its steps ("by_hand" = "align" + "witness_edits" -- on the host -- +
      "rescore"), one run per timing; spans, edits, candidates and proposals are counted.
Host clock around work that ends in a device synchronise; every leg is warmed up once; the device legs take the median of
--repeats (at least 5) timings, each of at least --min-seconds, the host legs the median of --host-repeats single runs; the
spread is (max - min) / median.  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater, timed      # noqa: E402
from tools.bench_words import corpus_sets      # noqa: E402


def witness_of(rng, text, substituted, dropped, inserted):
    """the text as a second engine might have read it: shares of its characters substituted, dropped, or followed by one more"""
    chars = np.array(list(text))
    lot = rng.random(len(chars))
    hit = lot < substituted
    chars[hit] = np.array(ALPHABET)[rng.integers(0, len(ALPHABET), int(hit.sum()))]
    more = np.where((lot >= substituted + dropped) & (lot < substituted + dropped + inserted),
                    np.array(ALPHABET)[rng.integers(0, len(ALPHABET), len(chars))], "")
    keep = ~((lot >= substituted) & (lot < substituted + dropped))
    return "".join(c + m for c, m, k in zip(chars.tolist(), more.tolist(), keep.tolist()) if k)


def summary(ts):
    med = statistics.median(ts)
    return {"seconds": med, "spread": (max(ts) - min(ts)) / med, "timings": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witnesses.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--host-documents", type=int, default=64)
    ap.add_argument("--host-lines", type=int, default=5000)
    ap.add_argument("--merge-documents", type=int, default=1024)
    ap.add_argument("--merge-lines", type=int, default=20000)
    ap.add_argument("--substituted", type=float, default=0.02)
    ap.add_argument("--dropped", type=float, default=0.005)
    ap.add_argument("--inserted", type=float, default=0.005)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_witnesses: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebatch, ratebulk
    sync = torch.cuda.synchronize
    repeats, host_repeats = max(5, args.repeats), max(1, args.host_repeats)
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_witnesses", "device": torch.cuda.get_device_name(0), "repeats": repeats, "host_repeats": host_repeats,
              "substituted": args.substituted, "dropped": args.dropped, "inserted": args.inserted,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "sets": {}}
    rng = np.random.default_rng(2028)
    codes = lambda strings: (np.frombuffer("".join(strings).encode("utf-32-le"), dtype=np.int32).copy(),
                             np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)

    def host_time(fn):
        ts = []
        for _ in range(host_repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return summary(ts)

    def device_times(legs):
        """the legs warmed up once each, then alternated"""
        inner = {}
        for leg, fn in legs.items():
            fn()
            inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        times = dict((leg, []) for leg in legs)
        for _ in range(repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, inner[leg]))
        return dict((leg, dict(summary(ts), runs_per_timing=inner[leg])) for leg, ts in times.items())

    for number, (name, texts, streams) in enumerate(corpus_sets(0.16)):
        max_dist = 128 if number == 0 else 32
        n_host = args.host_documents if number == 0 else args.host_lines
        n_merge = args.merge_documents if number == 0 else args.merge_lines
        others = [witness_of(rng, t, args.substituted, args.dropped, args.inserted) for t in texts]
        print("%s: %d pairs, max_dist %d" % (name, len(texts), max_dist), file=sys.stderr)

        # ---- (a) the device against the numpy statement
        a, b = codes(texts), codes(others)
        max_len = max(len(t) for t in texts + others)
        on_device = [up(x) for x in a + b]
        sub_a, sub_b = codes(texts[:n_host]), codes(others[:n_host])
        sub_len = max(len(t) for t in texts[:n_host] + others[:n_host])

        def align(n=len(texts), join=0):
            return rater.align(texts[:n], others[:n], max_dist=max_dist, join=join)

        def kernel():
            return lm.align_pairs(*on_device, max_len, max_dist, 0)

        def numpy_leg():
            return ratebulk.align_pairs_host(*sub_a, *sub_b, sub_len, max_dist, 0)

        got, want = align(n_host), numpy_leg()
        for p, one in enumerate(got):
            assert one.dist == want[0][p] and np.array_equal(one.spans, want[2][p, :want[1][p]]), "device and numpy statement disagree"
        raw = [t.cpu().numpy() for t in lm.align_pairs(*[up(x) for x in sub_a + sub_b], sub_len, max_dist, 0)]
        assert all(np.array_equal(g, w) for g, w in zip(raw, want)), "kernel and numpy statement disagree"
        whole = align()
        dist = np.array([one.dist for one in whole])
        cells = int(((np.diff(a[1]) + 1) * (2 * max_dist + 1)).sum())
        row = {"pairs": len(texts), "chars": int(a[1][-1]), "max_dist": max_dist, "max_len": max_len, "host_pairs": n_host,
               "aligned": int((dist >= 0).sum()), "too_far": int((dist == -1).sum()), "mean_dist": float(dist[dist >= 0].mean()),
               "spans": sum(len(one) for one in whole), "cells": cells,
               "workspace_bytes": int(lm.lib.kl_align_pairs_workspace_bytes(len(texts), max_len, max_dist)),
               "numpy": host_time(numpy_leg)}
        row.update(device_times({"align": align, "kernel": kernel, "align_subset": lambda: align(n_host)}))
        row["kernel"]["cells_per_s"] = cells / row["kernel"]["seconds"]
        row["speedup_on_subset"] = row["numpy"]["seconds"] / row["align_subset"]["seconds"]
        print("%-16s align %.4f s (kernel %.4f s, %.3g cells/s); %d pairs: device %.4f s, numpy %.2f s (%.0fx)"
              % (name, row["align"]["seconds"], row["kernel"]["seconds"], row["kernel"]["cells_per_s"], n_host,
                 row["align_subset"]["seconds"], row["numpy"]["seconds"], row["speedup_on_subset"]), file=sys.stderr)

        # ---- (b) merge_witnesses and its parts
        part, readings = texts[:n_merge], [[w] for w in others[:n_merge]]
        pairs = [(i, 0) for i in range(len(part))]
        rescoring = dict(streams=streams, precision="bf16")

        def merge():
            return rater.merge_witnesses(part, readings, context, max_dist=max_dist, **rescoring)

        def parts():
            """the chain by hand with a clock between its steps: (align, edits, rescore) in seconds"""
            sync()
            stamps = [time.perf_counter()]
            flat = align(n_merge, join=1)
            sync()
            stamps.append(time.perf_counter())
            edits, _ = ratebatch.witness_edits(flat, pairs, part, readings)
            stamps.append(time.perf_counter())
            rater.rescore(part, edits, context, **rescoring)
            sync()
            stamps.append(time.perf_counter())
            return np.diff(stamps)

        flat = align(n_merge, join=1)
        edits, skipped = ratebatch.witness_edits(flat, pairs, part, readings)
        alignments, rescored, merged_skipped = merge()
        assert merged_skipped == skipped and sum(len(one) for one in rescored) == len(edits)
        parts()
        whole, split = [], []
        for _ in range(repeats):      # (a call lasts longer than --min-seconds asks for: one run per timing, the two alternated)
            whole.append(timed(merge, sync, 1))
            split.append(parts())
        split = np.array(split)
        merge_row = {"texts": len(part), "chars": sum(len(t) for t in part), "streams": streams, "join": 1,
                     "spans": sum(len(one) for one in flat), "edits": len(edits), "candidates": sum(len(e[3]) for e in edits),
                     "skipped": skipped, "proposals": sum(int((one.best >= 0).sum()) for one in rescored),
                     "merge": summary(whole), "by_hand": summary(split.sum(axis=1).tolist())}
        for column, step in enumerate(("align", "witness_edits", "rescore")):
            merge_row[step] = summary(split[:, column].tolist())
        row["merge"] = merge_row
        result["sets"][name] = row
        print("%-16s merge %.3f s; by hand %.3f s = align %.4f + edits %.4f + rescore %.3f; %d spans, %d edits, %d proposals"
              % (name, merge_row["merge"]["seconds"], merge_row["by_hand"]["seconds"], merge_row["align"]["seconds"],
                 merge_row["witness_edits"]["seconds"], merge_row["rescore"]["seconds"], merge_row["spans"], merge_row["edits"],
                 merge_row["proposals"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
