#!/usr/bin/env python3
"""Suspect words of a corpus: `Rater.suspect_words(precision="bf16")` against what a caller writes without it --
`rate_alternatives(precision="bf16")`, every record off the device, then the words found, rated and picked out in numpy.

  python tools/bench_words.py [--out profiles/rate_words.json] [--repeats 5] [-k 3] [--suspect-share 0.02] [--min-rank 1]

The corpus shapes of bench_suspects.py, cfg2 size (depth 2, width 512, length 256): 1024 documents of 2048 characters and
20 000 lines of 30 to 90 characters, both at 1024 streams.  The shared generator draws a space once in 255 characters, so the
texts are drawn here: a space with probability --space-share (0.16: words of 1 to about 12 characters, 5 on average), any
other character of the alphabet otherwise.  The benchmark's model is untrained; as in bench_corrections.py `max_prob` is set
per corpus to the --suspect-share quantile of the bf16 probabilities (2 %: an OCR-like error rate).  Legs:
  "words"    Rater.suspect_words(precision="bf16"): bulk rating with alternatives, results kept in corpus order on the device,
             the words found, rated and picked out there (kl_word_bounds, kl_rate_segments, kl_segment_select); 52 bytes per
             selected word plus the bits leave the device;
  "parent"   Rater.rate_alternatives(precision="bf16") -- (8k + 8) bytes per character leave the device --, then the three
             numpy statements of lib/ratebulk.py over the whole corpus and the split per text;
  "rating"   the rating part of "parent" alone: rate_alternatives(precision="bf16") with its transfer and its split per text
             (segments_host walks the words in a Python loop, and most of "parent" is that loop: the speed-up is also given
             against "rating", a parent whose numpy part costs nothing);
  "kernels"  the three device calls alone on the device arrays of one bf16 run, with their two reads of a count, the transfer
             of the records and the split per text -- their share of the "words" leg is reported.
Both legs must find the same words: start, length, n, least probability, its place and the suspects exactly, bits and mean
probability to 1e-12 -- asserted per corpus.  Host clock around work that ends in a device synchronise; every leg is warmed up
once, then the legs are alternated in the same process; a leg is repeated inside one timing until it lasts at least
--min-seconds; the median of --repeats (at least 5) timings and the spread (max - min) / median.  One JSON line on stdout,
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

from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater, timed      # noqa: E402


def spaced_documents(rng, sizes, space_share):
    others = np.array([c for c in ALPHABET if c != " "])
    out = []
    for s in sizes:
        chars = others[rng.integers(0, len(others), int(s))]
        chars[rng.random(int(s)) < space_share] = " "
        out.append("".join(chars))
    return out


def corpus_sets(space_share):
    rng = np.random.default_rng(2026)
    docs = spaced_documents(rng, [2048] * 1024, space_share)
    lines = spaced_documents(rng, rng.integers(30, 91, 20000), space_share)
    return [("1024x2048@1024", docs, 1024), ("20000lines@1024", lines, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_words.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--suspect-share", type=float, default=0.02)
    ap.add_argument("--space-share", type=float, default=0.16)
    ap.add_argument("--min-rank", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_words: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
    sync = torch.cuda.synchronize
    repeats = max(5, args.repeats)
    k = args.k
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)      # (as bench_rate_batch --bulk: peaked distributions)
    lm = rater.model
    context = [17]
    delim = rater._delimiter_table(None)
    rule = dict(min_n=1, min_bad=1, min_bpc=0.0)       # (suspect_words' defaults)
    result = {"tool": "bench_words", "device": torch.cuda.get_device_name(0), "repeats": repeats, "k": k,
              "suspect_share": args.suspect_share, "space_share": args.space_share, "min_rank": args.min_rank,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "sets": {}}
    for name, docs, streams in corpus_sets(args.space_share):
        chars = sum(len(d) for d in docs)
        sizes = np.asarray([len(d) for d in docs], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        probs, _ = rater.rate_batch(docs, context, streams=streams, precision="bf16")
        max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
        del probs
        held = {}

        def words():
            return rater.suspect_words(docs, context, k=k, streams=streams, max_prob=max_prob, min_rank=args.min_rank,
                                       precision="bf16")

        def host_part(rated):
            corpus = windows.encode("".join(docs), rater.mapping[0])
            flat_p = np.concatenate([one.probs for one in rated])
            flat_r = np.concatenate([one.rank for one in rated])
            start, end = ratebulk.word_bounds_host(corpus, offsets, delim)
            records = ratebulk.segments_host(flat_p, flat_r, offsets, start, end, max_prob, args.min_rank)
            sel = ratebulk.segment_select_host(start, end, *records, **rule)[1:]
            held["words"] = len(start)
            return [ratebatch.Words.from_records(*([f[a:b] for f in sel] + [int(o)]))
                    for a, b, o in zip(np.searchsorted(sel[0], offsets[:-1]), np.searchsorted(sel[0], offsets[1:]), offsets[:-1])]

        def parent():
            rated, bits = rater.rate_alternatives(docs, context, k=k, streams=streams, precision="bf16")
            return host_part(rated), bits

        def rating():
            return rater.rate_alternatives(docs, context, k=k, streams=streams, precision="bf16")

        def kernels():
            arrays, keep = held["arrays"], held["keep"]
            start, end = lm.word_bounds(keep["corpus"], keep["offsets"], held["delim"])
            records = lm.rate_segments(arrays[0], arrays[1], keep["offsets"], start, end, max_prob, args.min_rank)
            sel = [t.cpu().numpy() for t in lm.segment_select(start, end, records, **rule)[1:]]
            return rater._words_per_text(sel, offsets)

        # both legs find the same words
        found, _ = words()
        other, _ = parent()
        count = sum(len(f) for f in found)
        assert count == sum(len(f) for f in other) and 0 < count < held["words"], (count, held["words"])
        for a, b in zip(found, other):
            for field in ("start", "length", "n", "worst", "suspects"):
                assert np.array_equal(getattr(a, field), getattr(b, field)), field
            assert np.array_equal(a.min_prob.view(np.uint32), b.min_prob.view(np.uint32))
            assert np.allclose(a.bits, b.bits, rtol=1e-12, atol=0) and np.allclose(a.mean_prob, b.mean_prob, rtol=1e-12, atol=0)
        del found, other
        keep = {}
        arrays = rater._rate_in_corpus_order(docs, [context] * len(docs), k, streams, "bf16", keep=keep)[1]
        held.update(arrays=arrays, keep=keep, delim=torch.from_numpy(delim).to(lm.device))
        legs = {"words": words, "parent": parent, "rating": rating, "kernels": kernels}
        inner = {}
        for leg, fn in legs.items():
            fn()
            inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        times = dict((leg, []) for leg in legs)
        for _ in range(repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, inner[leg]))
        n_words = held["words"]
        held.clear()
        row = {"documents": len(docs), "chars": chars, "streams": streams, "max_prob": max_prob, "words": n_words,
               "words_found": count,
               "bytes_from_device": count * 52 + 8 * len(docs),
               "bytes_from_device_parent": chars * (8 * k + 8) + 8 * len(docs),
               "device_bytes_corpus_order": chars * (8 * k + 8)}
        for leg, ts in times.items():
            med = statistics.median(ts)
            row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                        "runs_per_timing": inner[leg]}
        row["speedup"] = row["parent"]["seconds"] / row["words"]["seconds"]
        row["speedup_against_rating_alone"] = row["rating"]["seconds"] / row["words"]["seconds"]
        row["numpy_share_of_parent"] = 1.0 - row["rating"]["seconds"] / row["parent"]["seconds"]
        row["kernels_share"] = row["kernels"]["seconds"] / row["words"]["seconds"]
        result["sets"][name] = row
        print("%-16s words %10.0f  parent %10.0f chars/s (%.2fx; %.2fx against its rating part alone)  %d of %d words  %d / %d bytes  "
              "kernels %.1f %%" % (name, row["words"]["chars_per_s"], row["parent"]["chars_per_s"], row["speedup"],
                                   row["speedup_against_rating_alone"], count, n_words, row["bytes_from_device"],
                                   row["bytes_from_device_parent"], 100.0 * row["kernels_share"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
