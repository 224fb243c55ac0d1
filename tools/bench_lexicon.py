#!/usr/bin/env python3
"""Lexicon look-up of suspect words: the device path (kl_lexicon_neighbours, `Rater.correct_words`) against the numpy statement
of the same commit (`ratebulk.lexicon_neighbours_host`) -- the parent commit has no look-up at all, and no edit-distance
library is at hand, so vectorised numpy is what a caller would write.

  python tools/bench_lexicon.py [--out profiles/lexicon.json] [--repeats 5] [--host-repeats 3] [--queries 2000]
                                [--large-queries 20000] [--documents 32] [--lines 1000] [--max-dist 2] [--per-word 8]

The corpora are bench_words.py's (cfg2 size: depth 2, width 512, length 256; 1024 documents of 2048 characters and 20 000 lines
of 30 to 90 characters, a space with probability 0.16, 254 other characters).  The LEXICON is the distinct words of the clean
corpus in order of first occurrence -- 228 576 and 140 757 entries of 7 characters on average, the size of a real word
list --; the texts that are corrected are the corpus with OCR-like noise (--noise, 2 % of the characters replaced), so that
most suspect words are one or two edits away from an entry.  Legs:
  (a) "kernel" / "numpy": the --queries first distinct words of the noisy documents against the documents' lexicon, through
      `HipLM.lexicon_neighbours` (upload of the queries, the call, download of the results; the lexicon is on the device) and
      through `ratebulk.lexicon_neighbours_host`; all four outputs are asserted identical.  --queries is chosen so that the numpy
      leg lasts well under a minute (measured: 2.5 ms per query at this lexicon size, 5 s).  "kernel_large" is the same call at
      --large-queries distinct words, the size of a real suspect list, with pair distances per second (pairs: the entries of
      the length classes a query is compared with); "kernel_large_64bit" is that call with KL_LEXICON_NARROW=0, which keeps the
      queries of at most 32 ids on the 64-bit pattern word too -- alternated with it, same outputs asserted;
  (b) "correct" / "composed": `Rater.correct_words` against `suspect_words` + the numpy look-up of the distinct suspect words +
      `word_edits` + `rescore`, on the first --documents documents and the first --lines lines (cut down so that the numpy
      look-up of their suspect words lasts well under a minute; the lexicon stays the whole corpus's).  Same edits and same
      choices are asserted.  max_prob is the 2 % quantile of the bf16 probabilities, as in bench_words.py.
Host clock around work that ends in a device synchronise; every leg is warmed up once; the device legs take the median of
--repeats (at least 5) timings, each of at least --min-seconds, the numpy legs the median of --host-repeats single runs; the
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


def noisy(rng, docs, share):
    """the texts with `share` of their characters replaced by a random non-space character"""
    others = np.array([c for c in ALPHABET if c != " "])
    out = []
    for d in docs:
        chars = np.array(list(d))
        hit = rng.random(len(chars)) < share
        chars[hit] = others[rng.integers(0, len(others), int(hit.sum()))]
        out.append("".join(chars))
    return out


def distinct_words(docs):
    seen = {}
    for d in docs:
        for w in d.split(" "):
            if w and w not in seen:
                seen[w] = None
    return list(seen)


def summary(ts):
    med = statistics.median(ts)
    return {"seconds": med, "spread": (max(ts) - min(ts)) / med, "timings": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexicon.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--large-queries", type=int, default=20000)
    ap.add_argument("--documents", type=int, default=32)
    ap.add_argument("--lines", type=int, default=1000)
    ap.add_argument("--max-dist", type=int, default=2)
    ap.add_argument("--per-word", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--suspect-share", type=float, default=0.02)
    ap.add_argument("-k", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lexicon: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
    sync = torch.cuda.synchronize
    repeats, host_repeats = max(5, args.repeats), max(1, args.host_repeats)
    D, K = args.max_dist, args.per_word
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_lexicon", "device": torch.cuda.get_device_name(0), "repeats": repeats, "host_repeats": host_repeats,
              "max_dist": D, "per_word": K, "noise": args.noise, "suspect_share": args.suspect_share, "k": args.k,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "kernel": {}, "sets": {}}
    rng = np.random.default_rng(2027)
    encode = lambda words: (windows.encode("".join(words), rater.mapping[0]).astype(np.int32),
                            np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64))
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

    for number, (name, docs, streams) in enumerate(corpus_sets(0.16)):
        lexicon = rater.lexicon(distinct_words(docs))
        texts = noisy(rng, docs, args.noise)
        chars_d, order_d = lexicon.on_device(lm)
        print("%s: lexicon of %d entries, %d ids" % (name, len(lexicon), len(lexicon.pool)), file=sys.stderr)

        def pairs_of(q_off):
            m = np.diff(q_off)
            m = m[(m >= 1) & (m <= 64)]
            first = lexicon.class_first      # (first[L]: the entries shorter than L)
            return int((first[np.minimum(m + D, 64) + 1] - first[np.maximum(m - D, 1)]).sum())

        if number == 0:
            # ---- (a) the kernel against the numpy statement, same words, same lexicon
            words = distinct_words(texts)
            small, large = encode(words[:args.queries]), encode(words[:args.large_queries])

            def kernel(q=small):
                res = lm.lexicon_neighbours(chars_d, order_d, lexicon.class_first, rater.voc_size, up(q[0]), up(q[1]), D, K)
                return [t.cpu().numpy() for t in res]

            def kernel_wide():      # the 64-bit pattern word for every query
                os.environ["KL_LEXICON_NARROW"] = "0"
                try:
                    return kernel(large)
                finally:
                    del os.environ["KL_LEXICON_NARROW"]

            def numpy_leg():
                return ratebulk.lexicon_neighbours_host(small[0], small[1], lexicon.chars, lexicon.order, lexicon.class_first,
                                                        rater.voc_size, D, K)

            got, want = kernel(), numpy_leg()
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), "kernel and numpy statement disagree"
            again, wide = kernel(large), kernel_wide()
            assert all(np.array_equal(g[:len(w)], w) for g, w in zip(again, want))
            assert all(np.array_equal(g, w) for g, w in zip(again, wide))
            row = {"lexicon_entries": len(lexicon), "lexicon_ids": int(len(lexicon.pool)), "queries": len(small[1]) - 1,
                   "pairs": pairs_of(small[1]), "with_exact": int((want[0] >= 0).sum()), "with_neighbours": int((want[1] > 0).sum()),
                   "numpy": host_time(numpy_leg), "large_queries": len(large[1]) - 1, "large_pairs": pairs_of(large[1]),
                   "queries_of_at_most_32": int((np.diff(large[1]) <= 32).sum())}
            row.update(device_times({"kernel": kernel, "kernel_large": lambda: kernel(large), "kernel_large_64bit": kernel_wide}))
            row["speedup"] = row["numpy"]["seconds"] / row["kernel"]["seconds"]
            for leg in ("kernel_large", "kernel_large_64bit"):
                row[leg]["pairs_per_s"] = row["large_pairs"] / row[leg]["seconds"]
            result["kernel"] = row
            print("kernel %.4f s  numpy %.2f s (%.0fx) at %d queries; %d queries: %.4f s, %.3g pairs/s (64-bit word only: %.4f s)"
                  % (row["kernel"]["seconds"], row["numpy"]["seconds"], row["speedup"], row["queries"], row["large_queries"],
                     row["kernel_large"]["seconds"], row["kernel_large"]["pairs_per_s"], row["kernel_large_64bit"]["seconds"]),
                  file=sys.stderr)

        # ---- (b) correct_words against the composed call with the numpy look-up
        part = texts[:args.documents if number == 0 else args.lines]
        probs, _ = rater.rate_batch(part, context, streams=streams, precision="bf16")
        max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
        del probs
        rule = dict(k=args.k, streams=streams, max_prob=max_prob, min_rank=1, precision="bf16")
        held = {}

        def correct():
            return rater.correct_words(part, lexicon, context, max_dist=D, per_word=K, **rule)

        def composed():
            found, bits = rater.suspect_words(part, context, **rule)
            words = sorted(set(w for one, t in zip(found, part) for w in one.strings(t)))
            q = encode(words)
            exact, _, cand, _ = ratebulk.lexicon_neighbours_host(q[0], q[1], lexicon.chars, lexicon.order, lexicon.class_first,
                                                                 rater.voc_size, D, K)
            table = dict((w, [lexicon.words[i] for i in cand[n] if i >= 0] if exact[n] < 0 else []) for n, w in enumerate(words))
            edits = ratebatch.word_edits(found, part, table)
            held.update(words=len(words), edits=len(edits), candidates=sum(len(e[3]) for e in edits))
            return found, rater.rescore(part, edits, context, streams=streams, precision="bf16"), bits

        def suspects_only():
            return rater.suspect_words(part, context, **rule)

        mine, other = correct(), composed()
        for a, b in zip(mine[1], other[1]):
            assert a.candidates == b.candidates and np.array_equal(a.starts, b.starts) and np.array_equal(a.best, b.best)
            assert np.array_equal(a.gain, b.gain)
        row = {"documents": len(part), "chars": sum(len(t) for t in part), "streams": streams, "max_prob": max_prob,
               "lexicon_entries": len(lexicon), "suspect_words": sum(len(f) for f in mine[0]), "distinct_suspect_words": held["words"],
               "edits": held["edits"], "candidates": held["candidates"],
               "proposals": sum(int((one.best >= 0).sum()) for one in mine[1]),
               "composed": host_time(composed)}
        row.update(device_times({"correct": correct, "suspect_words_alone": suspects_only}))
        row["speedup"] = row["composed"]["seconds"] / row["correct"]["seconds"]
        result["sets"]["%dof%s" % (len(part), name)] = row
        print("%-16s correct %.3f s  composed %.2f s (%.1fx)  %d suspect words, %d edits, %d proposals"
              % (name, row["correct"]["seconds"], row["composed"]["seconds"], row["speedup"], row["suspect_words"], row["edits"],
                 row["proposals"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
