#!/usr/bin/env python3
"""Lexicon look-up across word boundaries: kl_lexicon_splits against the parent's look-up of the same words
(kl_lexicon_neighbours) and against its numpy statement (`ratebulk.lexicon_splits_host`), the share of planted boundary errors
that `Rater.correct_words` offers the true form for with and without `boundaries`, and what the flag costs.

  python tools/bench_lexicon_boundaries.py [--out profiles/lexicon_boundaries.json] [--repeats 5] [--host-repeats 3]
                                           [--queries 2000] [--large-queries 20000] [--host-queries 100] [--documents 32]
                                           [--recall-documents 4] [--max-dist 2] [--min-part 2] [--per-word 8] [--share 0.03]

The corpus and the lexicon are bench_lexicon.py's first set (1024 documents of 2048 characters, a space with probability 0.16,
254 other characters; the lexicon is the distinct words of the clean corpus in order of first occurrence).  The texts that are
looked at are the corpus with boundary errors planted and no other noise: --share of the spaces between two words are taken
away (the truth is `left right`), and --share of the words of at least 2 * min_part characters get a space at a random place
that leaves min_part characters on either side (the truth is the word).  Legs:
  (a) "splits" / "neighbours": the --queries (and --large-queries) first distinct words of the planted documents through
      `HipLM.lexicon_splits` and through `HipLM.lexicon_neighbours` at the same max_dist -- upload of the queries, the call,
      download of the results; the lexicon is on the device --, alternated.  "numpy" is `ratebulk.lexicon_splits_host` on the
      first --host-queries of them (chosen so that it lasts well under a minute), all five outputs asserted identical to the
      kernel's.
  (b) "recall": the first --recall-documents documents with EVERY word selected (max_prob 1, min_rank 0, min_suspects 0), so
      that the figure is the look-ups' and not the model's, which is untrained here: the share of the planted errors of either
      kind for which `correct_words` hands `rescore` an edit over exactly the planted span with the true form among its
      candidates, with and without `boundaries`.
  (c) "correct" / "correct_boundaries": `Rater.correct_words` without and with the flag on the first --documents documents,
      the suspect words chosen as in bench_lexicon.py (max_prob the 2 % quantile of the bf16 probabilities), alternated.
Host clock around work that ends in a device synchronise; every leg is warmed up once; the device legs take the median of
--repeats (at least 5) timings, each of at least --min-seconds, the numpy leg the median of --host-repeats single runs; the
spread is (max - min) / median.  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_lexicon import distinct_words, summary      # noqa: E402
from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater, timed      # noqa: E402
from tools.bench_words import corpus_sets      # noqa: E402


def planted(rng, docs, share, min_part):
    """the texts with boundary errors, and per text the planted errors as (kind, start, end, truth) in the new text"""
    texts, errors = [], []
    for d in docs:
        words = d.split(" ")
        out, marks, at, i = [], [], 0, 0
        while i < len(words):
            w = words[i]
            nxt = words[i + 1] if i + 1 < len(words) else ""
            if w and nxt and len(w) + len(nxt) < 64 and rng.random() < share:
                piece, mark = w + nxt, ("merged", at, at + len(w) + len(nxt), w + " " + nxt)
                i += 1
            elif len(w) >= 2 * min_part and rng.random() < share:
                s = int(rng.integers(min_part, len(w) - min_part + 1))
                piece, mark = w[:s] + " " + w[s:], ("split", at, at + len(w) + 1, w)
            else:
                piece, mark = w, None
            out.append(piece)
            if mark is not None:
                marks.append(mark)
            at += len(piece) + 1
            i += 1
        texts.append(" ".join(out))
        errors.append(marks)
        assert all(texts[-1][a:b].replace(" ", "") == t.replace(" ", "") for _, a, b, t in marks)
    return texts, errors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexicon_boundaries.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--large-queries", type=int, default=20000)
    ap.add_argument("--host-queries", type=int, default=100)
    ap.add_argument("--documents", type=int, default=32)
    ap.add_argument("--recall-documents", type=int, default=4)
    ap.add_argument("--max-dist", type=int, default=2)
    ap.add_argument("--min-part", type=int, default=2)
    ap.add_argument("--per-word", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.03)
    ap.add_argument("--suspect-share", type=float, default=0.02)
    ap.add_argument("-k", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lexicon_boundaries: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk, windows
    sync = torch.cuda.synchronize
    repeats, host_repeats = max(5, args.repeats), max(1, args.host_repeats)
    D, P, K = args.max_dist, args.min_part, args.per_word
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_lexicon_boundaries", "device": torch.cuda.get_device_name(0), "repeats": repeats,
              "host_repeats": host_repeats, "max_dist": D, "min_part": P, "per_word": K, "share": args.share,
              "suspect_share": args.suspect_share, "k": args.k, "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1)}
    rng = np.random.default_rng(2028)
    encode = lambda words: (windows.encode("".join(words), rater.mapping[0]).astype(np.int32),
                            np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)

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

    name, docs, streams = corpus_sets(0.16)[0]
    lexicon = rater.lexicon(distinct_words(docs))
    texts, errors = planted(rng, docs, args.share, P)
    chars_d, order_d = lexicon.on_device(lm)
    print("%s: lexicon of %d entries, %d ids" % (name, len(lexicon), len(lexicon.pool)), file=sys.stderr)

    # ---- (a) the kernel against the parent's look-up and against the numpy statement
    words = distinct_words(texts)
    sizes = {"small": encode(words[:args.queries]), "large": encode(words[:args.large_queries])}
    host = encode(words[:args.host_queries])

    def splits(q):
        res = lm.lexicon_splits(chars_d, order_d, lexicon.class_first, rater.voc_size, up(q[0]), up(q[1]), D, P, K)
        return [t.cpu().numpy() for t in res]

    def neighbours(q):
        res = lm.lexicon_neighbours(chars_d, order_d, lexicon.class_first, rater.voc_size, up(q[0]), up(q[1]), D, K)
        return [t.cpu().numpy() for t in res]

    def numpy_leg():
        return ratebulk.lexicon_splits_host(host[0], host[1], lexicon.chars, lexicon.order, lexicon.class_first, rater.voc_size, D, P, K)

    def entries_walked(q_off, low, high):
        m = np.diff(q_off)
        m = m[(m >= 1) & (m <= 64)]
        first = lexicon.class_first      # (first[L]: the entries shorter than L)
        return int((first[np.clip(high(m), 0, 64) + 1] - first[np.clip(low(m), 1, 65)]).clip(min=0).sum())

    ts = []
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        want = numpy_leg()
        ts.append(time.perf_counter() - t0)
    got = splits(sizes["large"])
    assert all(np.array_equal(g[:len(w)], w) for g, w in zip(got, want)), "kernel and numpy statement disagree"
    kernel = {"lexicon_entries": len(lexicon), "lexicon_ids": int(len(lexicon.pool)), "host_queries": len(host[1]) - 1,
              "numpy": summary(ts), "numpy_seconds_per_query": summary(ts)["seconds"] / max(len(host[1]) - 1, 1)}
    for size, q in sizes.items():
        row = {"queries": len(q[1]) - 1, "with_splits": int((splits(q)[0] > 0).sum()),
               # entries a query is compared with: twice the classes below it, against once the classes around it
               "entries_walked_splits": 2 * entries_walked(q[1], lambda m: m * 0 + max(1, P - (D - 1)), lambda m: m - P + (D - 1)),
               "entries_walked_neighbours": entries_walked(q[1], lambda m: m - D, lambda m: m + D)}
        row.update(device_times({"splits": lambda q=q: splits(q), "neighbours": lambda q=q: neighbours(q)}))
        row["splits_over_neighbours"] = row["splits"]["seconds"] / row["neighbours"]["seconds"]
        row["splits"]["entries_per_s"] = row["entries_walked_splits"] / row["splits"]["seconds"]
        row["neighbours"]["entries_per_s"] = row["entries_walked_neighbours"] / row["neighbours"]["seconds"]
        kernel[size] = row
        print("%d queries: splits %.4f s, neighbours %.4f s (x%.2f)" % (row["queries"], row["splits"]["seconds"],
                                                                       row["neighbours"]["seconds"], row["splits_over_neighbours"]),
              file=sys.stderr)
    kernel["speedup_over_numpy"] = kernel["numpy_seconds_per_query"] / (kernel["large"]["splits"]["seconds"] / kernel["large"]["queries"])
    result["kernel"] = kernel
    print("numpy %.2f s for %d queries" % (kernel["numpy"]["seconds"], kernel["host_queries"]), file=sys.stderr)

    # ---- (b) the share of planted errors whose true form is offered, every word looked up
    part, marks = texts[:args.recall_documents], errors[:args.recall_documents]
    everything = dict(k=args.k, streams=streams, max_prob=1.0, min_rank=0, min_suspects=0, precision="bf16")
    recall = {"documents": len(part), "planted": dict((kind, sum(1 for one in marks for m in one if m[0] == kind and m[1] >= 1))
                                                      for kind in ("merged", "split"))}
    for leg, flag in (("plain", False), ("boundaries", True)):
        _, rescored, _ = rater.correct_words(part, lexicon, context, max_dist=D, per_word=K, boundaries=flag, min_part=P, **everything)
        hits = dict(merged=0, split=0)
        for one, mine in zip(rescored, marks):
            offered = dict(((int(a), int(b)), one.candidates[int(f):int(g)]) for a, b, f, g in zip(one.starts, one.ends, one.first[:-1], one.first[1:]))
            for kind, a, b, truth in mine:
                hits[kind] += int(a >= 1 and truth in offered.get((a, b), ()))
        recall[leg] = dict(("%s_offered" % kind, hits[kind] / max(recall["planted"][kind], 1)) for kind in hits)
        recall[leg]["edits"] = sum(len(one) for one in rescored)
    result["recall"] = recall
    print("recall %r" % (recall,), file=sys.stderr)

    # ---- (c) correct_words without and with the flag, the suspect words chosen by the model
    part = texts[:args.documents]
    probs, _ = rater.rate_batch(part, context, streams=streams, precision="bf16")
    max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
    del probs
    rule = dict(k=args.k, streams=streams, max_prob=max_prob, min_rank=1, precision="bf16")
    correct = lambda flag: rater.correct_words(part, lexicon, context, max_dist=D, per_word=K, boundaries=flag, min_part=P, **rule)
    plain, wide = correct(False), correct(True)
    row = {"documents": len(part), "chars": sum(len(t) for t in part), "streams": streams, "max_prob": max_prob,
           "suspect_words": sum(len(f) for f in plain[0]),
           "edits": sum(len(one) for one in plain[1]), "edits_boundaries": sum(len(one) for one in wide[1]),
           "candidates": sum(len(one.candidates) for one in plain[1]), "candidates_boundaries": sum(len(one.candidates) for one in wide[1])}
    row.update(device_times({"correct": lambda: correct(False), "correct_boundaries": lambda: correct(True)}))
    row["boundaries_over_plain"] = row["correct_boundaries"]["seconds"] / row["correct"]["seconds"]
    result["correct_words"] = row
    print("correct %.3f s, with boundaries %.3f s (x%.2f); %d -> %d edits" % (row["correct"]["seconds"], row["correct_boundaries"]["seconds"],
                                                                              row["boundaries_over_plain"], row["edits"], row["edits_boundaries"]),
          file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
