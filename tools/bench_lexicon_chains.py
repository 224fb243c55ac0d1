#!/usr/bin/env python3
"""Lexicon chains: kl_lexicon_chains beside the family's other look-ups of the same words (kl_lexicon_neighbours,
kl_lexicon_splits), the share of words that lost TWO spaces for which `Rater.correct_words` offers the true form with
max_parts=3 and with the pairs alone, and how many planted compounds are offered a "correction" with and without `compounds`.

  python tools/bench_lexicon_chains.py [--out profiles/lexicon_chains.json] [--repeats 5] [--queries 2000]
                                       [--large-queries 20000] [--recall-documents 4] [--max-dist 2] [--min-part 2]
                                       [--max-parts 4] [--per-word 8] [--share 0.03]

The corpus and the lexicon are bench_lexicon.py's first set (1024 documents of 2048 characters, a space with probability 0.16,
254 other characters; the lexicon is the distinct words of the clean corpus in order of first occurrence).  Legs:
  (a) "chains" / "neighbours" / "splits": the --queries (and --large-queries) first distinct words of the documents with lost
      spaces through `HipLM.lexicon_chains` (max_parts, min_part, the link `s`), `HipLM.lexicon_neighbours` and
      `HipLM.lexicon_splits` (both at max_dist), queries and lexicon on the device, timed by device events around the call:
      the median of --repeats (at least 5) after one warm-up call each, alternated; the spread is (max - min) / median.  The
      chains walk the length classes min_part .. m, the neighbours m - max_dist .. m + max_dist: "entries_walked" counts the
      (query, entry) pairs of each, "entries_per_s" divides by the time.  This is a record, not a gate.
  (b) "recall": the first --recall-documents documents in which --share of the places with two spaces in a row of three words
      lost both (the truth is `a b c`), EVERY word selected (max_prob 1, min_rank 0, min_suspects 0), so that the figure is the
      look-ups' and not the model's, which is untrained here: the share of the planted spans for which `correct_words` hands
      `rescore` an edit over exactly the span with the true form among its candidates, with boundaries=True alone and with
      max_parts=3, in the same run.
  (c) "compounds": a list of compounds, each 2 .. 3 random entries of at least min_part characters run together, an `s` behind
      the first in a third of them, takes the place of --share of the words of the same documents; every word selected again:
      how many of the planted compounds get candidates (boundaries=True, so that a split is one) without and with
      compounds=3, links=("s",).
Results on a trained model and a real word list are unmeasured: the corpus is random, so a "word" is a random string and the
lexicon holds no natural compounds.  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_lexicon import distinct_words, summary      # noqa: E402
from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater      # noqa: E402
from tools.bench_words import corpus_sets      # noqa: E402


def two_lost(rng, docs, share):
    """the texts with three words run together at `share` of the places, and per text the planted spans as (start, end,
    truth) in the new text"""
    texts, marks = [], []
    for d in docs:
        words = d.split(" ")
        out, mine, at, i = [], [], 0, 0
        while i < len(words):
            three = words[i:i + 3]
            if len(three) == 3 and all(three) and sum(len(w) for w in three) < 64 and rng.random() < share:
                piece = "".join(three)
                mine.append((at, at + len(piece), " ".join(three)))
                i += 2
            else:
                piece = words[i]
            out.append(piece)
            at += len(piece) + 1
            i += 1
        texts.append(" ".join(out))
        marks.append(mine)
        assert all(texts[-1][a:b] == t.replace(" ", "") for a, b, t in mine)
    return texts, marks


def with_compounds(rng, docs, share, compounds):
    """the texts with `share` of the words replaced by a compound, and per text the planted spans as (start, end)"""
    texts, marks = [], []
    for d in docs:
        out, mine, at = [], [], 0
        for w in d.split(" "):
            if w and rng.random() < share:
                w = compounds[int(rng.integers(0, len(compounds)))]
                mine.append((at, at + len(w)))
            out.append(w)
            at += len(w) + 1
        texts.append(" ".join(out))
        marks.append(mine)
    return texts, marks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexicon_chains.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--large-queries", type=int, default=20000)
    ap.add_argument("--recall-documents", type=int, default=4)
    ap.add_argument("--max-dist", type=int, default=2)
    ap.add_argument("--min-part", type=int, default=2)
    ap.add_argument("--max-parts", type=int, default=4)
    ap.add_argument("--per-word", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.03)
    ap.add_argument("-k", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lexicon_chains: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk, windows
    repeats = max(5, args.repeats)
    D, P, K, N = args.max_dist, args.min_part, args.per_word, args.max_parts
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_lexicon_chains", "device": torch.cuda.get_device_name(0), "repeats": repeats, "max_dist": D,
              "min_part": P, "max_parts": N, "per_word": K, "share": args.share, "k": args.k,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1),
              "unmeasured": "a trained model and a real word list: the corpus is random strings"}
    rng = np.random.default_rng(2029)
    encode = lambda words: (windows.encode("".join(words), rater.mapping[0]).astype(np.int32),
                            np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)

    name, docs, streams = corpus_sets(0.16)[0]
    lexicon = rater.lexicon(distinct_words(docs))
    texts, marks = two_lost(rng, docs, args.share)
    chars_d, order_d = lexicon.on_device(lm)
    links = ratebulk.lexicon_links_host([[rater.mapping[0]["s"]]], rater.voc_size)
    print("%s: lexicon of %d entries, %d ids" % (name, len(lexicon), len(lexicon.pool)), file=sys.stderr)

    # ---- (a) the kernel beside the family's other look-ups, by device events
    words = distinct_words(texts)
    first = lexicon.class_first      # (first[L]: the entries shorter than L)

    def entries_walked(q_off, low, high):
        m = np.diff(q_off)
        m = m[(m >= 1) & (m <= 64)]
        return int((first[np.clip(high(m), 0, 64) + 1] - first[np.clip(low(m), 1, 65)]).clip(min=0).sum())

    def event_times(legs):
        times = dict((leg, []) for leg in legs)
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for leg, fn in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[leg].append(t0.elapsed_time(t1) * 1e-3)
        return dict((leg, summary(ts)) for leg, ts in times.items())

    kernel = {"lexicon_entries": len(lexicon), "lexicon_ids": int(len(lexicon.pool))}
    for size, count in (("small", args.queries), ("large", args.large_queries)):
        pool, off = encode(words[:count])
        pool_d, off_d = up(pool), up(off)
        common = (chars_d, order_d, lexicon.class_first, rater.voc_size, pool_d, off_d)
        legs = {"chains": lambda: lm.lexicon_chains(*common, links, N, P),
                "neighbours": lambda: lm.lexicon_neighbours(*common, D, K),
                "splits": lambda: lm.lexicon_splits(*common, D, P, K)}
        found = legs["chains"]()[0].cpu().numpy()
        row = {"queries": len(off) - 1, "entries": int((found & 1).sum()), "chains_of_two_or_more": int(((found >> 1) != 0).sum()),
               "entries_walked": {"chains": entries_walked(off, lambda m: m * 0 + P, lambda m: m),
                                  "neighbours": entries_walked(off, lambda m: m - D, lambda m: m + D),
                                  "splits": 2 * entries_walked(off, lambda m: m * 0 + max(1, P - (D - 1)), lambda m: m - P + (D - 1))}}
        row.update(event_times(legs))
        for leg in legs:
            row[leg]["entries_per_s"] = row["entries_walked"][leg] / row[leg]["seconds"]
        row["chains_over_neighbours"] = row["chains"]["seconds"] / row["neighbours"]["seconds"]
        row["chains_over_splits"] = row["chains"]["seconds"] / row["splits"]["seconds"]
        kernel[size] = row
        print("%d queries: chains %.5f s, neighbours %.5f s, splits %.5f s" % (row["queries"], row["chains"]["seconds"],
                                                                               row["neighbours"]["seconds"], row["splits"]["seconds"]),
              file=sys.stderr)
    result["kernel"] = kernel

    # ---- (b) two lost spaces: the true form among the candidates, every word looked up
    part, mine = texts[:args.recall_documents], marks[:args.recall_documents]
    everything = dict(k=args.k, streams=streams, max_prob=1.0, min_rank=0, min_suspects=0, precision="bf16")
    offered_of = lambda one: dict(((int(a), int(b)), one.candidates[int(f):int(g)])
                                  for a, b, f, g in zip(one.starts, one.ends, one.first[:-1], one.first[1:]))
    recall = {"documents": len(part), "planted": sum(1 for one in mine for m in one if m[0] >= 1)}
    for leg, more in (("boundaries", dict()), ("max_parts_3", dict(max_parts=3))):
        _, rescored, _ = rater.correct_words(part, lexicon, context, max_dist=D, per_word=K, boundaries=True, min_part=P, **more,
                                             **everything)
        hits = 0
        for one, spans in zip(rescored, mine):
            offered = offered_of(one)
            hits += sum(int(a >= 1 and truth in offered.get((a, b), ())) for a, b, truth in spans)
        recall[leg] = {"offered": hits / max(recall["planted"], 1), "edits": sum(len(one) for one in rescored),
                       "candidates": sum(len(one.candidates) for one in rescored)}
    result["recall"] = recall
    print("recall %r" % (recall,), file=sys.stderr)

    # ---- (c) compounds: left alone, or offered a "correction"?
    pieces = [w for w in lexicon.words if P <= len(w) <= 12]
    made = []
    for c in range(200):
        chosen = [pieces[int(i)] for i in rng.integers(0, len(pieces), int(rng.integers(2, 4)))]
        made.append(chosen[0] + ("s" if c % 3 == 0 else "") + "".join(chosen[1:]))
    texts, mine = with_compounds(rng, docs[:args.recall_documents], args.share, made)
    compounds = {"documents": len(texts), "list": len(made), "planted": sum(1 for one in mine for m in one if m[0] >= 1)}
    for leg, more in (("plain", dict()), ("compounds_3", dict(compounds=3, links=("s",)))):
        _, rescored, _ = rater.correct_words(texts, lexicon, context, max_dist=D, per_word=K, boundaries=True, min_part=P, **more,
                                             **everything)
        with_candidates = 0
        for one, spans in zip(rescored, mine):
            offered = offered_of(one)
            with_candidates += sum(int(a >= 1 and len(offered.get((a, b), ())) > 0) for a, b in spans)
        compounds[leg] = {"with_candidates": with_candidates, "edits": sum(len(one) for one in rescored)}
    result["compounds"] = compounds
    print("compounds %r" % (compounds,), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
