#!/usr/bin/env python3
"""Lexicon look-up under learned confusions: the weighted search on the device (kl_lexicon_channel, `Rater.lexicon_neighbours`
and `Rater.correct_words` with a channel) against its numpy statement (`ratebulk.lexicon_channel_host`), against the unit-cost
look-up it stands beside (kl_lexicon_neighbours at max_dist 2), and -- the figure that says whether it earns its place -- how
often the true form of a corrupted word is among its candidates under either.

  python tools/bench_lexicon_channel.py [--out profiles/lexicon_channel.json] [--repeats 5] [--host-repeats 1] [--queries 2000]
                                        [--large-queries 20000] [--host-queries 100] [--recall-words 20000] [--documents 32]
                                        [--max-bits 12] [--unit-bits 8] [--max-dist 2] [--per-word 8] [--noise 0.005]

The lexicon and the texts are bench_lexicon.py's first set (cfg2 size; 1024 documents of 2048 characters, a space with
probability 0.16; the lexicon is the distinct words of the clean corpus, 228 576 entries).  The OCR is bench_confusions.py's:
its planted table of 12 confusions -- eight of one character for one, four where the OCR writes TWO characters for one -- at
5 to 30 % of the occurrences plus uniform noise (--noise).  The channel is learned from these pairs with `Rater.confusions` and
`Rater.channel` (defaults: min_count 2), nothing of the planted table is handed over.  Legs:
  (a) "kernel" / "kernel_large": `HipLM.lexicon_channel` on the --queries / --large-queries first distinct words of the OCR
      (upload of the queries, the call, download; lexicon and rules are on the device) at --max-bits; "numpy": the statement on
      the first --host-queries of them (Python over every cell: it does not get through more in a benchmark's time), all four
      outputs asserted identical to the kernel's; "unit" / "unit_large": kl_lexicon_neighbours at --max-dist on the same words.
      "dp_over_bit_parallel" is kernel_large / unit_large: the DP is expected to be several times slower, recorded, not gated.
  (b) "recall": --recall-words entries of the lexicon that hold a planted character, each corrupted by ONE planted confusion;
      the share whose true form is among the --per-word candidates under the channel and under unit costs, split by single-
      (one for one) and multi-character (two for one) confusions.
  (c) "correct_channel" / "correct_unit": `Rater.correct_words` on the first --documents OCR documents with and without the
      channel: the time, the edits and the proposals.
On a trained model and a real table: not measured -- weights are random (seed 3) and the table is planted, so (c) says what
the step costs, not what it corrects.  Host clock around work that ends in a device synchronise; every leg is warmed up once;
the device legs take the median of --repeats (at least 5) timings, each of at least --min-seconds, the numpy leg the median of
--host-repeats single runs; the spread is (max - min) / median.  One JSON line on stdout, also written to --out.

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

from tools.bench_confusions import ocr_of, planted_table      # noqa: E402
from tools.bench_lexicon import distinct_words, summary      # noqa: E402
from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater, timed      # noqa: E402
from tools.bench_words import corpus_sets      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexicon_channel.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--large-queries", type=int, default=20000)
    ap.add_argument("--host-queries", type=int, default=100)
    ap.add_argument("--recall-words", type=int, default=20000)
    ap.add_argument("--documents", type=int, default=32)
    ap.add_argument("--max-bits", type=float, default=12.0)
    ap.add_argument("--unit-bits", type=float, default=8.0)
    ap.add_argument("--max-dist", type=int, default=2)
    ap.add_argument("--per-word", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.005)
    ap.add_argument("--suspect-share", type=float, default=0.02)
    ap.add_argument("-k", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lexicon_channel: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk, windows
    sync = torch.cuda.synchronize
    repeats, host_repeats = max(5, args.repeats), max(1, args.host_repeats)
    D, K = args.max_dist, args.per_word
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    context = [17]
    planted = planted_table()
    rng = np.random.default_rng(2031)
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

    name, truths, streams = corpus_sets(0.16)[0]
    lexicon = rater.lexicon(distinct_words(truths))
    texts = [ocr_of(rng, t, planted, args.noise) for t in truths]
    found = rater.confusions(texts, truths, max_dist=128)
    channel = rater.channel(found, unit_bits=args.unit_bits)
    max_cost = int(round(ratebulk.CHANNEL_SCALE * args.max_bits))
    chars_d, order_d = lexicon.on_device(lm)
    rules_d, cost_d = channel.on_device(lm)
    print("%s: lexicon of %d entries; %d records learned, %d rules kept (dropped %r), unit %d, max_cost %d"
          % (name, len(lexicon), len(found), len(channel), channel.dropped, channel.unit, max_cost), file=sys.stderr)
    result = {"tool": "bench_lexicon_channel", "device": torch.cuda.get_device_name(0), "repeats": repeats,
              "host_repeats": host_repeats, "max_bits": args.max_bits, "unit_bits": args.unit_bits, "max_dist": D, "per_word": K,
              "noise": args.noise, "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "set": name,
              "lexicon_entries": len(lexicon), "planted": [[read, truth, rate] for read, truth, rate in planted],
              "records": len(found), "rules": len(channel), "dropped": channel.dropped, "cer": found.cer,
              "trained_model_and_real_table": "not measured"}

    # ---- (a) the kernel against its statement and against the unit-cost look-up
    words = distinct_words(texts)
    small, large, few = encode(words[:args.queries]), encode(words[:args.large_queries]), encode(words[:args.host_queries])

    def weighted(q):
        res = lm.lexicon_channel(chars_d, order_d, lexicon.class_first, rater.voc_size, up(q[0]), up(q[1]), rules_d, cost_d,
                                 channel.unit, max_cost, K)
        return [t.cpu().numpy() for t in res]

    def unit(q):
        res = lm.lexicon_neighbours(chars_d, order_d, lexicon.class_first, rater.voc_size, up(q[0]), up(q[1]), D, K)
        return [t.cpu().numpy() for t in res]

    def numpy_leg():
        return ratebulk.lexicon_channel_host(few[0], few[1], lexicon.chars, lexicon.order, lexicon.class_first, rater.voc_size,
                                             channel.rules, channel.cost, channel.unit, max_cost, K)

    ts, want = [], None
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        want = numpy_leg()
        ts.append(time.perf_counter() - t0)
    got, again = weighted(few), weighted(large)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "kernel and numpy statement disagree"
    assert all(np.array_equal(g[:len(w)], w) for g, w in zip(again, want))
    row = {"queries": len(small[1]) - 1, "large_queries": len(large[1]) - 1, "host_queries": len(few[1]) - 1,
           "with_exact": int((again[0] >= 0).sum()), "with_candidates": int((again[1] > 0).sum()),
           "candidates_found_mean": float(again[1].mean()), "numpy": summary(ts)}
    row.update(device_times({"kernel": lambda: weighted(small), "kernel_large": lambda: weighted(large),
                             "kernel_host_queries": lambda: weighted(few), "unit": lambda: unit(small),
                             "unit_large": lambda: unit(large)}))
    row["speedup_over_numpy"] = row["numpy"]["seconds"] / row["kernel_host_queries"]["seconds"]
    row["dp_over_bit_parallel"] = row["kernel_large"]["seconds"] / row["unit_large"]["seconds"]
    result["kernel"] = row
    print("kernel %.4f s at %d, %.4f s at %d queries; unit-cost look-up %.4f s / %.4f s (DP / bit-parallel %.1fx); numpy %.2f s "
          "at %d queries (kernel %.4f s, %.0fx)"
          % (row["kernel"]["seconds"], row["queries"], row["kernel_large"]["seconds"], row["large_queries"], row["unit"]["seconds"],
             row["unit_large"]["seconds"], row["dp_over_bit_parallel"], row["numpy"]["seconds"], row["host_queries"],
             row["kernel_host_queries"]["seconds"], row["speedup_over_numpy"]), file=sys.stderr)

    # ---- (b) is the true form among the candidates?
    index = dict((w, i) for i, w in enumerate(lexicon.words))
    holders = [w for w in lexicon.words if any(truth in w for _, truth, _ in planted)]
    picked = [holders[int(i)] for i in rng.permutation(len(holders))[:args.recall_words]]
    corrupted, true_at, multi = [], [], []
    for w in picked:
        fits = [(read, truth) for read, truth, _ in planted if truth in w]
        read, truth = fits[int(rng.integers(0, len(fits)))]
        places = [p for p, c in enumerate(w) if c == truth]
        p = places[int(rng.integers(0, len(places)))]
        bad = w[:p] + read + w[p + 1:]
        if len(bad) <= 64:
            corrupted.append(bad)
            true_at.append(index[w])
            multi.append(len(read) > 1)
    true_at, multi = np.asarray(true_at), np.asarray(multi)
    q = encode(corrupted)
    hit = {"channel": (weighted(q)[2] == true_at[:, None]).any(axis=1), "unit": (unit(q)[2] == true_at[:, None]).any(axis=1)}
    share = lambda flags, kind: float(flags[kind].mean()) if kind.any() else None
    result["recall"] = {"words": len(corrupted), "single": int((~multi).sum()), "multi": int(multi.sum()),
                        "channel": {"all": share(hit["channel"], multi | ~multi), "single": share(hit["channel"], ~multi),
                                    "multi": share(hit["channel"], multi)},
                        "unit": {"all": share(hit["unit"], multi | ~multi), "single": share(hit["unit"], ~multi),
                                 "multi": share(hit["unit"], multi)}}
    print("true form among the %d candidates: channel %r, unit costs at max_dist %d %r"
          % (K, result["recall"]["channel"], D, result["recall"]["unit"]), file=sys.stderr)

    # ---- (c) correct_words with and without the channel
    part = texts[:args.documents]
    probs, _ = rater.rate_batch(part, context, streams=streams, precision="bf16")
    max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
    del probs
    rule = dict(k=args.k, streams=streams, max_prob=max_prob, min_rank=1, precision="bf16", per_word=K)
    legs = {"correct_channel": lambda: rater.correct_words(part, lexicon, context, channel=channel, max_bits=args.max_bits, **rule),
            "correct_unit": lambda: rater.correct_words(part, lexicon, context, max_dist=D, **rule)}
    row = {"documents": len(part), "chars": sum(len(t) for t in part), "streams": streams, "max_prob": max_prob}
    for leg, fn in legs.items():
        _, rescored, _ = fn()
        row[leg] = {"edits": sum(len(one) for one in rescored), "candidates": sum(len(one.candidates) for one in rescored),
                    "proposals": sum(int((one.best >= 0).sum()) for one in rescored)}
    for leg, times in device_times(legs).items():
        row[leg].update(times)
    result["correct_words"] = row
    print("correct_words on %d documents: channel %.3f s (%d edits, %d proposals), unit costs %.3f s (%d edits, %d proposals)"
          % (len(part), row["correct_channel"]["seconds"], row["correct_channel"]["edits"], row["correct_channel"]["proposals"],
             row["correct_unit"]["seconds"], row["correct_unit"]["edits"], row["correct_unit"]["proposals"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
