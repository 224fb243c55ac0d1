#!/usr/bin/env python3
"""Rescoring caller-supplied replacements over a corpus: `Rater.rescore(precision="bf16")` against the same answer with the
hypothesis windows built in numpy on the host and uploaded -- `ratebulk.span_windows_host`, `rate_window_bulk`,
`ratebulk.span_pick_host`.  The parent commit cannot rescore spans at all: the numpy baseline of the same commit is the yardstick.

  python tools/bench_rescore.py [--out profiles/rate_rescore.json] [--repeats 5] [--suspect-share 0.02] [--min-rank 1]
                                [--left 64] [--ahead 8] [--min-gain 1.0]

The corpus-sized inputs of bench_corrections.py, cfg2 size (depth 2, width 512, length 256): 1024 documents of 2048 characters
and 20 000 lines of 30 to 90 characters, both at 1024 streams.  The edits are the occurrences of a table of OCR confusions
(rn <-> m, ii <-> n, cl <-> d, vv <-> w, l / 1 / I, ...: `ratebatch.confusion_edits`) that hold a suspect character; as in
bench_corrections.py `max_prob` is set per corpus to the --suspect-share quantile of the bf16 probabilities (2 %: an OCR-like
error rate).  The suspects pass and the edit list are made once, outside the timings: both legs start from the same edits.
Legs:
  "rescore"       Rater.rescore(precision="bf16"): ids, offsets, contexts, spans and candidate pool uploaded once, the
                  hypothesis windows built on the device (kl_span_windows), the choice made there (kl_span_pick);
  "baseline"      the same host preparation, then per chunk (the same chunks) ratebulk.span_windows_host -> upload -> zero states
                  -> rate_window_bulk -> the rows' bits, one transfer of all bits at the end, ratebulk.span_pick_host;
  "windows"       the device windows of all chunks alone: its share of the "rescore" leg is reported; "windows_host" is the same
                  for span_windows_host and the "baseline" leg;
  "prepare_host"  the host preparation both legs share (texts and candidates normalised, each kind encoded as one string, the
                  span arrays): its share of either leg is reported.
Also reported, from one run each outside the timings: that both legs give identical costs and choices.
Host clock around work that ends in a device synchronise; every leg is warmed up once, then the legs are alternated in the
same process; a leg is repeated inside one timing until it lasts at least --min-seconds; the median of --repeats (at least
5) timings and the spread (max - min) / median.  One JSON line on stdout, also written to --out.

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
from tools.bench_suspects import corpus_sets      # noqa: E402

CONFUSIONS = [("rn", ["m"]), ("m", ["rn", "nn"]), ("ii", ["n", "u"]), ("n", ["ii", "u", "ri"]), ("cl", ["d"]), ("d", ["cl", "ol"]),
              ("vv", ["w"]), ("w", ["vv", "v"]), ("l", ["1", "I", "i"]), ("1", ["l", "I"]), ("I", ["l", "1"]), ("O", ["0", "Q"]),
              ("0", ["O", "o"]), ("e", ["c", "o"]), ("c", ["e", "o"]), ("o", ["e", "0", "c"]), ("u", ["n", "ii"]),
              ("h", ["b", "li"]), ("b", ["h", "lo"]), ("s", ["f", "5"]), ("f", ["s", "t"]), ("t", ["f", "l"]),
              (".", [",", ""]), (",", [".", ""]), ("'", ["", "`"]), (" ", [""]), ("-", ["", "="])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_rescore.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--suspect-share", type=float, default=0.02)
    ap.add_argument("--min-rank", type=int, default=1)
    ap.add_argument("--left", type=int, default=64)
    ap.add_argument("--ahead", type=int, default=8)
    ap.add_argument("--min-gain", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rescore: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebatch, ratebulk, windows
    sync = torch.cuda.synchronize
    repeats = max(5, args.repeats)
    left, ahead = args.left, args.ahead
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)      # (as bench_rate_batch --bulk: peaked distributions)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_rescore", "device": torch.cuda.get_device_name(0), "repeats": repeats,
              "suspect_share": args.suspect_share, "min_rank": args.min_rank, "left": left, "ahead": ahead,
              "min_gain": args.min_gain, "rules": len(CONFUSIONS), "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1),
              "sets": {}}
    for name, docs, streams in corpus_sets():
        chars = sum(len(d) for d in docs)
        probs, _ = rater.rate_batch(docs, context, streams=streams, precision="bf16")
        max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
        del probs
        found, _ = rater.suspects(docs, context, k=args.k, streams=streams, max_prob=max_prob, min_rank=args.min_rank)
        edits = ratebatch.confusion_edits(docs, CONFUSIONS, at=[f.positions for f in found])
        del found
        held = {}

        def rescore():
            return rater.rescore(docs, edits, context, streams=streams, left=left, ahead=ahead, min_gain=args.min_gain)

        def prepare_host():
            texts = [windows.normalize(t) for t in docs]
            offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
            corpus = windows.encode("".join(texts), rater.mapping[0]).astype(np.int32)
            strings = [windows.normalize(c) for e in edits for c in e[3]]
            text = np.asarray([e[0] for e in edits], dtype=np.int32)
            spans = dict(span_text=text, span_start=np.asarray([e[1] for e in edits], dtype=np.int64) + offsets[text],
                         span_len=np.asarray([e[2] - e[1] for e in edits], dtype=np.int32),
                         span_first=np.concatenate([[0], np.cumsum([len(e[3]) for e in edits])]).astype(np.int64),
                         pool=windows.encode("".join(strings), rater.mapping[0]).astype(np.int32),
                         cand_off=np.concatenate([[0], np.cumsum([len(c) for c in strings])]).astype(np.int64))
            M = max([1] + [int(spans["span_len"].max())] + [len(c) for c in strings])
            text_ctx = np.asarray([windows.clamp_context(context)] * len(docs), dtype=np.int32)
            return corpus, offsets, text_ctx, spans, M

        def host_windows(prepared, a, b):
            corpus, offsets, text_ctx, spans, M = prepared
            return ratebulk.span_windows_host(corpus, offsets, text_ctx, row0=a, rows=b - a, left=left, ahead=ahead, max_len=M,
                                              T=max(left + ahead + M - 1, ratebulk.MIN_T), **spans)

        def baseline():
            prepared = prepare_host()
            first = prepared[3]["span_first"]
            cost, valid = [], []
            for a, b in ratebulk.span_chunks(first, streams):
                x, z, y, ok = host_windows(prepared, a, b)
                lm.reset_states(len(x))
                lm.rate_window_bulk(x, z, y, want_probs=False)
                cost.append(lm.rate_bits_take_all())
                valid.append(ok)
            cost = torch.cat(cost).cpu().numpy()
            lm.rate_status_check()
            lm.reset_states(1)
            return ratebulk.span_pick_host(cost, np.concatenate(valid), first, args.min_gain)

        def windows_device():
            where, spans, M, first = held["device"]
            for a, b in ratebulk.span_chunks(first, streams):
                lm.span_windows(*(where + spans), row0=a, rows=b - a, left=left, ahead=ahead, max_len=M,
                                T=max(left + ahead + M - 1, ratebulk.MIN_T))

        def windows_host():
            for a, b in ratebulk.span_chunks(held["host"][3]["span_first"], streams):
                host_windows(held["host"], a, b)

        # one run of each outside the timings: the two legs agree
        got = rescore()
        best, gain, cost = baseline()
        order = np.argsort(np.asarray([e[0] for e in edits]), kind="stable")      # (rescore's results: text by text)
        first = np.concatenate([[0], np.cumsum([len(e[3]) for e in edits])])
        rows = np.concatenate([np.arange(first[s] + s, first[s + 1] + s + 1) for s in order] + [np.zeros(0, dtype=np.int64)])
        mine = np.concatenate([np.concatenate([[c0], f.cost[int(a):int(b)]])
                               for f in got for c0, a, b in zip(f.cost0, f.first[:-1], f.first[1:])] + [np.zeros(0)])
        identical = bool(np.array_equal(mine.view(np.uint64), cost[rows.astype(np.int64)].view(np.uint64))
                         and np.array_equal(np.concatenate([f.best for f in got]), best[order])
                         and np.array_equal(np.concatenate([f.gain for f in got]).view(np.uint64), gain[order].view(np.uint64)))
        prepared = prepare_host()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
        held.update(host=prepared, device=([up(prepared[0]), up(prepared[1]), up(prepared[2])],
                                           [up(prepared[3][n]) for n in ("span_text", "span_start", "span_len", "span_first", "pool",
                                                                        "cand_off")], prepared[4], prepared[3]["span_first"]))
        legs = {"rescore": rescore, "baseline": baseline, "windows": windows_device, "windows_host": windows_host,
                "prepare_host": prepare_host}
        inner = {}
        for leg, fn in legs.items():
            fn()
            inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        times = dict((leg, []) for leg in legs)
        for _ in range(repeats):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, sync, inner[leg]))
        held.clear()
        n_rows = len(edits) + int(first[-1])
        row = {"documents": len(docs), "chars": chars, "streams": streams, "max_prob": max_prob, "spans": len(edits),
               "rows": n_rows, "longest_span_or_candidate": prepared[4], "window_length": max(left + ahead + prepared[4] - 1, 3),
               "chunks": len(ratebulk.span_chunks(prepared[3]["span_first"], streams)),
               "proposals_kept": int((best >= 0).sum()), "costs_identical_to_baseline": identical,
               "bytes_from_device": n_rows * 8 + len(edits) * 12}
        for leg, ts in times.items():
            med = statistics.median(ts)
            row[leg] = {"rows_per_s": n_rows / med, "seconds": med, "spread": (max(ts) - min(ts)) / med, "runs_per_timing": inner[leg]}
        row["speedup"] = row["baseline"]["seconds"] / row["rescore"]["seconds"]
        row["windows_share"] = row["windows"]["seconds"] / row["rescore"]["seconds"]
        row["windows_host_share_of_baseline"] = row["windows_host"]["seconds"] / row["baseline"]["seconds"]
        row["prepare_host_share"] = row["prepare_host"]["seconds"] / row["rescore"]["seconds"]
        row["prepare_host_share_of_baseline"] = row["prepare_host"]["seconds"] / row["baseline"]["seconds"]
        result["sets"][name] = row
        print("%-16s rescore %9.0f  baseline %9.0f rows/s (%.2fx)  %d spans, %d rows  windows %.1f %% (host: %.1f %% of baseline)  "
              "prepare %.1f %%  identical %s" % (name, row["rescore"]["rows_per_s"], row["baseline"]["rows_per_s"], row["speedup"],
                                                  len(edits), n_rows, 100.0 * row["windows_share"],
                                                  100.0 * row["windows_host_share_of_baseline"], 100.0 * row["prepare_host_share"],
                                                  identical), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
