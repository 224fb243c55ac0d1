#!/usr/bin/env python3
"""Corrections of a corpus: `Rater.corrections(precision="bf16")` against the same answer from the calls the project had
before it -- `Rater.suspects`, the hypothesis windows built in numpy on the host and uploaded, `rate_window_bulk`, the pick in
numpy.

  python tools/bench_corrections.py [--out profiles/rate_corrections.json] [--repeats 5] [-k 3] [--suspect-share 0.02]
                                    [--min-rank 1] [--left 64] [--ahead 8] [--deletions] [--insertions] [--min-gain 1.0]
                                    [--share-left]

The corpus-sized inputs of bench_suspects.py, cfg2 size (depth 2, width 512, length 256): 1024 documents of 2048 characters
and 20 000 lines of 30 to 90 characters, both at 1024 streams.  The benchmark's model is untrained, and at a fixed threshold
nearly every character of random text would be a suspect; `max_prob` is therefore set per corpus to the --suspect-share
quantile of the bf16 probabilities (2 %: an OCR-like error rate), so that about that share of the characters is rescored.
Legs:
  "corrections"  Rater.corrections(precision="bf16"): corpus, offsets, contexts and selection stay on the device, the
                 hypothesis windows are built there (kl_variant_windows);
  "parent"       Rater.suspects(precision="bf16"), then per chunk of max(1, streams // R) suspects
                 ratebulk.variant_windows_host -> upload -> zero states -> rate_window_bulk -> the rows' bits, one transfer of
                 all bits at the end, ratebulk.variant_pick_host -- the same chunks, the same launches of the model;
  "windows"      the device windows of all chunks alone (kl_variant_windows on the held selection): its share of the
                 "corrections" leg is reported; "windows_host" is the same for variant_windows_host and the "parent" leg.
  "encode_host"  the parent leg's host preparation alone: the texts normalised and encoded once more (Rater.suspects has
                 encoded them already, but does not hand the ids out), suspects and alternatives gathered in corpus order;
                 its share of the "parent" leg is reported, so that the ratio is not credited to the device windows alone.
The parent leg takes a chunk's bits with rate_bits_take(rows), an index upload per chunk; corrections takes all rows at once.
Also reported, from one run each outside the timings: that both legs give identical costs, and the largest
|cost_bf16 - cost_split| over the variants of the suspects both precisions found with the same alternatives.
--insertions measures every set twice in the same run, first as without the flag and then with insertion hypotheses
(`Rater.corrections(insertions=True)`, R = 2k + 1 + deletions rows per suspect; the parent leg builds the same rows with
variant_windows_host(insertions=1)), adds a "first_pass" leg (Rater.suspects alone) so that the second pass of either can be
told apart, and writes the result under the key "insertions" of --out, whose other content stays as it is.
--share-left measures `Rater.corrections(share_left=True)` -- a suspect's left context read once for all its variants
(kl_prefix_windows, kl_state_fanout) -- against the call without the flag, the two alternated in the same run, beside a
"first_pass" leg (Rater.suspects alone), and nothing else: per set the key "share_left" of that set in --out, whose other
content stays as it is, with both legs' seconds and spread, the share of the suspects that took the shared route (those with
--left characters in front of them in their text), the window calls of each kind, the largest |cost_shared - cost_unshared|
in bits (beside the file's |cost_bf16 - cost_split|) and whether the kept proposals are identical.  The lines are measured
once more at --left 16, shared against unshared, under the key "share_left_left16": few suspects of a short line have 64
characters in front of them.
Host clock around work that ends in a device synchronise; every leg is warmed up once, then the legs are alternated in the
same process; a leg is repeated inside one timing until it lasts at least --min-seconds; the median of --repeats (at least
5) timings and the spread (max - min) / median.  One JSON line on stdout, also written to --out.

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

from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater, timed      # noqa: E402
from tools.bench_suspects import corpus_sets      # noqa: E402


def share_left_run(args, rater, context, repeats, sync):
    """--share-left: the shared call against the unshared one per set, the lines once more at left = 16; written under keys
    of their own of every set of --out"""
    k, deletions, insertions = args.k, bool(args.deletions), bool(args.insertions)
    whole = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            whole = json.load(f)
    for name, docs, streams in corpus_sets():
        chars = sum(len(d) for d in docs)
        probs, _ = rater.rate_batch(docs, context, streams=streams, precision="bf16")
        max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
        del probs
        common = dict(k=k, streams=streams, max_prob=max_prob, min_rank=args.min_rank)
        for key, left in [("share_left", args.left)] + ([("share_left_left16", 16)] if "lines" in name else []):
            def corrections(share_left=False):
                return rater.corrections(docs, context, left=left, ahead=args.ahead, deletions=deletions, min_gain=args.min_gain,
                                         precision="bf16", insertions=insertions, share_left=share_left, **common)

            # one run of each outside the timings: the costs side by side, the kept proposals
            found, _ = corrections()
            shared, _ = corrections(True)
            stats = dict(rater.shared_left or {})
            worst, same = 0.0, True
            for a, b in zip(found, shared):
                same &= bool(np.array_equal(a.positions, b.positions) and np.array_equal(np.isinf(a.cost), np.isinf(b.cost)))
                both = np.isfinite(a.cost) & np.isfinite(b.cost) if a.cost.shape == b.cost.shape else np.zeros(0, dtype=bool)
                if both.any():
                    worst = max(worst, float(np.abs(a.cost[both] - b.cost[both]).max()))
            kept = [np.concatenate([f.best_id for f in r]) for r in (found, shared)]
            ops = [np.concatenate([f.best_op for f in r]) for r in (found, shared)]
            legs = {"corrections": corrections, "share_left": lambda: corrections(True),
                    "first_pass": lambda: rater.suspects(docs, context, precision="bf16", **common)}
            inner = {}
            for leg, fn in legs.items():
                fn()
                inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
            times = dict((leg, []) for leg in legs)
            for _ in range(repeats):
                for leg, fn in legs.items():
                    times[leg].append(timed(fn, sync, inner[leg]))
            before = whole.get("sets", {}).get(name, {})
            row = {"left": left, "ahead": args.ahead, "k": k, "deletions": deletions, "insertions": insertions,
                   "variants_per_suspect": k + 1 + int(deletions) + k * int(insertions), "streams": streams, "max_prob": max_prob,
                   "suspects_found": int(sum(len(f) for f in found)),
                   "suspects_shared": int(stats.get("shared", 0)),
                   "shared_share": stats.get("shared", 0) / max(1, stats.get("suspects", 0)),
                   "prefix_windows": int(stats.get("prefix_windows", 0)), "suffix_windows": int(stats.get("suffix_windows", 0)),
                   "unshared_windows": int(stats.get("unshared_windows", 0)),
                   "same_suspects_and_inf_pattern": same,
                   "max_abs_cost_shared_minus_unshared": worst,
                   # (what the file's run without the flag measured, where it had the same hypotheses)
                   "max_abs_cost_bf16_minus_split": before.get("max_abs_cost_bf16_minus_split") if (
                       whole.get("left"), whole.get("ahead"), whole.get("deletions"), whole.get("k")) == (
                       left, args.ahead, deletions, k) and not insertions else None,
                   "proposals_kept": int((kept[0] != -1).sum()), "proposals_kept_shared": int((kept[1] != -1).sum()),
                   "proposals_identical": bool(np.array_equal(kept[0], kept[1]) and np.array_equal(ops[0], ops[1])),
                   "proposals_differing": int(((kept[0] != kept[1]) | (ops[0] != ops[1])).sum())}
            for leg, ts in times.items():
                med = statistics.median(ts)
                row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                            "runs_per_timing": inner[leg]}
            row["speedup"] = row["corrections"]["seconds"] / row["share_left"]["seconds"]
            row["second_pass_speedup"] = ((row["corrections"]["seconds"] - row["first_pass"]["seconds"])
                                          / max(row["share_left"]["seconds"] - row["first_pass"]["seconds"], 1e-9))
            # faster only if the medians differ by more than both legs' spreads
            gap = (row["corrections"]["seconds"] - row["share_left"]["seconds"]) / row["corrections"]["seconds"]
            row["faster_beyond_spread"] = bool(gap > max(row["corrections"]["spread"], row["share_left"]["spread"]))
            whole.setdefault("sets", {}).setdefault(name, {})[key] = row
            print("%-16s left %3d  corrections %.4f s (spread %.2f)  share_left %.4f s (spread %.2f): %.2fx, second pass %.2fx  "
                  "%d of %d suspects shared, %d + %d + %d windows  |shared - unshared| <= %.3g bits  proposals identical %s (%d differ)"
                  % (name, left, row["corrections"]["seconds"], row["corrections"]["spread"], row["share_left"]["seconds"],
                     row["share_left"]["spread"], row["speedup"], row["second_pass_speedup"], row["suspects_shared"],
                     row["suspects_found"], row["prefix_windows"], row["suffix_windows"], row["unshared_windows"], worst,
                     row["proposals_identical"], row["proposals_differing"]), file=sys.stderr)
    emit(whole, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_corrections.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--suspect-share", type=float, default=0.02)
    ap.add_argument("--min-rank", type=int, default=1)
    ap.add_argument("--left", type=int, default=64)
    ap.add_argument("--ahead", type=int, default=8)
    ap.add_argument("--deletions", action="store_true")
    ap.add_argument("--insertions", action="store_true")
    ap.add_argument("--min-gain", type=float, default=1.0)
    ap.add_argument("--share-left", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_corrections: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk, windows
    sync = torch.cuda.synchronize
    repeats = max(5, args.repeats)
    k, left, ahead, deletions = args.k, args.left, args.ahead, int(args.deletions)
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)      # (as bench_rate_batch --bulk: peaked distributions)
    lm = rater.model
    context = [17]
    if args.share_left:
        return share_left_run(args, rater, context, repeats, sync)
    result = {"tool": "bench_corrections", "device": torch.cuda.get_device_name(0), "repeats": repeats, "k": k,
              "suspect_share": args.suspect_share, "min_rank": args.min_rank, "left": left, "ahead": ahead,
              "deletions": bool(deletions), "min_gain": args.min_gain,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "sets": {}}
    for insertions in ([0, 1] if args.insertions else [0]):
        R = k + 1 + deletions + k * insertions
        T = max(left + ahead + insertions, ratebulk.MIN_T)
        sets = {}
        for name, docs, streams in corpus_sets():
            chars = sum(len(d) for d in docs)
            chunk = max(1, streams // R)
            probs, _ = rater.rate_batch(docs, context, streams=streams, precision="bf16")
            max_prob = float(np.quantile(np.concatenate([p[1:] for p in probs]), args.suspect_share))
            del probs
            common = dict(k=k, streams=streams, max_prob=max_prob, min_rank=args.min_rank)
            held = {}

            def corrections(precision="bf16"):
                return rater.corrections(docs, context, left=left, ahead=ahead, deletions=bool(deletions), min_gain=args.min_gain,
                                         precision=precision, insertions=bool(insertions), **common)

            def host_windows(corpus, offsets, text_ctx, pos, alts, a):
                return ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos[a:a + chunk], alts[a:a + chunk], left, ahead,
                                                     deletions, T, insertions)

            def host_inputs(found):
                ids = [windows.encode(windows.normalize(t), rater.mapping[0]) for t in docs]
                offsets = np.concatenate([[0], np.cumsum([len(a) for a in ids])]).astype(np.int64)
                pos = np.concatenate([f.positions + offsets[i] for i, f in enumerate(found)])
                alts = np.concatenate([f.alt_ids for f in found])
                text_ctx = np.asarray([windows.clamp_context(context)] * len(docs), dtype=np.int32)
                return np.concatenate(ids).astype(np.int32), offsets, text_ctx, pos, alts

            def parent():
                found, bits = rater.suspects(docs, context, precision="bf16", **common)
                corpus, offsets, text_ctx, pos, alts = host_inputs(found)
                S = len(pos)
                cost, valid = [], []
                for a in range(0, S, chunk):
                    x, z, y, ok = host_windows(corpus, offsets, text_ctx, pos, alts, a)
                    lm.reset_states(len(x))
                    lm.rate_window_bulk(x, z, y, want_probs=False)
                    cost.append(lm.rate_bits_take(np.arange(len(x))))
                    valid.append(ok)
                if not S:
                    return found, bits, np.zeros((0, R)), np.zeros(0, dtype=np.int32), np.zeros(0)
                cost = torch.cat(cost).cpu().numpy().reshape(S, R)
                lm.rate_status_check()
                lm.reset_states(1)
                return (found, bits) + ratebulk.variant_pick_host(cost, np.concatenate(valid).reshape(S, R))

            def windows_device():
                pos, alts = held["sel"]
                for a in range(0, pos.numel(), chunk):
                    lm.variant_windows(held["corpus"], held["offsets"], held["text_ctx"], pos[a:a + chunk], alts[a:a + chunk], left,
                                       ahead, deletions, T, insertions=bool(insertions))

            def encode_host():
                host_inputs(held["found"])

            def first_pass():
                rater.suspects(docs, context, precision="bf16", **common)

            def windows_host():
                corpus, offsets, text_ctx, pos, alts = held["host"]
                for a in range(0, len(pos), chunk):
                    host_windows(corpus, offsets, text_ctx, pos, alts, a)

            # one run of each outside the timings: the two legs agree, and bf16 against split
            found, _ = corrections()
            count = sum(len(f) for f in found)
            p_cost = parent()[2]
            cost = np.concatenate([f.cost for f in found])
            identical = bool(cost.shape == p_cost.shape and np.array_equal(cost.view(np.uint64), p_cost.view(np.uint64)))
            split, _ = corrections("split")
            worst, compared = 0.0, 0
            for a, b in zip(found, split):
                _, ia, ib = np.intersect1d(a.positions, b.positions, return_indices=True)
                same = (a.alt_ids[ia] == b.alt_ids[ib]).all(axis=1)
                ca, cb = a.cost[ia][same], b.cost[ib][same]
                both = np.isfinite(ca) & np.isfinite(cb)
                if both.any():
                    worst = max(worst, float(np.abs(ca[both] - cb[both]).max()))
                    compared += int(both.sum())
            keep = {}
            _, arrays, _ = rater._rate_in_corpus_order(docs, [context] * len(docs), k, streams, "bf16", keep=keep)
            sel = lm.rate_select(*arrays, max_prob=max_prob, min_rank=args.min_rank)
            held.update(keep, sel=(sel[0], sel[3]), host=host_inputs(found), found=found)
            del arrays, sel
            legs = {"corrections": corrections, "parent": parent, "windows": windows_device, "windows_host": windows_host,
                    "encode_host": encode_host}
            if args.insertions:
                legs["first_pass"] = first_pass
            inner = {}
            for leg, fn in legs.items():
                fn()
                inner[leg] = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
            times = dict((leg, []) for leg in legs)
            for _ in range(repeats):
                for leg, fn in legs.items():
                    times[leg].append(timed(fn, sync, inner[leg]))
            held.clear()
            row = {"documents": len(docs), "chars": chars, "streams": streams, "max_prob": max_prob, "suspects_found": count,
                   "variants_per_suspect": R, "window_length": T, "suspects_per_chunk": chunk,
                   "proposals_kept": int(sum((f.best_id != -1).sum() for f in found)),
                   "costs_identical_to_parent": identical,
                   "max_abs_cost_bf16_minus_split": worst, "variants_compared_with_split": compared,
                   "bytes_from_device_second_pass": count * 12 * R,
                   "bytes_to_device_second_pass_parent": count * R * T * 4 * (2 + len(context))}
            for leg, ts in times.items():
                med = statistics.median(ts)
                row[leg] = {"chars_per_s": chars / med, "seconds": med, "spread": (max(ts) - min(ts)) / med,
                            "runs_per_timing": inner[leg]}
            row["speedup"] = row["corrections"]["chars_per_s"] / row["parent"]["chars_per_s"]
            row["windows_share"] = row["windows"]["seconds"] / row["corrections"]["seconds"]
            row["windows_host_share_of_parent"] = row["windows_host"]["seconds"] / row["parent"]["seconds"]
            row["encode_host_share_of_parent"] = row["encode_host"]["seconds"] / row["parent"]["seconds"]
            if args.insertions:
                row["second_pass_seconds"] = row["corrections"]["seconds"] - row["first_pass"]["seconds"]
            sets[name] = row
            print("%-16s corrections %10.0f  parent %10.0f chars/s (%.2fx)  %d suspects  windows %.1f %% (host: %.1f %% of parent)  "
                  "encode %.1f %% of parent  identical %s  |bf16 - split| <= %.3g over %d" % (
                      name, row["corrections"]["chars_per_s"], row["parent"]["chars_per_s"], row["speedup"], count,
                      100.0 * row["windows_share"], 100.0 * row["windows_host_share_of_parent"],
                      100.0 * row["encode_host_share_of_parent"], identical, worst, compared),
                  file=sys.stderr)
        if not args.insertions:
            result["sets"] = sets
            continue
        # both measurements of a set side by side, and what the insertion rows cost the second pass
        for name, row in sets.items():
            one = result["sets"].setdefault(name, {})
            one["with_insertions" if insertions else "without_insertions"] = row
            if insertions:
                before = one["without_insertions"]
                one["rows_ratio"] = row["variants_per_suspect"] / before["variants_per_suspect"]
                one["second_pass_seconds_ratio"] = row["second_pass_seconds"] / before["second_pass_seconds"]
                one["corrections_seconds_ratio"] = row["corrections"]["seconds"] / before["corrections"]["seconds"]
    if args.insertions:
        # under a key of its own: the file's other content (the run without the flag) stays as it is
        whole = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                whole = json.load(f)
        whole["insertions"] = result
        result = whole
    emit(result, args.out)


if __name__ == "__main__":
    main()
