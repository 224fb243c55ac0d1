#!/usr/bin/env python3
"""Confusion tables: OCR output held against its ground truth and the differences counted on the device (kl_align_pairs ->
kl_confusion_counts, `Rater.confusions`) against what a caller would write without it -- `Rater.align` and then the statement
of the same commit (`ratebulk.confusion_counts_host`: Python over every span and every position).  The parent commit has no
such step at all.

  python tools/bench_confusions.py [--out profiles/confusions.json] [--repeats 5] [--host-repeats 3] [--host-documents 64]
                                   [--host-lines 5000] [--noise 0.005]

The corpora are bench_witnesses.py's (1024 documents of 2048 characters at max_dist 128, 20 000 lines of 30 to 90 characters at
max_dist 32); they are the TRUTH.  The OCR is made from it by a planted table of 12 confusions -- a character of the truth read
as one or two other characters, at rates of 5 to 30 % of its occurrences -- plus uniform noise: --noise of the characters
substituted, a fifth as many dropped and as many inserted (seed 2029).  Legs:
  "kernels"     `HipLM.confusion_counts` alone on inputs that lie on the device (the eight launches of kl_confusion_counts),
  "align"       `HipLM.align_pairs` alone, the launch in front of them,
  "confusions"  `Rater.confusions` on the whole set: normalising, encoding, one upload per side, both calls, one download,
  "host"        `Rater.align` plus `confusion_counts_host` on the first --host-documents / --host-lines pairs -- Python does
                not get through more in a benchmark's time --, "confusions_subset" the device on the same pairs, all outputs
                asserted identical; "host_scaled" is the host's time times pairs / host pairs, an extrapolation and said so.
Whether the planted rules head the table is checked and reported ("planted_lead": the first 12 sources of
`rules(min_count=2, per_source=1)` are the planted ones with the planted readings), with the character error rate.
Host clock around work that ends in a device synchronise; every leg is warmed up once; the device legs take the median of
--repeats (at least 5) timings, each of at least --min-seconds, the host leg the median of --host-repeats single runs; the
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

from tools.bench_rate_batch import ALPHABET, MODELS, emit, make_rater, timed      # noqa: E402
from tools.bench_witnesses import summary, witness_of      # noqa: E402
from tools.bench_words import corpus_sets      # noqa: E402


def planted_table():
    """[(what the OCR writes, what the truth holds, the share of the truth's occurrences read so)]: eight confusions of one
    character for one, four of two for one; no character is in two rules"""
    rules = []
    for k in range(12):
        truth = ALPHABET[40 + k]
        read = ALPHABET[70 + 2 * k] if k < 8 else ALPHABET[70 + 2 * k] + ALPHABET[71 + 2 * k]
        rules.append((read, truth, 0.05 + 0.25 * k / 11))
    return rules


def ocr_of(rng, text, rules, noise):
    """the truth as the planted OCR reads it: uniform noise first, then every rule at its rate on the characters left alone"""
    noisy = witness_of(rng, text, noise, noise / 5, noise / 5)
    chars = np.array(list(noisy), dtype=object)
    lot = rng.random(len(chars))
    for read, truth, rate in rules:
        chars[(chars == truth) & (lot < rate)] = read
    return "".join(chars.tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confusions.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--host-documents", type=int, default=64)
    ap.add_argument("--host-lines", type=int, default=5000)
    ap.add_argument("--noise", type=float, default=0.005)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_confusions: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk
    sync = torch.cuda.synchronize
    repeats, host_repeats = max(5, args.repeats), max(1, args.host_repeats)
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    rules = planted_table()
    result = {"tool": "bench_confusions", "device": torch.cuda.get_device_name(0), "repeats": repeats, "host_repeats": host_repeats,
              "noise": args.noise, "planted": [[read, truth, rate] for read, truth, rate in rules], "sets": {}}
    rng = np.random.default_rng(2029)
    codes = lambda strings: (np.frombuffer("".join(strings).encode("utf-32-le"), dtype=np.int32).copy(),
                             np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64))
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

    for number, (name, truths, _) in enumerate(corpus_sets(0.16)):
        max_dist = 128 if number == 0 else 32
        n_host = args.host_documents if number == 0 else args.host_lines
        texts = [ocr_of(rng, t, rules, args.noise) for t in truths]
        print("%s: %d pairs, max_dist %d" % (name, len(texts), max_dist), file=sys.stderr)
        max_len = max(len(t) for t in texts + truths)
        on_device = [up(x) for x in codes(texts) + codes(truths)]
        spans = lm.align_pairs(*on_device, max_len, max_dist, 0)
        sub = codes(texts[:n_host]) + codes(truths[:n_host])
        sub_len = max(len(t) for t in texts[:n_host] + truths[:n_host])

        def host_leg():
            found = rater.align(texts[:n_host], truths[:n_host], max_dist=max_dist)
            dist = np.array([one.dist for one in found], dtype=np.int32)
            n_spans = np.array([len(one) for one in found], dtype=np.int32)
            padded = np.full((n_host, max_dist, 4), -1, dtype=np.int32)
            for p, one in enumerate(found):
                padded[p, :len(one)] = one.spans
            return ratebulk.confusion_counts_host(*sub, dist, n_spans, padded, 4, 65536)

        want = host_leg()
        sub_d = [up(x) for x in sub]
        got = lm.confusion_counts(*sub_d, *lm.align_pairs(*sub_d, sub_len, max_dist, 0), 4, 65536)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), "kernels and statement disagree"
        found = rater.confusions(texts, truths, max_dist=max_dist)
        lead = found.rules(min_count=2, per_source=1)[:len(rules)]
        by_source = dict((found.sources[i], i) for i in reversed(range(len(found))) if (found.sources[i], found.targets[i]) in
                         set((read, truth) for read, truth, _ in rules))
        ts = []
        for _ in range(host_repeats):
            t0 = time.perf_counter()
            host_leg()
            ts.append(time.perf_counter() - t0)
        row = {"pairs": len(texts), "chars": sum(len(t) for t in truths), "max_dist": max_dist, "host_pairs": n_host,
               "span_slots": len(texts) * max_dist, "records": len(found), "spans": found.spans, "skipped": found.skipped,
               "cer": found.cer, "edits": found.edits,
               "workspace_bytes": int(lm.lib.kl_confusion_counts_workspace_bytes(len(texts), max_dist, on_device[0].numel())),
               "planted_lead": sorted((s, r[0]) for s, r in lead) == sorted((read, truth) for read, truth, _ in rules),
               "planted_found": [[read, truth, rate, int(found.count[by_source[read]]), int(found.occ[by_source[read]])]
                                 for read, truth, rate in rules if read in by_source],
               "host": summary(ts)}
        row.update(device_times({"kernels": lambda: lm.confusion_counts(*on_device, *spans, 4, 65536),
                                 "align": lambda: lm.align_pairs(*on_device, max_len, max_dist, 0),
                                 "confusions": lambda: rater.confusions(texts, truths, max_dist=max_dist),
                                 "confusions_subset": lambda: rater.confusions(texts[:n_host], truths[:n_host], max_dist=max_dist)}))
        row["host_scaled"] = {"seconds": row["host"]["seconds"] * len(texts) / n_host, "extrapolated_from_pairs": n_host}
        row["speedup_on_subset"] = row["host"]["seconds"] / row["confusions_subset"]["seconds"]
        result["sets"][name] = row
        print("%-16s kernels %.4f s (align %.4f s), Rater.confusions %.4f s; %d pairs: device %.4f s, align + Python %.2f s (%.0fx; "
              "scaled to all pairs %.1f s); %d records of %d spans, cer %.4f, planted rules lead: %s"
              % (name, row["kernels"]["seconds"], row["align"]["seconds"], row["confusions"]["seconds"], n_host,
                 row["confusions_subset"]["seconds"], row["host"]["seconds"], row["speedup_on_subset"], row["host_scaled"]["seconds"],
                 row["records"], row["spans"], row["cer"], row["planted_lead"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
