#!/usr/bin/env python3
"""Witness consensus: `Rater.consensus` -- the differing spans of all witnesses of a text clustered on the device
(kl_align_pairs -> kl_witness_clusters -> kl_witness_pool -> the rating of `rescore`) -- against the chains a caller has without
it, in the same run.  The parent commit has no clustering across witnesses at all.

  python tools/bench_consensus.py [--out profiles/consensus.json] [--repeats 5] [--host-repeats 3] [--documents 1024]
                                  [--lines 20000]

The corpora are bench_witnesses.py's (cfg2 size: depth 2, width 512, length 256; 1024 documents of 2048 characters at max_dist
128 and 20 000 lines of 30 to 90 characters at max_dist 32; a witness is its text with 2 % of the characters substituted, 0.5 %
dropped and 0.5 % inserted; seed 2028), join 1.  Legs:
  (a) ONE witness per text: "consensus" = `consensus(vote_bits=0)` alternated with "merge" = `merge_witnesses` (align -> the
      `Alignment`s -> `witness_edits` in Python -> rescore); spans, candidates, best, gain and the counts by reason are asserted
      identical, the costs too (both calls without costs are not compared: `merge_witnesses` always fetches them).
  (b) THREE witnesses per text: "consensus" alternated with "host_chain" = `align` of all pairs -> the `Alignment`s ->
      `ratebulk.witness_clusters_host` (Python over every span) -> `rescore` on the edits it amounts to; the same spans,
      candidates and choices asserted.  "host_clusters" is the statement's share of the chain, by a clock around it.
  (c) "clusters": `HipLM.witness_clusters` + `HipLM.witness_pool` alone on the three-witness inputs as they lie on the device,
      by device events around the launches; "align" the launch in front of them, likewise.
Host clock around work that ends in a device synchronise for (a) and (b), one run per timing, the two alternated; every leg is
warmed up once; the median of --repeats (at least 5) timings -- the host chain: of --host-repeats --, the spread is
(max - min) / median.  One JSON line on stdout, also written to --out.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--documents", type=int, default=1024)
    ap.add_argument("--lines", type=int, default=20000)
    ap.add_argument("--substituted", type=float, default=0.02)
    ap.add_argument("--dropped", type=float, default=0.005)
    ap.add_argument("--inserted", type=float, default=0.005)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_consensus: no GPU visible (the rater has no CPU path)")
    from ocrd_keraslm_amd.lib import ratebulk, windows
    sync = torch.cuda.synchronize
    repeats, host_repeats = max(5, args.repeats), max(1, args.host_repeats)
    rater = make_rater(**MODELS["cfg2"])
    rater.model.init_weights(seed=3, emb_std=0.3)
    lm = rater.model
    context = [17]
    result = {"tool": "bench_consensus", "device": torch.cuda.get_device_name(0), "repeats": repeats, "host_repeats": host_repeats,
              "substituted": args.substituted, "dropped": args.dropped, "inserted": args.inserted, "join": 1,
              "model": dict(MODELS["cfg2"], voc_size=len(ALPHABET) + 1), "sets": {}}
    rng = np.random.default_rng(2028)
    codes = lambda strings: (np.frombuffer("".join(strings).encode("utf-32-le"), dtype=np.int32).copy(),
                             np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)

    def alternated(legs, counts):
        """every leg warmed up once, then one run per timing, the legs in turn: counts[leg] timings each"""
        for fn in legs.values():
            fn()
        times = dict((leg, []) for leg in legs)
        for turn in range(max(counts.values())):
            for leg, fn in legs.items():
                if turn < counts[leg]:
                    times[leg].append(timed(fn, sync, 1))
        return dict((leg, summary(ts)) for leg, ts in times.items())

    def by_events(fn):
        """the median of `repeats` timings of at least --min-seconds each, by device events around the launches"""
        fn()
        inner = max(1, int(np.ceil(args.min_seconds / max(timed(fn, sync, 1), 1e-6))))
        ts = []
        for _ in range(repeats):
            first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            first.record()
            for _ in range(inner):
                fn()
            last.record()
            sync()
            ts.append(first.elapsed_time(last) / 1000.0 / inner)
        return dict(summary(ts), runs_per_timing=inner)

    def same(found, want, costs):
        for one, ref in zip(found, want):
            assert one.candidates == ref.candidates, "candidates differ"
            for name in ("starts", "ends", "first", "best", "gain") + (("cost0", "cost") if costs else ()):
                assert np.array_equal(getattr(one, name), getattr(ref, name)), name + " differs"

    for number, (name, texts, streams) in enumerate(corpus_sets(0.16)):
        max_dist = 128 if number == 0 else 32
        texts = texts[:args.documents if number == 0 else args.lines]
        n = len(texts)
        three = [[witness_of(rng, t, args.substituted, args.dropped, args.inserted) for _ in range(3)] for t in texts]
        one = [readings[:1] for readings in three]
        rating = dict(max_dist=max_dist, join=1, streams=streams, precision="bf16")
        print("%s: %d texts, max_dist %d" % (name, n, max_dist), file=sys.stderr)

        # ---- (a) one witness: against merge_witnesses
        found, dists, skipped = rater.consensus(texts, one, context, vote_bits=0.0, **rating)
        alignments, rescored, merged_skipped = rater.merge_witnesses(texts, one, context, **rating)
        same(found, rescored, costs=True)
        assert skipped == merged_skipped and [d.tolist() for d in dists] == [[al.dist for al in per] for per in alignments]
        row = {"texts": n, "chars": sum(len(t) for t in texts), "max_dist": max_dist, "streams": streams,
               "one_witness": dict(alternated({"consensus": lambda: rater.consensus(texts, one, context, vote_bits=0.0, **rating),
                                               "merge": lambda: rater.merge_witnesses(texts, one, context, **rating)},
                                              dict(consensus=repeats, merge=repeats)),
                                   spans=sum(len(f) for f in found), candidates=sum(len(f.candidates) for f in found), skipped=skipped,
                                   proposals=sum(int((f.best >= 0).sum()) for f in found))}
        row["one_witness"]["speedup"] = row["one_witness"]["merge"]["seconds"] / row["one_witness"]["consensus"]["seconds"]

        # ---- (b) three witnesses: against the host chain
        pairs = [(i, w) for i in range(n) for w in range(3)]
        normal = [windows.normalize(t) for t in texts]
        pair_first = 3 * np.arange(n + 1, dtype=np.int64)
        text_off = np.concatenate([[0], np.cumsum([len(t) for t in normal])]).astype(np.int64)
        b_strings = [windows.normalize(three[i][w]) for i, w in pairs]
        b_side = codes(b_strings)
        joined = "".join(b_strings)
        clock = []

        def host_chain():
            flat = rater.align([texts[i] for i, _ in pairs], [three[i][w] for i, w in pairs], max_dist=max_dist, join=1)
            t0 = time.perf_counter()
            spans = np.full((len(flat), max_dist, 4), -1, dtype=np.int32)
            for p, al in enumerate(flat):
                spans[p, :len(al)] = al.spans
            out = ratebulk.witness_clusters_host(*b_side, np.array([al.dist for al in flat], dtype=np.int32),
                                                 np.array([len(al) for al in flat], dtype=np.int32), spans, pair_first, text_off, 1)
            S = int(out[7][0])
            size = np.diff(out[5])
            edits = [(int(out[0][s]), int(out[1][s] - text_off[out[0][s]]), int(out[1][s] - text_off[out[0][s]] + out[2][s]),
                      [joined[out[4][c]:out[4][c] + size[c]] for c in range(int(out[3][s]), int(out[3][s + 1]))]) for s in range(S)]
            clock.append(time.perf_counter() - t0)
            return rater.rescore(texts, edits, context, streams=streams, precision="bf16"), out

        found, dists, skipped = rater.consensus(texts, three, context, **rating)
        want, out = host_chain()
        same(found, want, costs=True)
        assert skipped == dict(different=int(out[7][4]), first=int(out[7][5]), long=int(out[7][6]))
        del clock[:]
        row["three_witnesses"] = dict(alternated({"consensus": lambda: rater.consensus(texts, three, context, **rating),
                                                  "host_chain": host_chain}, dict(consensus=repeats, host_chain=host_repeats)),
                                      spans=int(out[7][0]), candidates=int(out[7][1]), skipped=skipped,
                                      several_readings=int((np.diff(out[3][:int(out[7][0]) + 1]) >= 2).sum()),
                                      proposals=sum(int((f.best >= 0).sum()) for f in found))
        row["three_witnesses"]["host_clusters"] = summary(clock[1:])      # (the first is the warm-up's)
        row["three_witnesses"]["speedup"] = (row["three_witnesses"]["host_chain"]["seconds"]
                                             / row["three_witnesses"]["consensus"]["seconds"])

        # ---- (c) the launches alone
        a_side = codes([normal[i] for i, _ in pairs])
        max_len = max(len(t) for t in normal + b_strings)
        on_device = [up(x) for x in a_side + b_side]
        firsts = [up(pair_first), up(text_off)]
        b_ids = up(windows.encode(joined, rater.mapping[0]).astype(np.int32))
        aligned = lm.align_pairs(*on_device, max_len, max_dist, 1)
        C, n_pool = int(out[7][1]), int(out[7][2])

        def clusters():
            got = lm.witness_clusters(on_device[2], on_device[3], *aligned, *firsts, 1)
            return got, lm.witness_pool(b_ids, got[4], got[5], C, n_pool)

        got, pool = clusters()
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, out)), "kernels and statement disagree"
        row["launches"] = {"pairs": len(pairs), "span_slots": len(pairs) * max_dist, "clusters": by_events(clusters),
                           "align": by_events(lambda: lm.align_pairs(*on_device, max_len, max_dist, 1)),
                           "workspace_bytes": int(lm.lib.kl_witness_clusters_workspace_bytes(len(pairs), max_dist, n))}
        result["sets"][name] = row
        print("%-16s one witness: consensus %.3f s, merge_witnesses %.3f s (%.2fx); three: consensus %.3f s, host chain %.3f s "
              "(%.2fx; its clustering in Python %.3f s); launches: clusters %.5f s, align %.5f s"
              % (name, row["one_witness"]["consensus"]["seconds"], row["one_witness"]["merge"]["seconds"], row["one_witness"]["speedup"],
                 row["three_witnesses"]["consensus"]["seconds"], row["three_witnesses"]["host_chain"]["seconds"],
                 row["three_witnesses"]["speedup"], row["three_witnesses"]["host_clusters"]["seconds"],
                 row["launches"]["clusters"]["seconds"], row["launches"]["align"]["seconds"]), file=sys.stderr)
    emit(result, args.out)


if __name__ == "__main__":
    main()
