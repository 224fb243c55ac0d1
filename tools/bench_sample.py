#!/usr/bin/env python3
"""`Rater.sample`: the chains drawn on the device (kl_sample_pick after every step, all characters enqueued without a wait)
against the same chains drawn on the host (step_slots, the probabilities fetched, gensample.pick_host: one wait per character).

  python tools/bench_sample.py [--out profiles/sample_generate.json] [--repeats 5] [--length 64] [--variants 256]

Draws `--variants` continuations of `--length` characters after a fixed 12-character prefix at temperature 0.8, top_k 40, on two
models with a synthetic vocabulary of 256 -- cfg2 size (depth 2, width 512) and the published size (depth 2, width 128).  Both
legs run in the same process on the same model, with the same seed and so the same uniform numbers, alternated host, device,
host, device, ... `--repeats` times each after one warm-up of each; host clock around `--calls` whole calls (each ends with the
strings on the host).  Reported per model: the median ms per character position (all chains advance one character) of both
legs, their spreads (max - min) / median, the ratio host / device, whether every device run beat every host run, and how many
of the strings are the same (the host leg sums the weights in float64, the kernel in float32: a pick whose u * S falls
within rounding of a running sum may differ, and the chain after it).  One JSON line on stdout, also written to --out.

Needs the GPU: there is no fallback.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_generate import ALPHABET, MODELS, PREFIX, make_rater      # noqa: E402  (the same models)

DRAW = dict(temperature=0.8, top_k=40, floor=0.0)


def sample_on_host(rater, prefix, length, context, variants, seed, temperature, top_k, floor):
    """the chains of `Rater.sample` with every character drawn on the host: per character one step_slots on the chains' pool
    slots, one fetch of [variants][V] (the wait), gensample.pick_host, one upload of the picks"""
    from ocrd_keraslm_amd.lib import gensample, windows
    lm, pool = rater.model, rater._state_pool()
    c_i, i_c = rater.mapping
    valid = np.zeros(rater.voc_size, dtype=np.uint8)
    valid[[i for i in i_c if 0 <= i < rater.voc_size]] = 1
    state = None
    for char in prefix[:-1]:
        _, states = rater._predict_refs([char], [state], context)
        state = states[0]
    slots = pool.take_slots(2 * variants)
    try:
        sets = (lm.to_device_i32(slots[:variants]), lm.to_device_i32(slots[variants:]))
        ctx_d = lm.to_device_i32(np.tile(np.asarray(windows.clamp_context(context), dtype=np.int32), (variants, 1)))
        idx = np.full(variants, c_i.get(prefix[-1], 0), dtype=np.int32)
        slot_in = lm.to_device_i32(np.full(variants, state.slot if state is not None else pool.zero_slot, dtype=np.int32))
        log = np.zeros((length, variants), dtype=np.int32)
        for s in range(length):
            probs = lm.step_slots(lm.to_device_i32(idx), ctx_d, slot_in, sets[s & 1]).cpu().numpy()
            log[s] = idx = gensample.pick_host(probs, gensample.philox_uniform(seed, s, variants), valid, temperature, top_k, floor)
            slot_in = sets[s & 1]
    finally:
        pool.release_slots(slots)
    return gensample.spell((log,), i_c, prefix[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_generate.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--length", type=int, default=64)
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--calls", type=int, default=4, help="calls per timed repetition")
    ap.add_argument("--models", default="cfg2,published")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sample: no GPU visible (the rater has no CPU path)")
    result = {"tool": "bench_sample", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls_per_repeat": args.calls,
              "length": args.length, "variants": args.variants, "voc_size": len(ALPHABET) + 2, "prefix_chars": len(PREFIX),
              "draw": DRAW, "models": {}}
    for model in args.models.split(","):
        rater = make_rater(**MODELS[model])
        ctx = [17]

        def leg(device, seed=7):
            if device:
                return rater.sample(PREFIX, args.length, ctx, args.variants, seed=seed, **DRAW)
            return sample_on_host(rater, PREFIX, args.length, ctx, args.variants, seed, **DRAW)

        texts = {device: leg(device) for device in (False, True)}      # warm-up: workspaces, the pool, code objects
        times = {False: [], True: []}
        for _ in range(args.repeats):
            for device in (False, True):
                gc.collect()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    out = leg(device)
                times[device].append((time.perf_counter() - t0) * 1e3 / (args.length * args.calls))
                assert out == texts[device]
        host_ms, dev_ms = statistics.median(times[False]), statistics.median(times[True])
        result["models"][model] = {
            "depth": rater.depth, "width": rater.width,
            "host_draw_ms_per_position": host_ms, "device_draw_ms_per_position": dev_ms, "ratio": host_ms / dev_ms,
            "host_draw_spread": (max(times[False]) - min(times[False])) / host_ms,
            "device_draw_spread": (max(times[True]) - min(times[True])) / dev_ms,
            "device_draw_faster": bool(max(times[True]) < min(times[False])),
            "same_strings": sum(a == b for a, b in zip(texts[False], texts[True])), "distinct_strings": len(set(texts[True])),
        }
    line = json.dumps(result, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
