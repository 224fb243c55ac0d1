#!/usr/bin/env python3
"""`Rater.generate`: the host path (one engine call and one wait per character, the beam kept in Python) against the device
beam (`device_beam=True`: kl_beam_expand chooses and prunes on the GPU, all characters enqueued without a wait).

  python tools/bench_generate.py [--out profiles/generate_device_beam.json] [--repeats 5] [--length 64]

Generates `--length` characters with variants=1 after a fixed 12-character prefix, on two models with a synthetic vocabulary of
256 -- cfg2 size (depth 2, width 512) and the published size (depth 2, width 128).  Both legs run in the same process on the
same model, alternated host, device, host, device, ... `--repeats` times each after one warm-up of each; host clock around
`--calls` whole `generate` calls (each ends with the strings on the host).  Reported per model: the median ms per generated character of
both legs, their spreads (max - min) / median, the ratio host / device, whether every device-beam run beat every host run
and whether both legs returned the same string.  One JSON line on stdout, also written to --out.  The host leg is `generate` as it
was before the device beam existed: the comparison inside one run is the acceptance.

Needs the GPU: there is no fallback.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALPHABET = [chr(c) for c in range(33, 127)] + [chr(c) for c in range(0xA1, 0xA1 + 160)]      # 254 characters + the space: V = 256
MODELS = {"cfg2": dict(depth=2, width=512), "published": dict(depth=2, width=128)}
PREFIX = "The quick br"


def make_rater(depth, width):
    from ocrd_keraslm_amd.lib import Rater
    chars = [" "] + ALPHABET
    r = Rater()
    r.width, r.depth, r.length = width, depth, 256
    r.stateful, r.incremental = False, True
    r.mapping = (dict((c, i) for i, c in enumerate(chars, 1)), dict((i, c) for i, c in enumerate(chars, 1)))
    r.voc_size = len(chars) + 1
    r.seed = 3
    r.configure()
    r.model.init_weights(seed=3, emb_std=0.5)      # (the default 0.001 gives a uniform model: every hypothesis would tie)
    r.model.prepare(3)
    r.status = 2
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_device_beam.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--length", type=int, default=64)
    ap.add_argument("--calls", type=int, default=4, help="generate calls per timed repetition")
    ap.add_argument("--models", default="cfg2,published")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_generate: no GPU visible (the rater has no CPU path)")
    result = {"tool": "bench_generate", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls_per_repeat": args.calls, "length": args.length,
              "variants": 1, "voc_size": len(ALPHABET) + 2, "prefix_chars": len(PREFIX), "models": {}}
    for model in args.models.split(","):
        rater = make_rater(**MODELS[model])
        ctx = [17]
        texts = {}
        for beam in (False, True):      # warm-up: workspaces, the pool, code objects
            texts[beam] = rater.generate(PREFIX, args.length, ctx, 1, device_beam=beam)
        times = {False: [], True: []}
        for _ in range(args.repeats):
            for beam in (False, True):
                gc.collect()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    out = rater.generate(PREFIX, args.length, ctx, 1, device_beam=beam)
                times[beam].append((time.perf_counter() - t0) * 1e3 / (args.length * args.calls))
                assert out == texts[beam]
        host_ms, dev_ms = statistics.median(times[False]), statistics.median(times[True])
        result["models"][model] = {
            "depth": rater.depth, "width": rater.width,
            "host_ms_per_char": host_ms, "device_beam_ms_per_char": dev_ms, "ratio": host_ms / dev_ms,
            "host_spread": (max(times[False]) - min(times[False])) / host_ms,
            "device_beam_spread": (max(times[True]) - min(times[True])) / dev_ms,
            "device_beam_faster": bool(max(times[True]) < min(times[False])),
            "same_string": texts[False] == texts[True],
        }
    line = json.dumps(result, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
