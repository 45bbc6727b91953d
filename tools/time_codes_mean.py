"""Times the mean folded from 8-bit level codes (CodeSlab.mean) against the float32
fold of the same K x P and against the fused uniform quantizer round, and the encoder alone.

Shapes: 1024 clients x 4 Mi, and 1024 clients x EMNIST-CNN (8 leaves, 1,206,590 params; configs[1]
of BASELINE.json). Legs of every shape:
  (c) CodeSlab.mean: fjcomp_codes_fold, K x P bytes read
  (m) ClientDeltaSlab.mean of the float32 slab the codes were encoded from: 4 K x P bytes read
  (q) uniform_stochastic_quantizer(num_levels).apply over the float32 client views: the fused round
  (e) CodeSlab.encode_from: the statistics pass and fjcomp_encode_uniform

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each, the ratios and the achieved
byte rates of (c) and (m); the summary record is appended to --out as well.

usage (MI355X): python tools/time_codes_mean.py [--passes 7] [--small] [--levels 16] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fedjax_amd  # noqa: E402
from fedjax_amd import kernels, random  # noqa: E402
from fedjax_amd.aggregators import compression  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}


def tmap(f, t):
    return {k: tmap(f, v) for k, v in t.items()} if isinstance(t, dict) else f(t)


def per_call_ms(fn, reps):
    s = torch.cuda.current_stream()
    e0, e1 = kernels.Event(), kernels.Event()
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--small", action="store_true", help="64 clients, a 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codes_mean_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 64 if args.small else 1024
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    key = random.PRNGKey(0)
    runs, reps, res = {}, {}, {"num_levels": args.levels}

    def legs(name, template, n):
        f32 = fedjax_amd.ClientDeltaSlab(template, K, device=dev).fill_synthetic(seed=len(runs))
        codes = fedjax_amd.CodeSlab(template, K, args.levels, device=dev).encode_from(f32, key)
        ones = [1.0] * K
        outs = [torch.empty(f32.num_params, dtype=torch.float32, device=dev) for _ in range(2)]
        agg = compression.uniform_stochastic_quantizer(args.levels, key)
        clients = [(k, f32.client(k), 1.0) for k in range(K)]
        state = agg.init()
        runs[name + "_c"] = lambda: codes.mean(ones, out=outs[0])
        runs[name + "_m"] = lambda: f32.mean(ones, out=outs[1])
        runs[name + "_q"] = lambda: agg.apply(clients, state)
        runs[name + "_e"] = lambda: codes.encode_from(f32, key)
        for leg, r in zip("cmqe", (n, n, 2, 2)):
            reps[name + "_" + leg] = r
        res[name] = [K, f32.num_params]

    legs("big", {"w": np.zeros(Pb, np.float32)}, 5)
    legs("emnist", tmap(lambda s: np.zeros(s, np.float32), EMNIST), 10)
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every leg of every shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for p in range(args.passes):
        row = {"pass": p}
        for name, fn in runs.items():
            ms = per_call_ms(fn, reps[name])
            times[name].append(ms)
            row[name + "_ms"] = round(ms, 4)
        print(json.dumps(row), flush=True)
    med = {k: float(np.median(v)) for k, v in times.items()}
    summary = dict(res, summary=True, tool="tools/time_codes_mean.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("big", "emnist"):
        for other in "mq":
            summary[f"{shape}_c_over_{other}"] = round(med[f"{shape}_c"] / med[f"{shape}_{other}"], 4)
        kp = res[shape][0] * res[shape][1]
        summary[f"{shape}_c_GBps"] = round(kp / med[f"{shape}_c"] / 1e6, 1)      # code bytes read per second
        summary[f"{shape}_m_GBps"] = round(4 * kp / med[f"{shape}_m"] / 1e6, 1)  # the float32 fold's HBM rate
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
