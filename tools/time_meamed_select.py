"""Times the mean around the median by rank selection (method="select") against the
trimmed mean by selection of the same slab (the existing kernel with the same tile, one descent
where this one has three: the yardstick) and, at 128 clients, against the sorting kernel.

Shapes: 128 x 4 Mi and 1024 x 4 Mi float32 as slabs; 1024 clients x EMNIST-CNN (8 leaves,
1,206,590 float32 params; configs[1] of BASELINE.json) as a slab and as separate pytrees; and one
Bulyan round (Gram pass, host selection, second stage by selection) over 512 such clients, f = 32.
Legs on each slab, with the keep count equal to the trimmed mean's K - 2t so that the sums match:
  (a) mean_around_median(K - 2t, method="select")
  (b) trimmed_mean(t, method="select")
  (c) mean_around_median(K - 2t, method="sort"), at 128 clients only

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each and (a) as a multiple of
(b) and (c); the summary record is appended to --out as well.

usage (MI355X): python tools/time_meamed_select.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import kernels, tree_util as tu  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}
TRIM = 0.1


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
    ap.add_argument("--small", action="store_true", help="64 Ki columns, a small model (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meamed_select_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    model = {"w": (1000,), "b": (7,)} if args.small else EMNIST
    template = tmap(lambda s: np.zeros(s, np.float32), model)

    runs, reps, res, ratios = {}, {}, {"trim": TRIM, "columns": Pb}, []

    def slab_legs(name, slab, n):
        K = slab.num_clients
        t = kernels.trim_count(TRIM, K, select=True)
        outs = [torch.empty(slab.num_params, dtype=torch.float32, device=dev) for _ in range(3)]
        runs[name + "_a"] = lambda: slab.mean_around_median(K - 2 * t, out=outs[0], method="select")
        runs[name + "_b"] = lambda: slab.trimmed_mean(t, out=outs[1], method="select")
        ratios.append((name + "_a", name + "_b"))
        if K <= kernels.TRIM_MAX_CLIENTS:
            runs[name + "_c"] = lambda: slab.mean_around_median(K - 2 * t, out=outs[2], method="sort")
            ratios.append((name + "_a", name + "_c"))
        for leg in "abc":
            reps[name + "_" + leg] = n
        res[name] = [K, slab.num_params, K - 2 * t]

    slabs = {}  # kept alive: the legs hold them
    for K in (128, 1024):
        slabs[K] = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=K)
        slab_legs(f"big{K}", slabs[K], 3)
    es = fedjax_amd.ClientDeltaSlab(template, 1024, device=dev).fill_synthetic(seed=2)
    slab_legs("emnist1024_slab", es, 5)
    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(1024)]
    t = kernels.trim_count(TRIM, 1024, select=True)
    runs["emnist1024_tree_a"] = lambda: tu.tree_mean_around_median(clients, 1024 - 2 * t, method="select")
    runs["emnist1024_tree_b"] = lambda: tu.tree_trimmed_mean(clients, t, method="select")
    ratios.append(("emnist1024_tree_a", "emnist1024_tree_b"))
    bs = fedjax_amd.ClientDeltaSlab(template, 512, device=dev).fill_synthetic(seed=3)
    runs["bulyan512_slab"] = lambda: bs.bulyan(32, method="select")
    reps.update(emnist1024_tree_a=5, emnist1024_tree_b=5, bulyan512_slab=3)
    res["bulyan512_slab"] = [512, bs.num_params, 32]
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every shape
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
    summary = dict(res, summary=True, tool="tools/time_meamed_select.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for a, b in ratios:
        summary[f"{a}_over_{b[-1]}"] = round(med[a] / med[b], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
