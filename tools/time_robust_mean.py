"""Times the coordinate-wise trimmed mean and median against the plain mean of the same bytes
(the floor: one read) and against the route a caller composes from torch ops today.

Shapes: 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json) as a slab and as separate pytrees (every (client, leaf) its own device tensor),
and 128 clients x 4 Mi float32 as a slab. Legs on each:
  (a) trimmed_mean(0.1)
  (b) median()
  (c) the mean with unit weights over the same deltas, same build: the floor
  (d) torch: torch.sort(rows, dim=0), a slice, .sum(0), a multiply (per leaf, after a
      torch.stack, for the pytrees): what users do today; a K x P temporary and several passes

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each, and (a), (b) as multiples
of (c) and of (d); the summary record is appended to --out as well.

usage (MI355X): python tools/time_robust_mean.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import kernels, pytree, tree_util as tu  # noqa: E402

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


def torch_trimmed(rows, t):
    K = rows.shape[0]
    return torch.sort(rows, dim=0).values[t:K - t].sum(0) * (1.0 / (K - 2 * t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="16 clients, 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_mean_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 16 if args.small else 128
    t = kernels.trim_count(TRIM, K)

    runs, reps, res = {}, {}, {"clients": K, "trim": TRIM, "t": t}

    def slab_legs(name, slab, n):
        ones = [1] * K
        outs = [torch.empty(slab.num_params, dtype=torch.float32, device=dev) for _ in range(3)]
        runs[name + "_a"] = lambda: slab.trimmed_mean(TRIM, out=outs[0])
        runs[name + "_b"] = lambda: slab.median(out=outs[1])
        runs[name + "_c"] = lambda: slab.mean(ones, out=outs[2])
        runs[name + "_d"] = lambda: torch_trimmed(slab.rows, t)
        for leg in "abcd":
            reps[name + "_" + leg] = n
        # the torch route agrees with (a) to rounding on these finite deltas (it sums in sorted order)
        a = torch.cat([x.reshape(-1) for x in pytree.leaves_of(slab.trimmed_mean(TRIM))])
        res[name + "_torch_max_abs_diff"] = float((a - runs[name + "_d"]()).abs().max().item())

    es = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), K, device=dev).fill_synthetic(seed=2)
    slab_legs("emnist_slab", es, 20)
    res["emnist"] = [K, es.num_params]

    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(K)]
    pairs = [(c, 1) for c in clients]
    leaves = [pytree.leaves_of(c) for c in clients]

    def tree_d():
        return [torch_trimmed(torch.stack([row[l].reshape(-1) for row in leaves]), t) for l in range(len(leaves[0]))]

    runs.update(emnist_tree_a=lambda: tu.tree_trimmed_mean(clients, TRIM), emnist_tree_b=lambda: tu.tree_median(clients),
                emnist_tree_c=lambda: tu.tree_mean(pairs), emnist_tree_d=tree_d)
    reps.update(emnist_tree_a=20, emnist_tree_b=20, emnist_tree_c=20, emnist_tree_d=20)

    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=0)
    slab_legs("big_slab", bs, 5)
    res["big"] = [K, Pb]
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
    summary = dict(res, summary=True, tool="tools/time_robust_mean.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("emnist_slab", "emnist_tree", "big_slab"):
        for leg in "ab":
            summary[f"{shape}_{leg}_over_c"] = round(med[f"{shape}_{leg}"] / med[f"{shape}_c"], 4)
            summary[f"{shape}_{leg}_over_d"] = round(med[f"{shape}_{leg}"] / med[f"{shape}_d"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
