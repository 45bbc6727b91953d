"""Times the bucketed trimmed mean and median (bucket means formed inside the column kernel)
against the route the parent's entries allow, a 128-row trimmed mean and the plain mean.

Shapes: 1024 clients x 4 Mi float32 as a slab, and 1024 clients x EMNIST-CNN (8 leaves, 1,206,590
float32 params; configs[1] of BASELINE.json) as a slab and as separate pytrees (every (client,
leaf) its own device tensor). Bucket size 8, consecutive clients: 128 buckets. Legs on each:
  (a) trimmed_mean(0.1, bucket_size=8)            one launch, no temporary
  (b) median(bucket_size=8)
  (c) two launches: grouped_mean of unit weights into a 128 x P result (the bucket means, up to
      the fold's +0 start), then the trimmed mean over it
  (d) the trimmed mean of the first 128 rows of the same slab (slab shapes only): the column
      routine alone, an eighth of the bytes
  (e) the mean with unit weights over the same deltas: the floor, one read

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each, and (a), (b) as multiples
of (c), (d) and (e); the summary record is appended to --out as well.

usage (MI355X): python tools/time_bucketed_mean.py [--passes 7] [--small] [--out FILE]
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
TRIM, S = 0.1, 8


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
    ap.add_argument("--small", action="store_true", help="64 clients, 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bucketed_mean_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 64 if args.small else 1024
    B = kernels.bucket_count(K, S)
    t = kernels.bucket_trim_count(TRIM, B)
    ids = [k // S for k in range(K)]
    ones = [1] * K
    scale = float(np.float32(tu._inverse(B - 2 * t)))

    runs, reps, res = {}, {}, {"clients": K, "bucket_size": S, "buckets": B, "trim": TRIM, "t": t,
                               "staging": "two reads (no second LDS tile)"}

    def slab_legs(name, slab, n):
        P = slab.num_params
        outs = [torch.empty(P, dtype=torch.float32, device=dev) for _ in range(5)]
        means = torch.empty(B, slab.row_stride, dtype=torch.float32, device=dev)
        head = slab.rows[:B]

        def two_launches():
            slab.grouped_mean(ones, ids, B, out=means)
            return kernels.trim_dense(means[:, :P], t, scale=scale, out=outs[2])

        runs[name + "_a"] = lambda: slab.trimmed_mean(TRIM, bucket_size=S, out=outs[0])
        runs[name + "_b"] = lambda: slab.median(bucket_size=S, out=outs[1])
        runs[name + "_c"] = two_launches
        runs[name + "_d"] = lambda: kernels.trim_dense(head, t, scale=scale, out=outs[3])
        runs[name + "_e"] = lambda: slab.mean(ones, out=outs[4])
        for leg in "abcde":
            reps[name + "_" + leg] = n
        # the two-launch route agrees with (a) to rounding (its bucket sums start from +0 and multiply by 1)
        runs[name + "_a"]()
        two_launches()
        res[name + "_two_launch_max_abs_diff"] = float((outs[0] - outs[2]).abs().max().item())

    es = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), K, device=dev).fill_synthetic(seed=2)
    slab_legs("emnist_slab", es, 10)
    res["emnist"] = [K, es.num_params]

    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(K)]
    pairs = [(c, 1) for c in clients]

    def tree_two_launches():
        return tu.tree_trimmed_mean(tu.tree_grouped_mean(pairs, ids, B), t)

    runs.update(emnist_tree_a=lambda: tu.tree_trimmed_mean(clients, TRIM, bucket_size=S),
                emnist_tree_b=lambda: tu.tree_median(clients, bucket_size=S), emnist_tree_c=tree_two_launches,
                emnist_tree_e=lambda: tu.tree_mean(pairs))
    reps.update(emnist_tree_a=10, emnist_tree_b=10, emnist_tree_c=10, emnist_tree_e=10)

    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=0)
    slab_legs("big_slab", bs, 3)
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
    summary = dict(res, summary=True, tool="tools/time_bucketed_mean.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("emnist_slab", "emnist_tree", "big_slab"):
        for leg in "ab":
            for other in "cde":
                if f"{shape}_{other}" in med:
                    summary[f"{shape}_{leg}_over_{other}"] = round(med[f"{shape}_{leg}"] / med[f"{shape}_{other}"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
