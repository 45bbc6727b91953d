"""Times the trimmed mean and median by rank selection (method="select") at 1024
clients against the plain mean of the same bytes (the floor: one read), the bucketed route and
the route a caller composes from torch ops, and at 128 clients against the sorting kernels.

Shapes: 1024 clients x 4 Mi float32 as a slab; 1024 clients x EMNIST-CNN (8 leaves, 1,206,590
float32 params; configs[1] of BASELINE.json) as a slab and as separate pytrees; 128 clients x
4 Mi float32 as a slab. Legs at 1024 clients:
  (a) trimmed_mean(0.1, method="select")
  (b) median(method="select")
  (c) the mean with unit weights over the same deltas: the floor
  (d) trimmed_mean(0.1, bucket_size=8): a different estimator, the only other route past 128 clients
  (e) torch: torch.sort(rows, dim=0), a slice, .sum(0), a multiply (per leaf, after a torch.stack,
      for the pytrees); skipped, and recorded as null, when it does not fit in memory
At 128 clients: trimmed_mean(0.1) with method="select" and with method="sort".

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each and the ratios; the summary
record is appended to --out as well.

usage (MI355X): python tools/time_trim_select.py [--passes 7] [--small] [--out FILE]
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
TRIM, BUCKET = 0.1, 8


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
    ap.add_argument("--small", action="store_true", help="160 clients, 64 Ki slabs (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_select_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 160 if args.small else 1024
    t = kernels.trim_count(TRIM, K, select=True)
    runs, reps, res = {}, {}, {"clients": K, "trim": TRIM, "t": t, "bucket_size": BUCKET}

    def fits(fn, name):
        """fn once: False (and a null record) if the torch route runs out of memory."""
        try:
            fn()
            torch.cuda.synchronize()
            return True
        except torch.OutOfMemoryError:
            res[name + "_e_ms"] = None
            torch.cuda.empty_cache()
            return False

    def slab_legs(name, slab, n, n_torch):
        ones = [1] * K
        outs = [torch.empty(slab.num_params, dtype=torch.float32, device=dev) for _ in range(4)]
        runs[name + "_a"] = lambda: slab.trimmed_mean(TRIM, out=outs[0], method="select")
        runs[name + "_b"] = lambda: slab.median(out=outs[1], method="select")
        runs[name + "_c"] = lambda: slab.mean(ones, out=outs[2])
        runs[name + "_d"] = lambda: slab.trimmed_mean(TRIM, bucket_size=BUCKET, out=outs[3])
        for leg in "abcd":
            reps[name + "_" + leg] = n
        if fits(lambda: torch_trimmed(slab.rows, t), name):
            runs[name + "_e"], reps[name + "_e"] = (lambda: torch_trimmed(slab.rows, t)), n_torch

    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=0)
    slab_legs("big_slab", bs, 3, 1)
    res["big"] = [K, Pb]

    es = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), K, device=dev).fill_synthetic(seed=2)
    slab_legs("emnist_slab", es, 5, 1)
    res["emnist"] = [K, es.num_params]
    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(K)]
    pairs = [(c, 1) for c in clients]
    leaves = [pytree.leaves_of(c) for c in clients]

    def tree_e():
        return [torch_trimmed(torch.stack([row[l].reshape(-1) for row in leaves]), t) for l in range(len(leaves[0]))]

    runs.update(emnist_tree_a=lambda: tu.tree_trimmed_mean(clients, TRIM, method="select"),
                emnist_tree_b=lambda: tu.tree_median(clients, method="select"),
                emnist_tree_c=lambda: tu.tree_mean(pairs),
                emnist_tree_d=lambda: tu.tree_trimmed_mean(clients, TRIM, bucket_size=BUCKET))
    reps.update(emnist_tree_a=5, emnist_tree_b=5, emnist_tree_c=5, emnist_tree_d=5)
    if fits(tree_e, "emnist_tree"):
        runs["emnist_tree_e"], reps["emnist_tree_e"] = tree_e, 1

    # 128 clients: the selection kernel against the sorting one, the same bits
    Ks = 16 if args.small else 128
    ss = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, Ks, device=dev).fill_synthetic(seed=1)
    o128 = [torch.empty(Pb, dtype=torch.float32, device=dev) for _ in range(2)]
    runs["k128_select"] = lambda: ss.trimmed_mean(TRIM, out=o128[0], method="select")
    runs["k128_sort"] = lambda: ss.trimmed_mean(TRIM, out=o128[1], method="sort")
    reps.update(k128_select=5, k128_sort=5)
    res["k128"] = [Ks, Pb]
    runs["k128_select"](), runs["k128_sort"]()
    res["k128_same_bits"] = bool(torch.equal(o128[0].view(torch.int32), o128[1].view(torch.int32)))
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
    summary = dict(res, summary=True, tool="tools/time_trim_select.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("big_slab", "emnist_slab", "emnist_tree"):
        for leg in "ab":
            for other in "cde":
                if f"{shape}_{other}" in med:
                    summary[f"{shape}_{leg}_over_{other}"] = round(med[f"{shape}_{leg}"] / med[f"{shape}_{other}"], 4)
    summary["k128_select_over_sort"] = round(med["k128_select"] / med["k128_sort"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
