"""Times the mean around the median against the trimmed mean and the plain mean of the same
bytes, and a Bulyan round against its parts and against a Krum round.

Shapes: 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json) as a slab and as separate pytrees, and 128 clients x 4 Mi float32 as a slab.
Legs on each:
  (e) mean_around_median(K - 12)
  (a) trimmed_mean(0.1) of the same build: the kernel (e) shares its sort and its sum with
  (c) the mean with unit weights over the same deltas: the floor, one read
Bulyan legs on a slab of 160 clients x EMNIST-CNN, f = 16 (theta = 128 selected, keep = 96):
  (g) the Gram pass
  (h) the host step alone: the device-to-host copy of G and robust.bulyan_select
  (b) the whole round, slab.bulyan(16)
  (k) a Krum round on the same slab, slab.krum(16, 128)

Each pass times every leg in turn (interleaved), after a warm-up of all of them, with the
fence-free kernels.Event around back-to-back calls; (h), (b) and (k) synchronise with the host
inside, so they are timed with the wall clock around a synchronised call. One JSON line per
pass and a summary line with the medians, the spread (max - min over the passes) of each, and
(e) as a multiple of (a) and of (c); the summary record is appended to --out as well.

usage (MI355X): python tools/time_bulyan.py [--passes 7] [--small] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fedjax_amd  # noqa: E402
from fedjax_amd import kernels, robust, tree_util as tu  # noqa: E402

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


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="16 / 23 clients, 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bulyan_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 16 if args.small else 128
    keep = K - 12 if K > 12 else K
    KB, f = (23, 5) if args.small else (160, 16)

    runs, reps, timer = {}, {}, {}
    res = {"clients": K, "keep": keep, "trim": TRIM, "bulyan_clients": KB, "bulyan_f": f}

    def slab_legs(name, slab, n):
        ones = [1] * K
        outs = [torch.empty(slab.num_params, dtype=torch.float32, device=dev) for _ in range(3)]
        runs[name + "_e"] = lambda: slab.mean_around_median(keep, out=outs[0])
        runs[name + "_a"] = lambda: slab.trimmed_mean(TRIM, out=outs[1])
        runs[name + "_c"] = lambda: slab.mean(ones, out=outs[2])
        for leg in "eac":
            reps[name + "_" + leg] = n

    template = tmap(lambda s: np.zeros(s, np.float32), EMNIST)
    es = fedjax_amd.ClientDeltaSlab(template, K, device=dev).fill_synthetic(seed=2)
    slab_legs("emnist_slab", es, 20)
    res["emnist"] = [K, es.num_params]

    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(K)]
    pairs = [(c, 1) for c in clients]
    runs.update(emnist_tree_e=lambda: tu.tree_mean_around_median(clients, keep),
                emnist_tree_a=lambda: tu.tree_trimmed_mean(clients, TRIM), emnist_tree_c=lambda: tu.tree_mean(pairs))
    reps.update(emnist_tree_e=20, emnist_tree_a=20, emnist_tree_c=20)

    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=0)
    slab_legs("big_slab", bs, 5)
    res["big"] = [K, Pb]

    bl = fedjax_amd.ClientDeltaSlab(template, KB, device=dev).fill_synthetic(seed=3)
    gram = bl.gram()
    got = bl.bulyan(f)
    res["bulyan_selected"], res["bulyan_keep"] = int(len(got.selected)), int(got.keep)
    runs.update(bulyan_g=lambda: bl.gram(out=gram), bulyan_h=lambda: robust.bulyan_select(gram.cpu().numpy(), f),
                bulyan_b=lambda: bl.bulyan(f), bulyan_k=lambda: bl.krum(f, KB - 2 * f))
    reps.update(bulyan_g=10, bulyan_h=3, bulyan_b=3, bulyan_k=3)
    timer.update(bulyan_h=wall_ms, bulyan_b=wall_ms, bulyan_k=wall_ms)
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every leg
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for p in range(args.passes):
        row = {"pass": p}
        for name, fn in runs.items():
            ms = timer.get(name, per_call_ms)(fn, reps[name])
            times[name].append(ms)
            row[name + "_ms"] = round(ms, 4)
        print(json.dumps(row), flush=True)
    med = {k: float(np.median(v)) for k, v in times.items()}
    summary = dict(res, summary=True, tool="tools/time_bulyan.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("emnist_slab", "emnist_tree", "big_slab"):
        summary[f"{shape}_e_over_a"] = round(med[f"{shape}_e"] / med[f"{shape}_a"], 4)
        summary[f"{shape}_e_over_c"] = round(med[f"{shape}_e"] / med[f"{shape}_c"], 4)
    summary["bulyan_b_over_k"] = round(med["bulyan_b"] / med["bulyan_k"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f_out:
        f_out.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
