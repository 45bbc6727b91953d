"""Times Krum, multi-Krum and geometric-median rounds with the selection on the host
(select="host": Gram, the copy to the host, numpy, a pinned upload, the fold) and on the device
(select="device": Gram, the select kernels, the fold, no host visit), and the two select entries
alone.

Shapes: 128 clients x 4 Mi float32 as a slab, and 128 clients x EMNIST-CNN (8 leaves, 1,206,590
float32 params; configs[1] of BASELINE.json) as a slab and as separate pytrees. Legs on each, for
both routes: krum(f, 1), krum(f, K - f) and geometric_median() (4 iterations), f = 12. Alone, on
the big slab's Gram matrix and on one of 1024 clients: fjagg_krum_select for m = 1 and m = K - f,
and fjagg_weiszfeld_select.

Each pass times every leg in turn (host and device routes of a leg back to back: interleaved),
after a warm-up of all of them, with the fence-free kernels.Event around back-to-back calls; the
host route's wait for the device between its two passes is inside its time. For the device route
the host's own time per call (a wall clock around the calls, before the synchronise) is recorded
too: that is how long the caller is held. One JSON line per pass and a summary line with the
medians and the spread (max - min over the passes) of each leg; the summary is appended to --out.

usage (MI355X): python tools/time_robust_select_device.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import kernels, tree_util as tu  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}


def tmap(f, t):
    return {k: tmap(f, v) for k, v in t.items()} if isinstance(t, dict) else f(t)


def per_call_ms(fn, reps):
    """(device ms per call between two events, host ms per call until the last call returned)."""
    s = torch.cuda.current_stream()
    e0, e1 = kernels.Event(), kernels.Event()
    torch.cuda.synchronize()
    e0.record(s)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = (time.perf_counter() - t0) * 1e3 / reps
    e1.record(s)
    return e0.elapsed_time(e1) / reps, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="16 clients, 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_select_device_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 16 if args.small else 128
    f = 2 if args.small else 12
    runs, reps = {}, {}
    res = {"clients": K, "num_byzantine": f, "iterations": 4}

    def legs(name, krum, median, n):
        for select in ("host", "device"):
            runs[f"{name}_krum1_{select}"] = lambda s=select: krum(f, 1, select=s)
            runs[f"{name}_krumKf_{select}"] = lambda s=select: krum(f, K - f, select=s)
            runs[f"{name}_median_{select}"] = lambda s=select: median(select=s)
        for leg in ("krum1", "krumKf", "median"):
            reps[f"{name}_{leg}_host"] = reps[f"{name}_{leg}_device"] = n

    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=0)
    legs("big_slab", bs.krum, bs.geometric_median, 4)
    res["big"] = [K, Pb]
    es = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), K, device=dev).fill_synthetic(seed=2)
    legs("emnist_slab", es.krum, es.geometric_median, 10)
    res["emnist"] = [K, es.num_params]
    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(K)]
    legs("emnist_tree", lambda *a, **kw: tu.tree_krum(clients, *a, **kw),
         lambda **kw: tu.tree_geometric_median(clients, **kw), 10)

    # the select entries alone
    K2 = 64 if args.small else 1024
    wide = fedjax_amd.ClientDeltaSlab({"w": np.zeros(4096, np.float32)}, K2, device=dev).fill_synthetic(seed=5)
    f2 = (K2 - 3) // 4
    for name, G, ff in ((f"select_K{K}", bs.gram(), f), (f"select_K{K2}", wide.gram(), f2)):
        k = G.shape[0]
        runs[name + "_krum1"] = lambda G=G, ff=ff: kernels.krum_select_device(G, ff, 1)
        runs[name + "_krumKf"] = lambda G=G, ff=ff, k=k: kernels.krum_select_device(G, ff, k - ff)
        runs[name + "_weiszfeld"] = lambda G=G: kernels.weiszfeld_select_device(G)
        for leg in ("krum1", "krumKf", "weiszfeld"):
            reps[f"{name}_{leg}"] = 20
    res["select_alone"] = {f"select_K{K}": [K, f], f"select_K{K2}": [K2, f2]}
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    hosts = {k: [] for k in runs}
    for p in range(args.passes):
        row = {"pass": p}
        for name, fn in runs.items():
            ms, host = per_call_ms(fn, reps[name])
            times[name].append(ms)
            hosts[name].append(host)
            row[name + "_ms"] = round(ms, 4)
        print(json.dumps(row), flush=True)
    summary = dict(res, summary=True, tool="tools/time_robust_select_device.py", passes=args.passes,
                   small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(float(np.median(times[k])), 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
        if not k.endswith("_host"):
            summary[k + "_host_wall_ms"] = round(float(np.median(hosts[k])), 4)
    for shape in ("big_slab", "emnist_slab", "emnist_tree"):
        for leg in ("krum1", "krumKf", "median"):
            h, d = summary[f"{shape}_{leg}_host_ms"], summary[f"{shape}_{leg}_device_ms"]
            summary[f"{shape}_{leg}_device_over_host"] = round(d / h, 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f_out:
        f_out.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
