"""Times an FLTrust round against centered clipping and the clipped mean on the same slab, and
against a torch expression of the rule.

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py), synthetic deltas:
  (f)  ClientDeltaSlab.fltrust against the slab's own mean: every client has a small positive cosine,
       so every client is trusted and the fold reads every row
  (h)  the same against an unrelated synthetic vector: the cosines fall on both sides of 0, about half
       the clients are gated out and the fold skips their rows
  (cc) ClientDeltaSlab.centered_clip(tau, iterations=1) on the same slab: the yardstick, the same two
       reads plus a small factor step
  (cm) ClientDeltaSlab.clipped_mean([1] * K, tau)
  (e)  a torch expression of the rule (skipped with --no-torch: it makes K x P temporaries)
  (rp) the row pass alone, kernels.dotsq_dense     (rc) kernels.center_l2sq_rows over the same rows
Slab and pytrees, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json): (f), (cc), (cm), (e) on the slab as tf / tcc / tcm / te, and
  (d)  tree_util.tree_fltrust over separate pytrees, every (client, leaf) its own tensor

Each pass times every leg in turn (interleaved), after a warm-up of every shape, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line with
the medians, the spread (max - min) of each, the ratios and the acceptance figure: f within cc plus
three times the larger of the two spreads. --out appends the lines to a file
(profiles/fltrust_timing.jsonl). --kernel-stats DIR starts ONE fresh child of this tool under
`rocprofv3 --kernel-trace --stats` (a few calls of f, h, cc, tf and tcc, nothing timed), leaves its
CSVs in DIR and adds fltrust_kernel_by_grid.csv, the trace per kernel and grid.

usage (MI355X): python tools/time_fltrust.py [--passes 7] [--small] [--no-torch] [--out FILE]
                                             [--kernel-stats DIR]
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fedjax_amd  # noqa: E402
from fedjax_amd import kernels, tree_util as tu  # noqa: E402

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


def torch_route(rows, g):
    a = rows @ g
    n = rows.norm(dim=1)
    ns = g.norm()
    ts = torch.clamp(a / (n * ns), min=0.0, max=1.0)
    c = torch.where(ts > 0, ts * ns / n, torch.zeros_like(ts))
    return (rows * c[:, None]).sum(0) / ts.sum()


def setup(template, K, dev, seed):
    """(slab, g_all, g_half, tau): synthetic deltas; the slab's own mean as the server delta that
    trusts everybody, an unrelated synthetic vector as the one that gates about half; tau = the median
    distance from g_half for the two yardsticks."""
    slab = fedjax_amd.ClientDeltaSlab(template, K, device=dev).fill_synthetic(seed=seed)
    g_all = torch.empty(slab.num_params, dtype=torch.float32, device=dev)
    slab.mean([1] * K, out=g_all)
    g_half = torch.empty(1, slab.num_params, dtype=torch.float32, device=dev)
    kernels.fill_synth(g_half, seed=seed + 100, amp=0.01)
    tau = float(slab.centered_clip(1.0, g_half[0]).distances[0].median().item())
    return slab, g_all, g_half[0], tau


def row_image(rows, g, dev):
    """ptrs[K] | n[K] | ref_ptrs[K] of a slab's rows against one vector."""
    K, P = rows.shape
    ptrs = rows.data_ptr() + 4 * rows.stride(0) * np.arange(K, dtype=np.int64)
    return torch.from_numpy(np.concatenate([ptrs, np.full(K, P), np.full(K, g.data_ptr())]).astype(np.int64)).to(dev)


def summarise_trace(directory):
    """fltrust_kernel_by_grid.csv beside the profiler's CSVs: this library's kernels of the trace per
    (kernel, grid), calls and min / median / max duration. The profiler's own stats add up the shapes."""
    import csv
    import glob
    import re

    groups = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                m = re.search(r"(k_\w+(?:<[^>(]*>)?)", r["Kernel_Name"])
                if m:
                    key = (m.group(1), int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
                    groups.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(os.path.join(directory, "fltrust_kernel_by_grid.csv"), "w") as f:
        f.write("kernel,grid_x,grid_y,calls,min_ns,median_ns,max_ns\n")
        for (name, gx, gy), v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
            f.write(f'"{name}",{gx},{gy},{len(v)},{min(v)},{int(np.median(v))},{max(v)}\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch legs")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR",
                    help="run one fresh child under rocprofv3 --kernel-trace --stats, CSVs into DIR; nothing else")
    ap.add_argument("--stats-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_stats:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.kernel_stats, "-o", "fltrust", "--output-format",
               "csv", "--", sys.executable, os.path.abspath(__file__), "--stats-child"] + (["--small"] if args.small else [])
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(cmd).returncode
        if rc == 0:
            summarise_trace(args.kernel_stats)
        sys.exit(rc)
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab, g_all, g_half, taus = setup({"w": np.zeros(Ps, np.float32)}, Ks, dev, 0)
    outs = {k: torch.empty(Ps, dtype=torch.float32, device=dev) for k in ("f", "h", "cc", "cm")}
    ones = [1] * Ks
    nt = slab.rows.numel() * 4 >= tu.NONTEMPORAL_MIN_BYTES
    runs = {
        "f": lambda: slab.fltrust(g_all, out=outs["f"]),
        "h": lambda: slab.fltrust(g_half, out=outs["h"]),
        "cc": lambda: slab.centered_clip(taus, g_half, out=outs["cc"]),
    }
    if args.stats_child:  # a few calls of the rounds of both shapes under the profiler, nothing timed
        tslab, tg_all, tg_half, taut = setup(tmap(lambda s: np.zeros(s, np.float32), EMNIST), 8 if args.small else 128,
                                             dev, 2)
        runs["tf"] = lambda: tslab.fltrust(tg_all)
        runs["tcc"] = lambda: tslab.centered_clip(taut, tg_half)
        for _ in range(3):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        return
    image = row_image(slab.rows, g_half, dev)
    runs.update({
        "cm": lambda: slab.clipped_mean(ones, taus, out=outs["cm"]),
        "rp": lambda: kernels.dotsq_dense(slab.rows, g_half, nontemporal=nt),
        "rc": lambda: kernels.center_l2sq_rows(image, Ks, Ps),
    })

    Kt = 8 if args.small else 128
    tslab, tg_all, tg_half, taut = setup(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, dev, 2)
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    gtree = tmap(lambda v: v.clone(), tslab.unflatten(tg_all))
    touts = {k: torch.empty(tslab.num_params, dtype=torch.float32, device=dev) for k in ("tf", "tcc", "tcm")}
    tones = [1] * Kt
    runs.update({
        "tf": lambda: tslab.fltrust(tg_all, out=touts["tf"]),
        "tcc": lambda: tslab.centered_clip(taut, tg_half, out=touts["tcc"]),
        "tcm": lambda: tslab.clipped_mean(tones, taut, out=touts["tcm"]),
        "d": lambda: tu.tree_fltrust(clients, gtree),
    })
    reps = {"f": 10, "h": 10, "cc": 10, "cm": 10, "rp": 10, "rc": 10, "tf": 20, "tcc": 20, "tcm": 20, "d": 20, "e": 3,
            "te": 10}
    if not args.no_torch:
        runs["e"] = lambda: torch_route(slab.rows, g_all)
        runs["te"] = lambda: torch_route(tslab.rows, tg_all)

    got_f, got_h, got_tf, got_d = runs["f"](), runs["h"](), runs["tf"](), runs["d"]()
    flat = lambda tree: torch.cat([x.reshape(-1) for x in fedjax_amd.pytree.leaves_of(tree)])  # noqa: E731
    res = {"slab": [Ks, Ps], "pytree": [Kt, tslab.num_params], "nontemporal": bool(nt),
           "trusted_f": int(got_f.count.item()), "trusted_h": int(got_h.count.item()),
           "trusted_tf": int(got_tf.count.item()), "trusted_d": int(got_d.count.item()),
           "slab_and_tree_same_bits": bool(torch.equal(flat(got_d.mean).view(torch.int32),
                                                       flat(got_tf.mean).view(torch.int32)))}
    if not args.no_torch:
        res["torch_route_max_abs_diff"] = float((runs["te"]() - touts["tf"]).abs().max().item())
        res["mean_max_abs"] = float(touts["tf"].abs().max().item())
    emit(res)

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
        emit(row)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    summary = {"summary": True, "passes": args.passes}
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(spread[k], 4)
    for a, b in (("f", "cc"), ("h", "f"), ("f", "cm"), ("rp", "rc"), ("tf", "tcc"), ("d", "tf")):
        summary[f"{a}_over_{b}"] = round(med[a] / med[b], 4)
    if "e" in runs:
        summary["e_over_f"] = round(med["e"] / med["f"], 4)
        summary["te_over_tf"] = round(med["te"] / med["tf"], 4)
    for a, b in (("f", "cc"), ("tf", "tcc")):  # the acceptance figure: within the yardstick plus 3 spreads
        limit = med[b] + 3 * max(spread[a], spread[b])
        summary[f"{a}_limit_ms"] = round(limit, 4)
        summary[f"{a}_within_limit"] = bool(med[a] <= limit)
    # bytes the fold skips in h: the gated share of the second read, over the two reads of f
    summary["h_expected_over_f"] = round((1 + res["trusted_h"] / Ks) / 2, 4)
    summary["f_read_GBs"] = round(2 * Ks * Ps * 4 / med["f"] / 1e6, 1)
    summary["cc_read_GBs"] = round(2 * Ks * Ps * 4 / med["cc"] / 1e6, 1)
    emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
