"""Times the top-k sparsified mean against the dense mean of the same bytes and a torch route.

Slab, 128 clients x 4 Mi float32, Gaussian deltas, k = 1 % and 10 % (suffix 1 / 10):
  (a) ClientDeltaSlab.topk_mean
  (b) ClientDeltaSlab.topk_thresholds alone (the three histogram passes and the scans)
  (c) ClientDeltaSlab.mean of the same slab: the one-read floor (the select reads the deltas
      three times and the masked fold once more)
  (d) the torch route: topk of abs, a where against the k-th value, mean over the K x P copy
      (skipped with --no-torch)
  (e) leg (a) on a slab whose magnitudes all share one top-level histogram bin ([1, 1.125)):
      what contention on a hot bin costs
Slab and pytrees, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json): (a), (b), (c), (d) on the slab as ta / tb / tc / td, and tree_util.tree_topk_mean
against tree_util.tree_mean over separate pytrees as tp / tpc.

Each pass times every leg in turn (interleaved), after a warm-up of every shape, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line
with the medians, the spread (max - min) of each and the ratios: reported, not gated. --out
appends the lines to a file (profiles/topk_mean_timing.jsonl).

usage (MI355X): python tools/time_topk_mean.py [--passes 7] [--small] [--no-torch] [--out FILE]
"""
import argparse
import json
import os
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


def torch_route(rows, c, inv_k):
    """Unit weights: keep every |x| >= the c-th largest |x| of its row, then the mean."""
    mag = rows.abs()
    kth = torch.topk(mag, c, dim=1, sorted=False).values.amin(dim=1, keepdim=True)
    return torch.where(mag >= kth, rows, torch.zeros((), dtype=rows.dtype, device=rows.device)).sum(0) * inv_k


def gaussian_slab(template, K, dev, seed):
    slab = fedjax_amd.ClientDeltaSlab(template, K, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    slab.rows.copy_(torch.randn(slab.rows.shape, generator=g, device=dev) * 0.01)
    return slab


def hot_bin_slab(template, K, dev, seed):
    """Every magnitude in [1, 1.125): one bin of the top-level histogram."""
    slab = fedjax_amd.ClientDeltaSlab(template, K, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    mag = 1.0 + 0.1249 * torch.rand(slab.rows.shape, generator=g, device=dev)
    sign = torch.randint(0, 2, slab.rows.shape, generator=g, device=dev).to(torch.float32) * 2 - 1
    slab.rows.copy_(mag * sign)
    return slab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="8 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch legs")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    Ks, Ps = (8, 64 * 1024) if args.small else (128, 4 * 1024 * 1024)
    slab = gaussian_slab({"w": np.zeros(Ps, np.float32)}, Ks, dev, 0)
    hot = hot_bin_slab({"w": np.zeros(Ps, np.float32)}, Ks, dev, 1)
    Kt = 8 if args.small else 128
    tslab = gaussian_slab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, dev, 2)
    Pt = tslab.num_params
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    ones, tones = [1] * Ks, [1] * Kt
    pairs = list(zip(clients, tones))
    outs = {n: torch.empty(Ps, dtype=torch.float32, device=dev) for n in ("a1", "a10", "c", "e1", "e10")}
    touts = {n: torch.empty(Pt, dtype=torch.float32, device=dev) for n in ("ta1", "ta10", "tc")}

    runs, reps = {}, {}
    for pct, frac in ((1, 0.01), (10, 0.1)):
        runs[f"a{pct}"] = lambda f=frac, o=outs[f"a{pct}"]: slab.topk_mean(ones, f, out=o)
        runs[f"b{pct}"] = lambda f=frac: slab.topk_thresholds(f)
        runs[f"e{pct}"] = lambda f=frac, o=outs[f"e{pct}"]: hot.topk_mean(ones, f, out=o)
        runs[f"ta{pct}"] = lambda f=frac, o=touts[f"ta{pct}"]: tslab.topk_mean(tones, f, out=o)
        runs[f"tb{pct}"] = lambda f=frac: tslab.topk_thresholds(f)
        runs[f"tp{pct}"] = lambda f=frac: tu.tree_topk_mean(pairs, f)
        reps.update({f"a{pct}": 10, f"b{pct}": 10, f"e{pct}": 10, f"ta{pct}": 20, f"tb{pct}": 20, f"tp{pct}": 20})
        if not args.no_torch:
            runs[f"d{pct}"] = lambda c=kernels.topk_count(frac, Ps): torch_route(slab.rows, c, 1.0 / Ks)
            runs[f"td{pct}"] = lambda c=kernels.topk_count(frac, Pt): torch_route(tslab.rows, c, 1.0 / Kt)
            reps.update({f"d{pct}": 2, f"td{pct}": 5})
    runs["c"] = lambda: slab.mean(ones, out=outs["c"])
    runs["tc"] = lambda: tslab.mean(tones, out=touts["tc"])
    runs["tpc"] = lambda: tu.tree_mean(pairs)
    reps.update({"c": 20, "tc": 40, "tpc": 40})

    got = runs["a10"]()
    tree10, slab10 = runs["tp10"](), runs["ta10"]()
    flat = lambda t: torch.cat([x.reshape(-1) for x in fedjax_amd.pytree.leaves_of(t)])
    res = {"slab": [Ks, Ps], "pytree": [Kt, Pt], "chunk": kernels.TOPK_CHUNK,
           "sent_10pct_min_max": [int(got.sent.min().item()), int(got.sent.max().item())],
           "hot_sent_10pct_min_max": [int(v.item()) for v in (lambda s: (s.min(), s.max()))(runs["e10"]().sent)],
           "slab_and_tree_same_bits": bool(torch.equal(flat(tree10.mean).view(torch.int32),
                                                       flat(slab10.mean).view(torch.int32))),
           "full_keep_equals_mean": bool(torch.equal(flat(tslab.topk_mean(tones, Pt).mean).view(torch.int32),
                                                     flat(tslab.mean(tones)).view(torch.int32)))}
    if not args.no_torch:
        res["torch_route_max_abs_diff"] = float((runs["td10"]() - touts["ta10"]).abs().max().item())
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
    summary = {"summary": True, "passes": args.passes}
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for pct in (1, 10):
        summary[f"a{pct}_over_c"] = round(med[f"a{pct}"] / med["c"], 3)
        summary[f"b{pct}_over_c"] = round(med[f"b{pct}"] / med["c"], 3)
        summary[f"e{pct}_over_a{pct}"] = round(med[f"e{pct}"] / med[f"a{pct}"], 3)
        summary[f"ta{pct}_over_tc"] = round(med[f"ta{pct}"] / med["tc"], 3)
        summary[f"tp{pct}_over_tpc"] = round(med[f"tp{pct}"] / med["tpc"], 3)
        summary[f"tp{pct}_over_ta{pct}"] = round(med[f"tp{pct}"] / med[f"ta{pct}"], 3)
        if f"d{pct}" in runs:
            summary[f"d{pct}_over_a{pct}"] = round(med[f"d{pct}"] / med[f"a{pct}"], 2)
            summary[f"td{pct}_over_ta{pct}"] = round(med[f"td{pct}"] / med[f"ta{pct}"], 2)
        summary[f"a{pct}_read_GBs"] = round(4 * Ks * Ps * 4 / med[f"a{pct}"] / 1e6, 1)  # four reads of the slab
        summary[f"b{pct}_read_GBs"] = round(3 * Ks * Ps * 4 / med[f"b{pct}"] / 1e6, 1)
        summary[f"fold{pct}_read_GBs"] = round(Ks * Ps * 4 / max(med[f"a{pct}"] - med[f"b{pct}"], 1e-9) / 1e6, 1)
    summary["c_read_GBs"] = round(Ks * Ps * 4 / med["c"] / 1e6, 1)
    emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
