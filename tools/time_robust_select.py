"""Times the Gram pass and the two aggregates built on it (Krum, the geometric median) against the
unit-weight mean of the same bytes and against torch.mm / torch.cdist on the slab.

Shapes: 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json) as a slab and as separate pytrees (every (client, leaf) its own device tensor),
and 128 clients x 4 Mi float32 as a slab. Legs on each:
  (g) the Gram pass alone: slab.gram() / tree_gram
  (k) a whole Krum round, f = 12, one client selected: Gram, the copy to the host, the selection, the fold
  (m) a whole geometric-median round, 4 iterations: Gram, the copy, Weiszfeld on the host, the fold
  (c) the mean with unit weights over the same deltas, same build: one read of the bytes
  (t) torch.mm(rows, rows.T) (float32 accumulation, no stated bound)   } slabs only, where torch
  (d) torch.cdist(rows, rows)                                          } runs them
The rounds (k) and (m) wait for the host between their two passes; their times include that wait.

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each, the Gram pass as a multiple
of (c), of (t) and of the derived matrix-instruction floor pairs * P * 2 / 157.3e12 (pairs: the
K (K + 1) / 2 entries of one triangle); the summary record is appended to --out as well.

usage (MI355X): python tools/time_robust_select.py [--passes 7] [--small] [--out FILE]
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
MFMA_F32_PEAK = 157.3e12  # FLOP/s of v_mfma_f32_32x32x2_f32 on MI355X


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
    ap.add_argument("--small", action="store_true", help="16 clients, 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_select_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 16 if args.small else 128
    f = 2 if args.small else 12

    runs, reps, res = {}, {}, {"clients": K, "num_byzantine": f, "iterations": 4, "chain": kernels.GRAM_CHAIN}

    def floor_ms(P):
        return K * (K + 1) / 2 * P * 2 / MFMA_F32_PEAK * 1e3

    def slab_legs(name, slab, n):
        ones = [1] * K
        out = torch.empty(slab.num_params, dtype=torch.float32, device=dev)
        gram = torch.empty(K, K, dtype=torch.float64, device=dev)
        runs[name + "_g"] = lambda: slab.gram(out=gram)
        runs[name + "_k"] = lambda: slab.krum(f)
        runs[name + "_m"] = lambda: slab.geometric_median()
        runs[name + "_c"] = lambda: slab.mean(ones, out=out)
        legs = "gkmc"
        for leg, fn in (("t", lambda: torch.mm(slab.rows, slab.rows.T)), ("d", lambda: torch.cdist(slab.rows, slab.rows))):
            try:  # where torch runs them
                got = fn()
                torch.cuda.synchronize()
                runs[name + "_" + leg] = fn
                legs += leg
                if leg == "t":
                    g64 = slab.gram()
                    res[name + "_mm_max_rel_diff"] = float(((got.double() - g64).abs().max() / g64.abs().max()).item())
            except Exception as e:  # noqa: BLE001
                res[name + "_" + leg + "_error"] = type(e).__name__
        for leg in legs:
            reps[name + "_" + leg] = n
        res[name + "_floor_ms"] = round(floor_ms(slab.num_params), 4)

    es = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), K, device=dev).fill_synthetic(seed=2)
    slab_legs("emnist_slab", es, 10)
    res["emnist"] = [K, es.num_params]

    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(K)]
    pairs = [(c, 1) for c in clients]
    runs.update(emnist_tree_g=lambda: tu.tree_gram(clients), emnist_tree_k=lambda: tu.tree_krum(clients, f),
                emnist_tree_m=lambda: tu.tree_geometric_median(clients), emnist_tree_c=lambda: tu.tree_mean(pairs))
    reps.update(emnist_tree_g=10, emnist_tree_k=10, emnist_tree_m=10, emnist_tree_c=10)
    res["emnist_tree_floor_ms"] = res["emnist_slab_floor_ms"]

    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, K, device=dev).fill_synthetic(seed=0)
    slab_legs("big_slab", bs, 4)
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
    summary = dict(res, summary=True, tool="tools/time_robust_select.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("emnist_slab", "emnist_tree", "big_slab"):
        summary[f"{shape}_g_over_c"] = round(med[f"{shape}_g"] / med[f"{shape}_c"], 4)
        summary[f"{shape}_g_over_floor"] = round(med[f"{shape}_g"] / res[f"{shape}_floor_ms"], 4)
        for leg in "td":
            if f"{shape}_{leg}" in med:
                summary[f"{shape}_g_over_{leg}"] = round(med[f"{shape}_g"] / med[f"{shape}_{leg}"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f_out:
        f_out.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
