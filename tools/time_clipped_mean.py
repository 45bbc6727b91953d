"""Times the clipped weighted mean against its floor and against the per-client route.

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py):
  (a) ClientDeltaSlab.clipped_mean
  (b) kernels.l2_squared_dense + kernels.weighted_sum_l2_dense on the same slab: the same
      bytes read twice with no clipping, the floor of a two-pass exact clipped mean.
Pytree, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json), every (client, leaf) its own device tensor:
  (c) tree_util.tree_clipped_mean
  (d) the loop of fedjax/algorithms/mime_lite.py:131-149 over the existing per-client
      functions: tree_l2_norm, tree_clip_by_global_norm, tree_l2_norm, tree_add(tree_weight).

Each pass times (a), (b), (c), (d) in turn (interleaved), after a warm-up of every shape,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a
summary line with the medians, the spread of each and the ratios (a)/(b), (c)/(d).

usage (MI355X): python tools/time_clipped_mean.py [--passes 5] [--small]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)

    # ---- slab
    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Ps, np.float32)}, Ks, device=dev).fill_synthetic(seed=0)
    ws = rng.randint(1, 501, size=Ks).tolist()
    # client k scaled by 2**((k % 5) - 2), clip norm = the median norm: about half are clipped
    slab.rows.mul_(torch.tensor([2.0 ** ((k % 5) - 2) for k in range(Ks)], device=dev)[:, None])
    Cs = float(slab.l2_norms().median().item())
    w_dev = slab.weight_vector(ws)
    inv = float(np.float32(1.0 / float(sum(ws))))
    out_a = torch.empty(Ps, dtype=torch.float32, device=dev)
    out_b = torch.empty(Ps, dtype=torch.float32, device=dev)

    def run_a():
        return slab.clipped_mean(ws, Cs, out=out_a)

    def run_b():
        kernels.l2_squared_dense(slab.rows)
        return kernels.weighted_sum_l2_dense(slab.rows, w_dev, scale=inv, out=out_b, nontemporal=True)

    # ---- pytree
    Kt = 8 if args.small else 128
    tslab = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, device=dev)
    tslab.fill_synthetic(seed=2)
    tslab.rows.mul_(torch.tensor([2.0 ** ((k % 5) - 2) for k in range(Kt)], device=dev)[:, None])
    Ct = float(tslab.l2_norms().median().item())
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    wt = rng.randint(1, 501, size=Kt).tolist()
    pairs = list(zip(clients, wt))

    def run_c():
        return tu.tree_clipped_mean(pairs, Ct)

    def run_d():
        total, W, diag = tu.tree_zeros_like(clients[0]), 0.0, []
        for delta, n in pairs:
            norm = tu.tree_l2_norm(delta)
            delta = tu.tree_clip_by_global_norm(delta, Ct)
            clipped_norm = tu.tree_l2_norm(delta)
            diag.append((norm, clipped_norm))
            total = tu.tree_add(total, tu.tree_weight(delta, n))
            W += n
        return tu._eager(tu.tree_inverse_weight(total, W)), diag

    got_a, got_c = run_a(), run_c()
    res = {"slab": [Ks, Ps], "pytree": [Kt, tslab.num_params],
           "slab_clipped": int(got_a.clipped.sum().item()), "pytree_clipped": int(got_c.clipped.sum().item())}
    # the two pytree routes compute the same mean (norm reduction orders differ: last bits)
    mean_d, _ = run_d()
    err = max(float((a - b).abs().max().item()) for a, b in
              zip(fedjax_amd.pytree.leaves_of(got_c.mean), fedjax_amd.pytree.leaves_of(mean_d)))
    res["pytree_routes_max_abs_diff"] = err
    print(json.dumps(res), flush=True)

    reps = {"a": 10, "b": 10, "c": 20, "d": 3}
    runs = {"a": run_a, "b": run_b, "c": run_c, "d": run_d}
    for name, fn in runs.items():  # warm up every shape
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
    summary = {"summary": True, "passes": args.passes}
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    summary["a_over_b"] = round(med["a"] / med["b"], 4)
    summary["c_over_d"] = round(med["c"] / med["d"], 4)
    summary["a_read_GBs"] = round(2 * Ks * Ps * 4 / med["a"] / 1e6, 1)
    summary["b_read_GBs"] = round(2 * Ks * Ps * 4 / med["b"] / 1e6, 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
