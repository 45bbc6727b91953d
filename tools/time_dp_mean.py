"""Times the differentially private clipped mean against the clipped mean alone and against
the composed route (clipped mean, then a normal draw per leaf, then an add).

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py), and pytree, 128 clients x
EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of BASELINE.json), every
(client, leaf) its own device tensor. On each:
  (a) dp_clipped_mean: the noise drawn in the fold's epilogue
  (b) clipped_mean: the same passes without noise, the floor of (a)
  (c) clipped_mean, then random.normal(keys[l]) per leaf, then leaf.add_(z * stddev): what a
      caller composes from the existing parts (L + 1 more launches, a noise tensor per leaf)

Each pass times (a), (b), (c) on the slab and on the pytrees in turn (interleaved), after a
warm-up of every shape, with the fence-free kernels.Event around back-to-back calls. One JSON
line per pass and a summary line with the medians, the spread (max - min over the passes) of
each and the ratios (a)/(b), (a)/(c); the summary record is appended to --out as well.

usage (MI355X): python tools/time_dp_mean.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import kernels, pytree, random as fjr, tree_util as tu  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}
STDDEV = 1e-3


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


def add_noise(mean, key, sd):
    leaves = pytree.leaves_of(mean)
    for leaf, k in zip(leaves, fjr.split(key, len(leaves))):
        leaf.add_(fjr.normal(k, tuple(leaf.shape), device=leaf.device) * sd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dp_mean_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    key = fjr.PRNGKey(7)
    sd = torch.tensor(np.float32(STDDEV), device=dev)

    # ---- slab
    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Ps, np.float32)}, Ks, device=dev).fill_synthetic(seed=0)
    ws = rng.randint(1, 501, size=Ks).tolist()
    # client k scaled by 2**((k % 5) - 2), clip norm = the median norm: about half are clipped
    slab.rows.mul_(torch.tensor([2.0 ** ((k % 5) - 2) for k in range(Ks)], device=dev)[:, None])
    Cs = float(slab.l2_norms().median().item())
    outs = [torch.empty(Ps, dtype=torch.float32, device=dev) for _ in range(3)]

    def slab_a():
        return slab.dp_clipped_mean(ws, Cs, STDDEV, key, out=outs[0])

    def slab_b():
        return slab.clipped_mean(ws, Cs, out=outs[1])

    def slab_c():
        got = slab.clipped_mean(ws, Cs, out=outs[2])
        add_noise(got.mean, key, sd)
        return got

    # ---- pytree
    Kt = 8 if args.small else 128
    tslab = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, device=dev)
    tslab.fill_synthetic(seed=2)
    tslab.rows.mul_(torch.tensor([2.0 ** ((k % 5) - 2) for k in range(Kt)], device=dev)[:, None])
    Ct = float(tslab.l2_norms().median().item())
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    wt = rng.randint(1, 501, size=Kt).tolist()
    pairs = list(zip(clients, wt))

    def tree_a():
        return tu.tree_dp_clipped_mean(pairs, Ct, STDDEV, key)

    def tree_b():
        return tu.tree_clipped_mean(pairs, Ct)

    def tree_c():
        got = tu.tree_clipped_mean(pairs, Ct)
        add_noise(got.mean, key, sd)
        return got

    runs = {"slab_a": slab_a, "slab_b": slab_b, "slab_c": slab_c, "tree_a": tree_a, "tree_b": tree_b, "tree_c": tree_c}
    reps = {"slab_a": 10, "slab_b": 10, "slab_c": 10, "tree_a": 20, "tree_b": 20, "tree_c": 20}
    res = {"slab": [Ks, Ps], "pytree": [Kt, tslab.num_params], "stddev": STDDEV}
    for route in ("slab", "tree"):  # the fused and the composed route give the same bits
        fused, composed = runs[route + "_a"](), runs[route + "_c"]()
        res[route + "_fused_equals_composed"] = all(
            torch.equal(x.view(torch.int32), y.view(torch.int32))
            for x, y in zip(pytree.leaves_of(fused.mean), pytree.leaves_of(composed.mean)))
        res[route + "_clipped"] = int(fused.clipped.sum().item())
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
    summary = dict(res, summary=True, tool="tools/time_dp_mean.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for route in ("slab", "tree"):
        summary[route + "_a_over_b"] = round(med[route + "_a"] / med[route + "_b"], 4)
        summary[route + "_a_over_c"] = round(med[route + "_a"] / med[route + "_c"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
