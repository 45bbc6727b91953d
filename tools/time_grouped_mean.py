"""Times the grouped weighted mean against its one-read floor and against what a user could
do before it.

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py), G = 4 groups, once with equal
groups and once with 70 / 20 / 9 / 1 % groups (clients assigned by a seeded shuffle):
  (a) ClientDeltaSlab.grouped_mean with the same weights and ids on every call: the member
      tables of the first call stay on the device (no table build or upload after it)
  (a_fresh) the same with other weights on every call, as a real round has them: every call
      sorts the ids, builds the tables and uploads them
  (b) ClientDeltaSlab.mean of the same slab: every row read once into ONE mean, the floor
  (c) G masked ClientDeltaSlab.mean passes with zero weights for the non-members: the slab is
      read G times (and 0 * inf poisons every group; the timing ignores that).
Pytree, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json), every (client, leaf) its own device tensor, G = 4 equal groups:
  (d) tree_util.tree_grouped_mean
  (e) one running sum per group on the library's tree ops, the loop of
      fedjax/algorithms/hyp_cluster.py:268-303.

Each pass times every leg in turn (interleaved), after a warm-up of every leg, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line
with the medians, the spread (max - min over passes) of each and the ratios (a)/(b), (a)/(c),
(d)/(e); everything is appended to profiles/grouped_mean_timing.jsonl as well.

usage (MI355X): python tools/time_grouped_mean.py [--passes 5] [--small] [--out FILE]
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
G = 4


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


def split_ids(K, fractions, seed):
    """K ids with the given group fractions (the last group takes the remainder), shuffled."""
    counts = [int(round(f * K)) for f in fractions[:-1]]
    counts.append(K - sum(counts))
    ids = np.repeat(np.arange(len(fractions)), counts)
    return np.random.RandomState(seed).permutation(ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_mean_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    sink = open(args.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    # ---- slab
    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Ps, np.float32)}, Ks, device=dev).fill_synthetic(seed=0)
    ws = rng.randint(1, 501, size=Ks).tolist()
    ws_turns = [ws[i:] + ws[:i] for i in range(1, 4)]  # a_fresh: consecutive calls never share weights
    out_g = torch.empty(G, slab.row_stride, dtype=torch.float32, device=dev)
    out_m = torch.empty(Ps, dtype=torch.float32, device=dev)
    splits = {"equal": split_ids(Ks, [0.25] * 4, 3), "skewed": split_ids(Ks, [0.70, 0.20, 0.09, 0.01], 4)}
    runs, reps = {}, {}
    for name, ids in splits.items():
        masked = [[w if g == gid else 0 for w, g in zip(ws, ids)] for gid in range(G)]

        def run_a(ids=ids):
            return slab.grouped_mean(ws, ids, G, out=out_g)

        def run_a_fresh(ids=ids, turn=[0]):
            turn[0] += 1
            return slab.grouped_mean(ws_turns[turn[0] % len(ws_turns)], ids, G, out=out_g)

        def run_c(masked=masked):
            return [slab.mean(m, out=out_g[g, :Ps]) for g, m in enumerate(masked)]

        runs.update({f"a_{name}": run_a, f"a_fresh_{name}": run_a_fresh, f"c_{name}": run_c})
        reps.update({f"a_{name}": 10, f"a_fresh_{name}": 10, f"c_{name}": 3})
    runs["b"], reps["b"] = (lambda: slab.mean(ws, out=out_m)), 10

    # ---- pytree
    Kt = 8 if args.small else 128
    tslab = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, device=dev)
    tslab.fill_synthetic(seed=2)
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    wt = rng.randint(1, 501, size=Kt).tolist()
    pairs = list(zip(clients, wt))
    tids = split_ids(Kt, [0.25] * 4, 5)

    def run_d():
        return tu.tree_grouped_mean(pairs, tids, G)

    def run_e():
        sums, totals = [tu.tree_zeros_like(clients[0]) for _ in range(G)], [0] * G
        for (delta, n), g in zip(pairs, tids):
            sums[g] = tu.tree_add(sums[g], tu.tree_weight(delta, n))
            totals[g] += n
        return [tu._eager(tu.tree_inverse_weight(s, W)) if W > 0 else None for s, W in zip(sums, totals)]

    runs.update({"d": run_d, "e": run_e})
    reps.update({"d": 20, "e": 3})
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for x, y in zip(run_d(), run_e())
               for a, b in zip(fedjax_amd.pytree.leaves_of(x), fedjax_amd.pytree.leaves_of(y)))
    a_bits = {}
    for name in splits:
        got = [t["w"].clone() for t in runs[f"a_{name}"]()]
        runs[f"c_{name}"]()
        # (c) adds the +-0 products of the non-members: the same bits unless a sum is exactly zero
        a_bits[name] = all(torch.equal(got[g].view(torch.int32), out_g[g, :Ps].view(torch.int32)) for g in range(G))
    emit({"slab": [Ks, Ps], "a_bitwise_equal_to_masked_passes": a_bits, "groups": G,
          "pytree": [Kt, tslab.num_params], "small": bool(args.small),
          "group_sizes": {k: np.bincount(v, minlength=G).tolist() for k, v in splits.items()},
          "pytree_routes_bitwise_equal": bool(same)})

    for fn in runs.values():  # warm up every leg
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
    for name in splits:
        summary[f"a_over_b_{name}"] = round(med[f"a_{name}"] / med["b"], 4)
        summary[f"a_fresh_over_b_{name}"] = round(med[f"a_fresh_{name}"] / med["b"], 4)
        summary[f"a_over_c_{name}"] = round(med[f"a_{name}"] / med[f"c_{name}"], 4)
        summary[f"a_{name}_read_GBs"] = round(Ks * Ps * 4 / med[f"a_{name}"] / 1e6, 1)
    summary["b_read_GBs"] = round(Ks * Ps * 4 / med["b"] / 1e6, 1)
    summary["d_over_e"] = round(med["d"] / med["e"], 4)
    emit(summary)


if __name__ == "__main__":
    main()
