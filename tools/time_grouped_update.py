"""Times one HypCluster round's server side — the per-cluster means and each cluster's server
step (fedjax/algorithms/hyp_cluster.py:107-128) — as ONE launch against the grouped mean alone
and against the two-step route a user had before.

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py), G = 4 equal groups (clients
assigned by a seeded shuffle), Adam:
  (a) server.fused_grouped_mean_update: the fold with every cluster's step in its epilogue
  (b) ClientDeltaSlab.grouped_mean alone: the floor (no step at all)
  (c) ClientDeltaSlab.grouped_mean, then server.fused_tree_mean_update([(mean_g, 1.0)], ...)
      per cluster: the G means go to HBM and come back, G more launches and host calls.
Pytree, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json), every (client, leaf) its own device tensor, G = 4 equal groups, Adam:
  (a) server.fused_tree_grouped_mean_update  (b) tree_util.tree_grouped_mean  (c) as above.
Every call of every leg takes other weights than the call before it, as a real round does, so
every leg builds and uploads its tables per call.

Each pass times every leg in turn (interleaved), after a warm-up of every leg, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line
with the medians, the spread (max - min over passes) of each and the ratios (a)/(b), (a)/(c);
everything is appended to profiles/grouped_update_timing.jsonl as well.

usage (MI355X): python tools/time_grouped_update.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import kernels, pytree, server, tree_util as tu  # noqa: E402

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


def split_ids(K, seed):
    return np.random.RandomState(seed).permutation(np.repeat(np.arange(G), K // G))


def turns(ws):
    """Weights that differ from one call to the next (rotations of ws)."""
    rot, i = [ws[j:] + ws[:j] for j in range(4)], [0]

    def nxt():
        i[0] += 1
        return rot[i[0] % len(rot)]
    return nxt


def two_step(means, opt, params, states):
    """The route before the fused kernel: one fused step per cluster on a one-client mean of
    weight 1 (the identity), reading the mean back from HBM."""
    return [st if mean is None else server.fused_tree_mean_update([(mean, 1.0)], opt, p, st)
            for mean, p, st in zip(means, params, states)]


def flat_bits(trees):
    return torch.cat([x.reshape(-1).view(torch.int32) for t in trees for x in pytree.leaves_of(t)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_update_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    sink = open(args.out, "a")
    opt = server.adam(10 ** -2.5, b1=0.9, b2=0.999, eps=1e-4)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    # ---- slab
    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Ps, np.float32)}, Ks, device=dev).fill_synthetic(seed=0)
    ws = rng.randint(1, 501, size=Ks).tolist()
    ids = split_ids(Ks, 3)
    out_g = torch.empty(G, slab.row_stride, dtype=torch.float32, device=dev)

    def slab_state():
        params = torch.zeros(G, Ps, device=dev)
        return params, [opt.init(params[g]) for g in range(G)]

    def slab_c(params, states, w):
        means = slab.grouped_mean(w, ids, G, out=out_g)
        trees = [slab.unflatten(params[g]) for g in range(G)]
        sts = [dict(st, m=slab.unflatten(st["m"]), v=slab.unflatten(st["v"])) for st in states]
        new = two_step(means, opt, trees, sts)
        return [dict(st, count=n["count"]) for st, n in zip(states, new)]

    (pa, sa), (pc, sc) = slab_state(), slab_state()
    sa, _ = server.fused_grouped_mean_update(slab, ws, ids, G, opt, pa, sa)
    sc = slab_c(pc, sc, ws)
    slab_same = bool(torch.equal(pa.view(torch.int32), pc.view(torch.int32)) and all(
        torch.equal(a[k].view(torch.int32), c[k].view(torch.int32)) for a, c in zip(sa, sc) for k in ("m", "v")))
    box = {"sa": sa, "sc": sc}
    wa, wb, wc = turns(ws), turns(ws), turns(ws)

    def run_a_slab():
        box["sa"], _ = server.fused_grouped_mean_update(slab, wa(), ids, G, opt, pa, box["sa"])

    def run_b_slab():
        return slab.grouped_mean(wb(), ids, G, out=out_g)

    def run_c_slab():
        box["sc"] = slab_c(pc, box["sc"], wc())

    # ---- pytree
    Kt = 8 if args.small else 128
    tslab = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, device=dev)
    tslab.fill_synthetic(seed=2)
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    wt = rng.randint(1, 501, size=Kt).tolist()
    tids = split_ids(Kt, 5)

    def tree_state():
        params = [tmap(lambda v: torch.zeros_like(v), clients[0]) for _ in range(G)]
        return params, [opt.init(p) for p in params]

    (ta, tsa), (tc, tsc) = tree_state(), tree_state()
    tsa, _ = server.fused_tree_grouped_mean_update(list(zip(clients, wt)), tids, opt, ta, tsa)
    tsc = two_step(tu.tree_grouped_mean(list(zip(clients, wt)), tids, G), opt, tc, tsc)
    tree_same = bool(torch.equal(flat_bits(ta), flat_bits(tc)) and all(
        torch.equal(flat_bits([a[k]]), flat_bits([c[k]])) for a, c in zip(tsa, tsc) for k in ("m", "v")))
    box.update({"tsa": tsa, "tsc": tsc})
    ua, ub, uc = turns(wt), turns(wt), turns(wt)

    def run_a_tree():
        box["tsa"], _ = server.fused_tree_grouped_mean_update(list(zip(clients, ua())), tids, opt, ta, box["tsa"])

    def run_b_tree():
        return tu.tree_grouped_mean(list(zip(clients, ub())), tids, G)

    def run_c_tree():
        box["tsc"] = two_step(tu.tree_grouped_mean(list(zip(clients, uc())), tids, G), opt, tc, box["tsc"])

    runs = {"a_slab": run_a_slab, "b_slab": run_b_slab, "c_slab": run_c_slab,
            "a_tree": run_a_tree, "b_tree": run_b_tree, "c_tree": run_c_tree}
    reps = {"a_slab": 10, "b_slab": 10, "c_slab": 10, "a_tree": 20, "b_tree": 20, "c_tree": 20}
    # what the algorithm must move: every member row once, and per cluster params, m, v in and out
    fold_bytes, state_bytes = Ks * Ps * 4, G * Ps * 4 * 6
    emit({"slab": [Ks, Ps], "groups": G, "pytree": [Kt, tslab.num_params], "small": bool(args.small), "rule": "adam",
          "a_bitwise_equal_to_two_step_route": {"slab": slab_same, "pytree": tree_same},
          "slab_fold_bytes": fold_bytes, "slab_state_bytes": state_bytes})

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
    for route in ("slab", "tree"):
        summary[f"a_over_b_{route}"] = round(med[f"a_{route}"] / med[f"b_{route}"], 4)
        summary[f"a_over_c_{route}"] = round(med[f"a_{route}"] / med[f"c_{route}"], 4)
    summary["a_slab_GBs"] = round((fold_bytes + state_bytes) / med["a_slab"] / 1e6, 1)
    summary["b_slab_GBs"] = round((fold_bytes + G * Ps * 4) / med["b_slab"] / 1e6, 1)
    # the expectations of DESIGN §3i, confirmed or refuted by this run
    summary["tree_a_below_c_by_more_than_c_spread"] = bool(med["c_tree"] - med["a_tree"] > spread["c_tree"])
    extra_ms = med["b_slab"] * (state_bytes - G * Ps * 4) / (fold_bytes + G * Ps * 4)  # at (b)'s own rate
    summary["slab_extra_state_ms_at_b_rate"] = round(extra_ms, 4)
    summary["slab_a_within_b_spread_plus_state_traffic"] = bool(
        med["a_slab"] <= med["b_slab"] + spread["b_slab"] + extra_ms)
    emit(summary)


if __name__ == "__main__":
    main()
