"""Times centered clipping against the clipped mean on the same slab and against a torch route.

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py):
  (a) ClientDeltaSlab.centered_clip, one iteration
  (b) the same with three iterations
  (c) ClientDeltaSlab.clipped_mean([1] * K, tau) on the same slab: the yardstick, two passes over
      the same bytes on the same build
  (e) a torch route: (rows - v).norm(dim=1), the factors, v + ((rows - v) * c[:, None]).mean(0)
      (skipped where its K x P temporaries do not fit: --no-torch)
Slab and pytrees, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json):
  (a), (c), (e) on the slab, as ta / tc / te
  (d) tree_util.tree_centered_clip over separate pytrees, every (client, leaf) its own tensor

Each pass times every leg in turn (interleaved), after a warm-up of every shape, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line
with the medians, the spread (max - min) of each and the ratios a/c and b/(3c): reported, not
gated. --out appends the lines to a file (profiles/centered_clip_timing.jsonl).

usage (MI355X): python tools/time_centered_clip.py [--passes 7] [--small] [--no-torch] [--out FILE]
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


def torch_route(rows, v, tau):
    d = rows - v
    n = d.norm(dim=1)
    c = torch.clamp(tau / n, max=1.0)
    return v + (d * c[:, None]).mean(0)


def scaled_slab(template, K, dev, seed):
    """Client k scaled by 2**((k % 5) - 2); tau = the median distance from the centre, so about
    half the clients are clipped. The centre is a small synthetic vector."""
    slab = fedjax_amd.ClientDeltaSlab(template, K, device=dev).fill_synthetic(seed=seed)
    slab.rows.mul_(torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], device=dev)[:, None])
    centre = torch.empty(1, slab.num_params, dtype=torch.float32, device=dev)
    kernels.fill_synth(centre, seed=seed + 100, amp=0.001)
    return slab, centre[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch legs")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab, vs = scaled_slab({"w": np.zeros(Ps, np.float32)}, Ks, dev, 0)
    taus = float(slab.centered_clip(1.0, vs).distances[0].median().item())
    out_a, out_b, out_c = (torch.empty(Ps, dtype=torch.float32, device=dev) for _ in range(3))
    ones = [1] * Ks

    Kt = 8 if args.small else 128
    tslab, vt = scaled_slab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, dev, 2)
    taut = float(tslab.centered_clip(1.0, vt).distances[0].median().item())
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    vtree = tmap(lambda v: v.clone(), tslab.unflatten(vt))
    out_ta, out_tc = (torch.empty(tslab.num_params, dtype=torch.float32, device=dev) for _ in range(2))
    tones = [1] * Kt

    runs = {
        "a": lambda: slab.centered_clip(taus, vs, out=out_a),
        "b": lambda: slab.centered_clip(taus, vs, iterations=3, out=out_b),
        "c": lambda: slab.clipped_mean(ones, taus, out=out_c),
        "ta": lambda: tslab.centered_clip(taut, vt, out=out_ta),
        "tc": lambda: tslab.clipped_mean(tones, taut, out=out_tc),
        "d": lambda: tu.tree_centered_clip(clients, taut, vtree),
    }
    reps = {"a": 10, "b": 4, "c": 10, "ta": 20, "tc": 20, "d": 20, "e": 3, "te": 10}
    if not args.no_torch:
        runs["e"] = lambda: torch_route(slab.rows, vs, taus)
        runs["te"] = lambda: torch_route(tslab.rows, vt, taut)

    got_a, got_d = runs["a"](), runs["d"]()
    res = {"slab": [Ks, Ps], "pytree": [Kt, tslab.num_params], "tau_slab": taus, "tau_pytree": taut,
           "slab_clipped": int((got_a.factors[0] < 1).sum().item()),
           "pytree_clipped": int((got_d.factors[0] < 1).sum().item()),
           "slab_and_tree_same_bits": bool(torch.equal(
               torch.cat([x.reshape(-1) for x in fedjax_amd.pytree.leaves_of(got_d.center)]).view(torch.int32),
               torch.cat([x.reshape(-1) for x in fedjax_amd.pytree.leaves_of(runs["ta"]().center)]).view(torch.int32)))}
    if not args.no_torch:
        res["torch_route_max_abs_diff"] = float((runs["te"]() - out_ta).abs().max().item())
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
    summary["a_over_c"] = round(med["a"] / med["c"], 4)
    summary["b_over_3c"] = round(med["b"] / (3 * med["c"]), 4)
    summary["ta_over_tc"] = round(med["ta"] / med["tc"], 4)
    summary["d_over_ta"] = round(med["d"] / med["ta"], 4)
    if "e" in runs:
        summary["e_over_a"] = round(med["e"] / med["a"], 4)
        summary["te_over_ta"] = round(med["te"] / med["ta"], 4)
    summary["a_read_GBs"] = round(2 * Ks * Ps * 4 / med["a"] / 1e6, 1)
    summary["c_read_GBs"] = round(2 * Ks * Ps * 4 / med["c"] / 1e6, 1)
    emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
