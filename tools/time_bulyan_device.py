"""Times Bulyan rounds with the selection on the host (select="host": Gram, the copy to the host,
numpy, the second stage with its row table in the kernel arguments) and on the device
(select="device": Gram, fjagg_bulyan_select, the second stage from device tables, no host visit),
the select entry alone, and the two second stages against each other.

Shapes: 160 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json), f = 16, as a slab and as separate pytrees; 128 clients x 4 Mi float32 as a slab,
f = 16. Alone: fjagg_bulyan_select on the Gram of 160 clients (f = 16) and of 252 (f = 62), and
fjagg_meamed_dense_dev against fjagg_meamed_dense over the same 96 rows of the 128 x 4 Mi slab.

Each pass times every leg in turn (the host and device routes of a leg back to back:
interleaved), after a warm-up of all of them, with the fence-free kernels.Event around
back-to-back calls; the host route's wait for the device between its two passes is inside its
time. For the device route the host's own time per call (a wall clock around the calls, before
the synchronise) is recorded too. One JSON line per pass and a summary line with the medians and
the spread (max - min over the passes) of each leg; the summary is appended to --out.

usage (MI355X): python tools/time_bulyan_device.py [--passes 7] [--small] [--out FILE]
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
    ap.add_argument("--small", action="store_true", help="23 clients, 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bulyan_device_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    Ke, Kb, f = (23, 23, 3) if args.small else (160, 128, 16)
    runs, reps = {}, {}
    res = {"num_byzantine": f}

    def legs(name, bulyan, n):
        for select in ("host", "device"):
            runs[f"{name}_{select}"] = lambda s=select: bulyan(f, select=s)
            reps[f"{name}_{select}"] = n

    es = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Ke, device=dev).fill_synthetic(seed=2)
    legs("emnist_slab", es.bulyan, 10)
    res["emnist"] = [Ke, es.num_params]
    clients = [tmap(lambda v: v.clone(), es.client(k)) for k in range(Ke)]
    legs("emnist_tree", lambda *a, **kw: tu.tree_bulyan(clients, *a, **kw), 10)
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    bs = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Pb, np.float32)}, Kb, device=dev).fill_synthetic(seed=0)
    legs("big_slab", bs.bulyan, 4)
    res["big"] = [Kb, Pb]

    # the select entry alone
    K2, f2 = (43, 5) if args.small else (252, 62)
    wide = fedjax_amd.ClientDeltaSlab({"w": np.zeros(4096, np.float32)}, K2, device=dev).fill_synthetic(seed=5)
    for name, G, ff in ((f"select_K{Ke}", es.gram(), f), (f"select_K{K2}", wide.gram(), f2)):
        runs[name] = lambda G=G, ff=ff: kernels.bulyan_select_device(G, ff)
        reps[name] = 20
    res["select_alone"] = {f"select_K{Ke}": [Ke, f], f"select_K{K2}": [K2, f2]}

    # the two second stages over the same rows of the big slab: what the selection of a round chose
    _, count, _, tables = kernels.bulyan_select_device(bs.gram(), f)
    M, keep = int(count), int(tables.keep)
    rows = tables.rows[:M].cpu().numpy()
    out_a = torch.empty(Pb, dtype=torch.float32, device=dev)
    out_b = torch.empty(Pb, dtype=torch.float32, device=dev)
    nt = M * Pb * 4 >= tu.NONTEMPORAL_MIN_BYTES
    runs["meamed_args"] = lambda: kernels.meamed_dense(bs.rows, keep, rows, scale=float(np.float32(1.0 / keep)),
                                                       out=out_a, nontemporal=nt)
    runs["meamed_dev"] = lambda: kernels.meamed_dense_device(bs.rows, tables, out=out_b, nontemporal=nt)
    reps["meamed_args"] = reps["meamed_dev"] = 6
    res["second_stage"] = {"rows": M, "keep": keep, "columns": Pb}
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))  # the same bits, or the times mean nothing
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
    summary = dict(res, summary=True, tool="tools/time_bulyan_device.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(float(np.median(times[k])), 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
        if not k.endswith("_host"):
            summary[k + "_host_wall_ms"] = round(float(np.median(hosts[k])), 4)
    for shape in ("emnist_slab", "emnist_tree", "big_slab"):
        summary[f"{shape}_device_over_host"] = round(summary[f"{shape}_device_ms"] / summary[f"{shape}_host_ms"], 4)
    summary["meamed_dev_over_args"] = round(summary["meamed_dev_ms"] / summary["meamed_args_ms"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f_out:
        f_out.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
