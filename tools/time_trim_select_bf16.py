"""Times the trimmed mean of a bfloat16 slab by 16-bit rank selection (method="select")
against the routes a bfloat16 user had before it: the float32 selection kernel on the same values,
without and with the float32 copy it needs, and the plain mean of the bfloat16 slab as the floor.

Shapes: 1024 clients x 4 Mi, 128 clients x 4 Mi, and 1024 clients x EMNIST-CNN (8 leaves, 1,206,590
params; configs[1] of BASELINE.json), each as a bfloat16 slab and a float32 slab holding the same
values. Legs of every shape:
  (s) trimmed_mean(0.1, method="select") of the bfloat16 slab: fjagg_trim_select16_dense
  (a) trimmed_mean(0.1, method="select") of the float32 slab: fjagg_trim_select_dense, no copy timed
  (b) the bfloat16 rows' .float() copy and then fjagg_trim_select_dense over it
  (c) the mean with unit weights of the bfloat16 slab: one read of the same bytes

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each and the ratios; the summary
record is appended to --out as well.

usage (MI355X): python tools/time_trim_select_bf16.py [--passes 7] [--small] [--out FILE]
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
TRIM = 0.1


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
    ap.add_argument("--small", action="store_true", help="160 / 16 clients, 64 Ki slabs (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_select_bf16_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    Kb, Ks = (160, 16) if args.small else (1024, 128)
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    runs, reps, res = {}, {}, {"trim": TRIM}

    def legs(name, template, K, n):
        b16 = fedjax_amd.ClientDeltaSlab(template, K, dtype=torch.bfloat16, device=dev).fill_synthetic(seed=len(runs))
        f32 = fedjax_amd.ClientDeltaSlab(template, K, device=dev)
        f32.rows.copy_(b16.rows)  # exact
        t = kernels.trim_count(TRIM, K, select=True)
        scale = float(np.float32(tu._inverse(K - 2 * t)))
        ones = [1] * K
        outs = [torch.empty(b16.num_params, dtype=torch.float32, device=dev) for _ in range(4)]
        runs[name + "_s"] = lambda: b16.trimmed_mean(TRIM, out=outs[0], method="select")
        runs[name + "_a"] = lambda: f32.trimmed_mean(TRIM, out=outs[1], method="select")
        runs[name + "_b"] = lambda: kernels.trim_select_dense(b16.rows.float(), t, scale=scale, out=outs[2], nontemporal=True)
        runs[name + "_c"] = lambda: b16.mean(ones, out=outs[3])
        for leg in "sabc":
            reps[name + "_" + leg] = n
        runs[name + "_s"](), runs[name + "_a"](), runs[name + "_b"]()
        res[name] = [K, b16.num_params]
        res[name + "_same_bits"] = bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
                                        and torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32)))

    legs("big", {"w": np.zeros(Pb, np.float32)}, Kb, 3)
    legs("k128", {"w": np.zeros(Pb, np.float32)}, Ks, 5)
    legs("emnist", tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kb, 5)
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
    summary = dict(res, summary=True, tool="tools/time_trim_select_bf16.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("big", "k128", "emnist"):
        for other in "abc":
            summary[f"{shape}_s_over_{other}"] = round(med[f"{shape}_s"] / med[f"{shape}_{other}"], 4)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
