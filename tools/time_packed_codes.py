"""Times the mean folded from 1-, 2- and 4-bit packed level codes (CodeSlab(bits=b).mean, DESIGN
§3z) against the 8-bit fold of the same codes and the float32 fold of the same K x P, and the
packed encoder against the 8-bit one.

Shapes: 1024 clients x 4 Mi, and 1024 clients x EMNIST-CNN (8 leaves, 1,206,590 params; configs[1]
of BASELINE.json). For num_levels 16, 4 and 2 (4, 2 and 1 bits) the legs of every shape are
  (p)  CodeSlab(bits=b).mean: fjcomp_codes_fold_packed, K x P x b / 8 bytes read
  (c)  CodeSlab(bits=8).mean of the same codes: fjcomp_codes_fold, K x P bytes read
  (ep) CodeSlab(bits=b).encode_from: the statistics pass and fjcomp_encode_uniform_packed
  (e)  CodeSlab(bits=8).encode_from: the statistics pass and fjcomp_encode_uniform
and once per shape
  (m)  ClientDeltaSlab.mean of the float32 slab the codes were encoded from: 4 K x P bytes read

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each and the ratios p/c, p/m and
ep/e; the summary record is appended to --out as well.

usage (MI355X): python tools/time_packed_codes.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import kernels, random  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}
FORMS = [(16, 4), (4, 2), (2, 1)]  # (num_levels, bits)


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
    ap.add_argument("--small", action="store_true", help="64 clients, a 64 Ki slab (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_codes_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 64 if args.small else 1024
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    key = random.PRNGKey(0)
    runs, reps, res = {}, {}, {}

    def legs(name, template, n):
        f32 = fedjax_amd.ClientDeltaSlab(template, K, device=dev).fill_synthetic(seed=len(runs))
        ones = [1.0] * K
        out_m = torch.empty(f32.num_params, dtype=torch.float32, device=dev)
        runs[name + "_m"], reps[name + "_m"] = (lambda: f32.mean(ones, out=out_m)), n
        for levels, bits in FORMS:
            for leg, b in (("p", bits), ("c", 8)):
                slab = fedjax_amd.CodeSlab(template, K, levels, bits=b, device=dev).encode_from(f32, key)
                out = torch.empty(f32.num_params, dtype=torch.float32, device=dev)
                tag, enc = f"{name}_{bits}b_", "ep" if leg == "p" else "e"
                runs[tag + leg] = lambda slab=slab, out=out: slab.mean(ones, out=out)
                runs[tag + enc] = lambda slab=slab: slab.encode_from(f32, key)
                reps[tag + leg], reps[tag + enc] = n, 2
        res[name] = [K, f32.num_params]

    legs("big", {"w": np.zeros(Pb, np.float32)}, 5)
    legs("emnist", tmap(lambda s: np.zeros(s, np.float32), EMNIST), 10)
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every leg of every shape
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
    summary = dict(res, summary=True, tool="tools/time_packed_codes.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("big", "emnist"):
        for _, bits in FORMS:
            tag = f"{shape}_{bits}b_"
            summary[tag + "p_over_c"] = round(med[tag + "p"] / med[tag + "c"], 4)
            summary[tag + "p_over_m"] = round(med[tag + "p"] / med[shape + "_m"], 4)
            summary[tag + "ep_over_e"] = round(med[tag + "ep"] / med[tag + "e"], 4)
            kp = res[shape][0] * res[shape][1]
            summary[tag + "p_GBps"] = round(kp * bits / 8 / med[tag + "p"] / 1e6, 1)  # packed bytes read per second
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
