"""Times the mean folded from DRIVE's transmitted form (drive_mean_aggregator.apply on DriveDelta
clients) against structured_drive_quantizer.apply on the float32 deltas those clients
were encoded from, and the encoder (drive_encode_pytree) once.

Shapes: 1024 clients x one 4 Mi leaf, and 1024 clients x EMNIST-CNN (8 leaves, 1,206,590 params;
configs[1] of BASELINE.json). The legs of every shape are
  (s) drive_mean_aggregator.apply: the sign bits and scales in, K x sum(d / 8 + 8) bytes read
  (f) structured_drive_quantizer.apply: the fused round, rotation and statistics included
  (e) drive_encode_pytree over the K clients, once after a warm-up of one client

Each pass times (s) and (f) of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls: host work of a call (key splits,
tables) is inside the window for both legs. One JSON line per pass and a summary line with the
medians, the spread (max - min over the passes), the ratio s/f and the payload bytes per second of
(s); the summary record is appended to --out as well. Before the timing the two rounds' means are
compared: bit for bit, the largest difference, the number of rotated coordinates that are exactly
zero or NaN (where the forms differ by design) and the clients that have one, and bit for bit again
over the other clients alone.

usage (MI355X): python tools/time_drive_signs.py [--passes 5] [--small] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fedjax_amd import _compress, kernels, pytree, random  # noqa: E402
from fedjax_amd.aggregators import compression as comp  # noqa: E402
from fedjax_amd.aggregators import walsh_hadamard as wh  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}


def per_call_ms(fn, reps):
    s = torch.cuda.current_stream()
    e0, e1 = kernels.Event(), kernels.Event()
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    return e0.elapsed_time(e1) / reps


def carve(row, template):
    """The pytree of ``template``'s shapes as views of the float32 vector ``row``."""
    o = [0]

    def leaf(shape):
        n = int(np.prod(shape))
        o[0] += n
        return row[o[0] - n:o[0]].view(shape)

    def walk(t):
        return {k: walk(v) for k, v in t.items()} if isinstance(t, dict) else leaf(t)

    return walk(template)


def sizes(t):
    return [int(np.prod(t))] if not isinstance(t, dict) else [n for k in sorted(t) for n in sizes(t[k])]


def walk_leaves(t):
    return [x for k in sorted(t) for x in walk_leaves(t[k])] if isinstance(t, dict) else [t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="64 clients, a 64 Ki leaf (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drive_signs_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 64 if args.small else 1024
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    key = random.PRNGKey(0)
    runs, reps, res, summary = {}, {}, {}, {}

    def legs(name, template, n):
        leaf_n = sizes(template)
        P = sum(leaf_n)
        gen = torch.Generator(device=dev).manual_seed(len(runs))
        slab = torch.randn(K, P, generator=gen, device=dev)
        deltas = [carve(slab[k], template) for k in range(K)]
        _, client_keys = comp.drive_round_keys(key, K)
        comp.drive_encode_pytree(deltas[0], client_keys[0])  # warm-up
        enc = []
        summary[name + "_e_ms"] = round(per_call_ms(
            lambda: enc.extend(comp.drive_encode_pytree(d, ck) for d, ck in zip(deltas, client_keys)), 1), 4)
        fused, signs = comp.structured_drive_quantizer(key), comp.drive_mean_aggregator(key)
        runs[name + "_f"] = lambda: fused.apply([(k, d, 1.0) for k, d in enumerate(deltas)], fused.init())
        runs[name + "_s"] = lambda: signs.apply([(k, e, 1.0) for k, e in enumerate(enc)], signs.init())
        reps[name + "_f"] = reps[name + "_s"] = n
        lay = _compress.DriveSignsLayout(leaf_n)
        res[name] = [K, P, K * int((lay.nbytes + 8).sum())]  # clients, params, payload bytes
        a, b = runs[name + "_f"]()[0], runs[name + "_s"]()[0]  # same keys, same deltas: the same mean
        a, b = (torch.cat([x.reshape(-1) for x in walk_leaves(t)]) for t in (a, b))
        summary[name + "_bitwise_equal"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        summary[name + "_max_abs_diff"] = float((a - b).abs().max())
        # The forms differ by design where a rotated coordinate is exactly zero (or NaN): it is sent as + and
        # decodes to +A/b, the fused round has sign(0) = 0. Count those coordinates, and compare the two rounds
        # again over the clients that have none, under the same keys.
        zero = []
        for d, ck in zip(deltas, client_keys):
            y = torch.cat([x.reshape(-1) for x in walk_leaves(wh.structured_rotation_pytree(d, ck)[0])])
            zero.append(((y == 0) | torch.isnan(y)).sum())
        zero = torch.stack(zero).cpu().numpy()
        keep = np.nonzero(zero == 0)[0]
        summary[name + "_zero_rotated_coords"] = int(zero.sum())
        summary[name + "_clients_with_one"] = int(K - keep.size)
        _, rows = comp._rows([deltas[k] for k in keep])
        leaf_keys = random.split_many(client_keys, len(leaf_n))[keep]
        w, scale = np.ones(keep.size, np.float32), float(np.float32(1.0 / keep.size))
        a, b = (torch.empty(P, dtype=torch.float32, device=dev) for _ in range(2))
        _compress.drive_mean(rows, leaf_keys, w, scale, a)
        _compress.drive_signs_mean([pytree.leaves_of(enc[k].signs) for k in keep],
                                   torch.stack([enc[k].scales for k in keep]), leaf_keys, w, scale, leaf_n, b)
        summary[name + "_bitwise_equal_without_them"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))

    legs("big", {"w": (Pb,)}, 12)  # windows of 0.3 - 0.6 s at the full size
    legs("emnist", EMNIST, 20)
    print(json.dumps(res), flush=True)

    for fn in runs.values():  # warm up every leg of every shape
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
    summary = dict(res, summary=True, tool="tools/time_drive_signs.py", passes=args.passes, small=bool(args.small),
                   **summary)
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("big", "emnist"):
        summary[shape + "_s_over_f"] = round(med[shape + "_s"] / med[shape + "_f"], 4)
        summary[shape + "_s_GBps"] = round(res[shape][2] / med[shape + "_s"] / 1e6, 2)  # payload bytes read per second
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
