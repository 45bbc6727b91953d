"""Times the mean folded from top-k clients' (index, value) lists (SparseSlab.mean)
against the dense routes over the same deltas and against its byte floor.

Two slabs of Gaussian deltas, 1024 clients x 4 Mi float32 (prefix s) and 1024 clients x EMNIST-CNN
(8 leaves, 1,206,590 float32 params; configs[1] of BASELINE.json; prefix t), k = 1 % and 10 %
(suffix 1 / 10):
  (f) SparseSlab.mean: fjcomp_sparse_fold, 8 * nnz bytes read
  (e) ClientDeltaSlab.topk_encode: the select, the compaction and the table upload, one host
      synchronisation inside (timed with the host clock around a synchronised call)
  (a) ClientDeltaSlab.topk_mean of the dense slab: four reads of K * P * 4 bytes
  (c) ClientDeltaSlab.mean of the dense slab: one read
Each pass times every leg in turn (interleaved), after a warm-up of every shape, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line with
the medians, the spread (max - min) of each, the ratios and, for (f), the rate 8 * nnz / time
against --hbm-gbs (the byte floor's rate): reported, not gated. --out appends the lines to a file
(profiles/sparse_mean_timing.jsonl).

usage (MI355X): python tools/time_sparse_mean.py [--passes 7] [--small] [--hbm-gbs 8000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fedjax_amd  # noqa: E402
from fedjax_amd import kernels  # noqa: E402

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


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def gaussian_slab(template, K, dev, seed):
    slab = fedjax_amd.ClientDeltaSlab(template, K, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for k in range(K):  # row by row: no second K x P tensor
        slab.rows[k].copy_(torch.randn(slab.num_params, generator=g, device=dev) * 0.01)
    return slab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="16 clients x 64 Ki (a rehearsal, not a measurement)")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the byte floor is taken at")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    K, Ps = (16, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slabs = {"s": gaussian_slab({"w": np.zeros(Ps, np.float32)}, K, dev, 0),
             "t": gaussian_slab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), K, dev, 2)}
    ones = [1] * K
    runs, reps, timer, nnz, same = {}, {}, {}, {}, {}
    for p, slab in slabs.items():
        out = torch.empty(slab.num_params, dtype=torch.float32, device=dev)
        runs[p + "c"], reps[p + "c"] = (lambda s=slab, o=out: s.mean(ones, out=o)), 5
        for pct, frac in ((1, 0.01), (10, 0.1)):
            sparse = slab.topk_encode(frac)
            nnz[f"{p}{pct}"] = sparse.nnz
            flat = lambda t: torch.cat([x.reshape(-1) for x in fedjax_amd.pytree.leaves_of(t)])
            same[f"{p}{pct}"] = bool(torch.equal(flat(sparse.mean(ones)).view(torch.int32),
                                                 flat(slab.topk_mean(ones, frac).mean).view(torch.int32)))
            runs[f"{p}f{pct}"], reps[f"{p}f{pct}"] = (lambda s=sparse, o=out: s.mean(ones, o)), 10
            runs[f"{p}e{pct}"], reps[f"{p}e{pct}"] = (lambda s=slab, f=frac: s.topk_encode(f)), 2
            runs[f"{p}a{pct}"], reps[f"{p}a{pct}"] = (lambda s=slab, f=frac, o=out: s.topk_mean(ones, f, out=o)), 2
            timer[f"{p}e{pct}"] = host_ms
    emit({"clients": K, "params": {p: s.num_params for p, s in slabs.items()}, "nnz": nnz,
          "wave_tile": kernels.SPARSE_WAVE_TILE, "group_tile": kernels.SPARSE_GROUP_TILE,
          "sparse_and_masked_fold_same_bits": same, "hbm_gbs": args.hbm_gbs})

    for fn in runs.values():  # warm up every shape
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for i in range(args.passes):
        row = {"pass": i}
        for name, fn in runs.items():
            ms = timer.get(name, per_call_ms)(fn, reps[name])
            times[name].append(ms)
            row[name + "_ms"] = round(ms, 4)
        emit(row)
    med = {k: float(np.median(v)) for k, v in times.items()}
    summary = {"summary": True, "passes": args.passes}
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for p in slabs:
        for pct in (1, 10):
            f = med[f"{p}f{pct}"]
            floor_ms = nnz[f"{p}{pct}"] * 8 / (args.hbm_gbs * 1e6)
            summary[f"{p}f{pct}_read_GBs"] = round(nnz[f"{p}{pct}"] * 8 / f / 1e6, 1)
            summary[f"{p}f{pct}_floor_ms"] = round(floor_ms, 4)
            summary[f"{p}f{pct}_over_floor"] = round(f / floor_ms, 2)
            summary[f"{p}a{pct}_over_f{pct}"] = round(med[f"{p}a{pct}"] / f, 2)
            summary[f"{p}c_over_f{pct}"] = round(med[p + "c"] / f, 2)
            summary[f"{p}e{pct}_over_a{pct}"] = round(med[f"{p}e{pct}"] / med[f"{p}a{pct}"], 2)
    emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
