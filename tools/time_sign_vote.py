"""Times the sign-bit majority vote (fjcomp_sign_vote) against the 1-bit codes fold of
the same bit volume, the float32 fold of the same K x P and the byte floor, and the sign encoder
(fjcomp_sign_pack) against the 1-bit uniform encoder.

Shapes: 1024 clients x one 4 Mi leaf, and 1024 clients x EMNIST-CNN (8 leaves, 1,206,590 params;
configs[1] of BASELINE.json). The bit rows the vote reads ARE the rows of a CodeSlab(2, bits=1)
encoded from the float32 slab: the same bytes at the same addresses as leg (c). Legs of a shape:
  (vs) k_sign_vote, sign mode, tables uploaded beforehand: K x P / 8 bytes read, 4 P written
  (vm) k_sign_vote, mean mode
  (c)  CodeSlab(2, bits=1).mean: fjcomp_codes_fold_packed over the same rows
  (m)  ClientDeltaSlab.mean of the float32 slab: 4 K x P bytes read
  (sp) k_sign_pack over the K x L float32 rows, tables uploaded beforehand
  (ep) CodeSlab(2, bits=1).encode_from: the statistics pass and fjcomp_encode_uniform_packed<1>
and floor_ms = (K P / 8 + 4 P) bytes / 8 TB/s, computed, not measured.

Each pass times every leg of every shape in turn (interleaved), after a warm-up of all of them,
with the fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary
line with the medians, the spread (max - min over the passes) of each and the ratios vs/c, vs/m,
vs/floor and sp/ep; the summary record is appended to --out as well.

usage (MI355X): python tools/time_sign_vote.py [--passes 7] [--small] [--out FILE]
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
from fedjax_amd import _compress, _lib, kernels, random  # noqa: E402

EMNIST = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 64)},
          "linear": {"b": (128,), "w": (9216, 128)}, "linear_1": {"b": (62,), "w": (128, 62)}}
PEAK_BYTES_PER_MS = 8e9  # 8 TB/s


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign_vote_timing.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_sign_vote.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    K = 64 if args.small else 1024
    Pb = 64 * 1024 if args.small else 4 * 1024 * 1024
    key = random.PRNGKey(0)
    runs, reps, res, keep = {}, {}, {}, []

    def legs(name, template, n):
        f32 = fedjax_amd.ClientDeltaSlab(template, K, device=dev).fill_synthetic(seed=len(runs))
        codes = fedjax_amd.CodeSlab(template, K, 2, bits=1, device=dev).encode_from(f32, key)
        ones = [1.0] * K
        P, sizes = f32.num_params, np.array(f32.sizes, dtype=np.int64)
        out_m, out_c, out_v = (torch.empty(P, dtype=torch.float32, device=dev) for _ in range(3))
        vote = _compress.SignVote(codes._code_ptrs(), sizes, (out_v.data_ptr() + 4 * f32.offsets[:-1]).astype(np.uint64),
                                  dev)
        packed = torch.empty_like(codes.storage)
        rows = np.arange(K, dtype=np.int64)[:, None]
        in_ptrs = (f32.storage.data_ptr() + 4 * (rows * f32.row_stride + f32.offsets[None, :-1])).astype(np.uint64)
        out_ptrs = (packed.data_ptr() + rows * codes.row_stride + codes.code_offsets[None, :-1]).astype(np.uint64)
        pack = _compress.SignPack(in_ptrs.reshape(-1), np.tile(sizes, K), out_ptrs.reshape(-1), dev)
        keep.extend([f32, codes, packed, out_m, out_c, out_v])
        runs[name + "_vs"], reps[name + "_vs"] = (lambda: vote.launch(_lib.VOTE_SIGN)), n
        runs[name + "_vm"], reps[name + "_vm"] = (lambda: vote.launch(_lib.VOTE_MEAN)), n
        runs[name + "_c"], reps[name + "_c"] = (lambda: codes.mean(ones, out=out_c)), n
        runs[name + "_m"], reps[name + "_m"] = (lambda: f32.mean(ones, out=out_m)), n
        runs[name + "_sp"], reps[name + "_sp"] = pack.launch, 2
        runs[name + "_ep"], reps[name + "_ep"] = (lambda: codes.encode_from(f32, key)), 2
        res[name] = [K, P]
        # the timed vote computes what numpy computes from the same bytes (first 4096 coordinates of leaf 0)
        vote.launch(_lib.VOTE_MEAN)
        nb = min(512, (int(sizes[0]) + 7) // 8)
        b = codes.storage[:, :nb].cpu().numpy()
        c = np.unpackbits(b, axis=1, bitorder="little").sum(axis=0, dtype=np.int64)[:min(int(sizes[0]), 8 * nb)]
        want = (K - 2 * c).astype(np.float32) * np.float32(1.0 / K)
        if not np.array_equal(out_v[:want.size].cpu().numpy(), want):
            sys.exit(f"{name}: the vote differs from the numpy count")

    legs("big", {"w": np.zeros(Pb, np.float32)}, 10)
    legs("emnist", tmap(lambda s: np.zeros(s, np.float32), EMNIST), 20)
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
    summary = dict(res, summary=True, tool="tools/time_sign_vote.py", passes=args.passes, small=bool(args.small))
    for k in runs:
        summary[k + "_ms"] = round(med[k], 4)
        summary[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
    for shape in ("big", "emnist"):
        Ks, P = res[shape]
        floor = (Ks * P / 8 + 4 * P) / PEAK_BYTES_PER_MS
        summary[shape + "_floor_ms"] = round(floor, 4)
        summary[shape + "_vs_over_c"] = round(med[shape + "_vs"] / med[shape + "_c"], 4)
        summary[shape + "_vm_over_c"] = round(med[shape + "_vm"] / med[shape + "_c"], 4)
        summary[shape + "_vs_over_m"] = round(med[shape + "_vs"] / med[shape + "_m"], 4)
        summary[shape + "_vs_over_floor"] = round(med[shape + "_vs"] / floor, 4)
        summary[shape + "_sp_over_ep"] = round(med[shape + "_sp"] / med[shape + "_ep"], 4)
        summary[shape + "_vs_GBps"] = round((Ks * P / 8 + 4 * P) / med[shape + "_vs"] / 1e6, 1)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
