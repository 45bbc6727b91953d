"""Times one clipped round's server side — the clipped weighted mean and the server step on it
(fedjax/algorithms/mime_lite.py:131-149, then :162-167) — as ONE fold against the clipped mean
alone and against the two-step route a user had before.

Slab, 1024 clients x 4 Mi float32 (the c3 shape of bench.py), Adam, half the clients clipped
(max_norm = the median norm):
  (a) server.fused_clipped_mean_update: the clipped fold with the step in its epilogue
  (b) ClientDeltaSlab.clipped_mean alone: the floor (no step at all)
  (c) ClientDeltaSlab.clipped_mean, then server.fused_tree_mean_update([(mean, 1.0)], ...):
      the mean goes to HBM and comes back, one more launch, plan and upload.
Pytree, 128 clients x EMNIST-CNN (8 leaves, 1,206,590 float32 params; configs[1] of
BASELINE.json), every (client, leaf) its own device tensor, Adam, half the clients clipped:
  (a) server.fused_tree_clipped_mean_update  (b) tree_util.tree_clipped_mean  (c) as above.
Every call of every leg takes other weights than the call before it, as a real round does.

Each pass times every leg in turn (interleaved), after a warm-up of every leg, with the
fence-free kernels.Event around back-to-back calls. One JSON line per pass and a summary line
with the medians, the spread (max - min over passes) of each and the ratios (a)/(b), (a)/(c);
everything is appended to profiles/clipped_update_timing.jsonl as well.

usage (MI355X): python tools/time_clipped_update.py [--passes 7] [--small] [--out FILE]
                python tools/time_clipped_update.py --once   (one call of every leg: for a kernel trace)
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


def turns(ws):
    """Weights that differ from one call to the next (rotations of ws)."""
    rot, i = [ws[j:] + ws[:j] for j in range(4)], [0]

    def nxt():
        i[0] += 1
        return rot[i[0] % len(rot)]
    return nxt


def spread_rows(slab, K):
    """Scale client k's row by 2**((k % 5) - 2) so the norms differ and the median clips half."""
    f = torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], dtype=torch.float32, device=slab.storage.device)
    slab.storage.mul_(f[:, None])


def flat_bits(trees):
    return torch.cat([x.reshape(-1).view(torch.int32) for t in trees for x in pytree.leaves_of(t)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--small", action="store_true",
                    help="64 x 64 Ki slab and 8 clients (a rehearsal, not a measurement)")
    ap.add_argument("--once", action="store_true", help="one call of every leg after the warm-up, no timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clipped_update_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    opt = server.adam(10 ** -2.5, b1=0.9, b2=0.999, eps=1e-4)

    # ---- slab
    Ks, Ps = (64, 64 * 1024) if args.small else (1024, 4 * 1024 * 1024)
    slab = fedjax_amd.ClientDeltaSlab({"w": np.zeros(Ps, np.float32)}, Ks, device=dev).fill_synthetic(seed=0)
    spread_rows(slab, Ks)
    ws = rng.randint(1, 501, size=Ks).tolist()
    Cs = float(torch.median(slab.l2_norms()).item())
    out_m = torch.empty(Ps, dtype=torch.float32, device=dev)

    def slab_state():
        params = torch.zeros(Ps, device=dev)
        return params, opt.init(params)

    def slab_c(params, state, w):
        cm = slab.clipped_mean(w, Cs, out=out_m)
        st = dict(state, m=slab.unflatten(state["m"]), v=slab.unflatten(state["v"]))
        new = server.fused_tree_mean_update([(cm.mean, 1.0)], opt, slab.unflatten(params), st)
        return dict(state, count=new["count"]), cm

    (pa, sa), (pc, sc) = slab_state(), slab_state()
    ga = server.fused_clipped_mean_update(slab, ws, Cs, opt, pa, sa)
    sa = ga.state
    sc, cm = slab_c(pc, sc, ws)
    slab_same = bool(torch.equal(pa.view(torch.int32), pc.view(torch.int32)) and all(
        torch.equal(sa[k].view(torch.int32), sc[k].view(torch.int32)) for k in ("m", "v")) and torch.equal(
        ga.clipped_norms.view(torch.int32), cm.clipped_norms.view(torch.int32)))
    slab_clipped = int(ga.clipped.sum().item())
    box = {"sa": sa, "sc": sc}
    wa, wb, wc = turns(ws), turns(ws), turns(ws)

    def run_a_slab():
        box["sa"] = server.fused_clipped_mean_update(slab, wa(), Cs, opt, pa, box["sa"]).state

    def run_b_slab():
        return slab.clipped_mean(wb(), Cs, out=out_m)

    def run_c_slab():
        box["sc"], _ = slab_c(pc, box["sc"], wc())

    # ---- pytree
    Kt = 8 if args.small else 128
    tslab = fedjax_amd.ClientDeltaSlab(tmap(lambda s: np.zeros(s, np.float32), EMNIST), Kt, device=dev)
    tslab.fill_synthetic(seed=2)
    spread_rows(tslab, Kt)
    clients = [tmap(lambda v: v.clone(), tslab.client(k)) for k in range(Kt)]
    wt = rng.randint(1, 501, size=Kt).tolist()
    Ct = float(torch.median(tslab.l2_norms()).item())

    def tree_state():
        params = tmap(lambda v: torch.zeros_like(v), clients[0])
        return params, opt.init(params)

    def tree_c(params, state, w):
        cmt = tu.tree_clipped_mean(list(zip(clients, w)), Ct)
        return server.fused_tree_mean_update([(cmt.mean, 1.0)], opt, params, state), cmt

    (ta, tsa), (tc, tsc) = tree_state(), tree_state()
    gt = server.fused_tree_clipped_mean_update(list(zip(clients, wt)), Ct, opt, ta, tsa)
    tsa = gt.state
    tsc, cmt = tree_c(tc, tsc, wt)
    tree_same = bool(torch.equal(flat_bits([ta]), flat_bits([tc])) and all(
        torch.equal(flat_bits([tsa[k]]), flat_bits([tsc[k]])) for k in ("m", "v")) and torch.equal(
        gt.clipped_norms.view(torch.int32), cmt.clipped_norms.view(torch.int32)))
    tree_clipped = int(gt.clipped.sum().item())
    box.update({"tsa": tsa, "tsc": tsc})
    ua, ub, uc = turns(wt), turns(wt), turns(wt)

    def run_a_tree():
        box["tsa"] = server.fused_tree_clipped_mean_update(list(zip(clients, ua())), Ct, opt, ta, box["tsa"]).state

    def run_b_tree():
        return tu.tree_clipped_mean(list(zip(clients, ub())), Ct)

    def run_c_tree():
        box["tsc"], _ = tree_c(tc, box["tsc"], uc())

    runs = {"a_slab": run_a_slab, "b_slab": run_b_slab, "c_slab": run_c_slab,
            "a_tree": run_a_tree, "b_tree": run_b_tree, "c_tree": run_c_tree}
    reps = {"a_slab": 10, "b_slab": 10, "c_slab": 10, "a_tree": 20, "b_tree": 20, "c_tree": 20}
    for fn in runs.values():  # warm up every leg
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    if args.once:
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        return
    sink = open(args.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    # what the algorithm must move on the slab: every row twice (norms, fold); (a) also reads and
    # writes params, m, v; (b) writes the mean
    fold_bytes, state_bytes, mean_bytes = 2 * Ks * Ps * 4, Ps * 4 * 6, Ps * 4
    emit({"slab": [Ks, Ps], "pytree": [Kt, tslab.num_params], "small": bool(args.small), "rule": "adam",
          "clipped_clients": {"slab": slab_clipped, "pytree": tree_clipped},
          "a_bitwise_equal_to_two_step_route": {"slab": slab_same, "pytree": tree_same},
          "slab_fold_bytes": fold_bytes, "slab_state_bytes": state_bytes})
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
    summary["b_slab_GBs"] = round((fold_bytes + mean_bytes) / med["b_slab"] / 1e6, 1)
    # the expectations of DESIGN §3j, confirmed or refuted by this run
    for route in ("slab", "tree"):
        summary[f"{route}_a_below_c_by_more_than_c_spread"] = bool(
            med[f"c_{route}"] - med[f"a_{route}"] > spread[f"c_{route}"])
    extra_ms = med["b_slab"] * (state_bytes - mean_bytes) / (fold_bytes + mean_bytes)  # at (b)'s own rate
    summary["slab_extra_state_ms_at_b_rate"] = round(extra_ms, 4)
    summary["slab_a_minus_b_ms"] = round(med["a_slab"] - med["b_slab"], 4)
    summary["slab_a_minus_b_within_b_spread_plus_state_traffic"] = bool(
        med["a_slab"] - med["b_slab"] <= spread["b_slab"] + extra_ms)
    emit(summary)


if __name__ == "__main__":
    main()
