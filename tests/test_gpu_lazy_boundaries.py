"""The state fjhost keeps between calls, at the boundaries where it can go wrong silently: lazy
norms and deferred running sums across the start of a graph capture (A), a norm taken on one
stream and folded by a mean on another (B), DLPack producers as leaves (C), the fused-norm fold
on a second device (D) and more pytree structures than solo_structure's table holds (E).

References: a mean is bitwise oracle/tree_util_ref.tree_mean; a norm is within rtol 2e-6 of the
float64 norm and bitwise the norm of a clone of the same delta computed alone,
eagerly. The alone bits are computed after the view under test has been read, so a column
nothing wrote cannot hold the right answer by accident.
"""
import json
import os
import re
import textwrap

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import kernels, pytree, tree_util as tu
from oracle import tree_util_ref as ref
from tests.test_gpu_lazy_norms import (SMALL, bits, example_round, f64norm, lazy_on, make_deltas,  # noqa: F401
                                       same_mean, tmap, want_mean)

pytestmark = pytest.mark.gpu
H = tu._HOST
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = [3, 1, 4, 1, 5, 9]


def alone_bits(delta):
    """The norm of a clone of `delta`, computed by its own launch."""
    return bits(tu.tree_l2_norm(tmap(lambda x: x.clone(), delta))).clone()


def check_norms(views, deltas):
    got = [bits(v).clone() for v in views]  # (read first: the alone norms below launch nothing into these columns)
    np.testing.assert_allclose([float(g.view(torch.float32)) for g in got], [f64norm(d) for d in deltas], rtol=2e-6)
    for k, (g, d) in enumerate(zip(got, deltas)):
        assert torch.equal(g, alone_bits(d)), k


def rewrite(xs, seed):
    new = make_deltas(SMALL, len(xs), seed, xs[0]["a"].device)
    with torch.no_grad():
        for x, y in zip(xs, new):
            for a, b in zip(pytree.leaves_of(x), pytree.leaves_of(y)):
                a.copy_(b)


def warm(xs, ws, st):
    """One eager round on the default stream and one on the capture's, then a synchronize
    (test_captured_rounds_with_norms_replay's preamble)."""
    example_round(xs, ws)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        example_round(xs, ws)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ A. capture boundary
@pytest.mark.parametrize("pre", ["unrelated", "same_tree"])
def test_capture_with_a_norm_pending_from_before(cuda, pre):
    """A1 / A2: a standalone norm is still pending when the capture starts (of a delta outside
    the round, or of the round's first delta itself). The norms taken inside the capture are
    recorded launches all the same: every replay refreshes them (the bits of the new contents'
    norms alone) and the mean (the oracle's bits); the view of xs[0] returned inside the capture
    is not the pre-capture node. The pre-capture view reads its own delta's norm afterwards."""
    xs = make_deltas(SMALL, 6, 31, cuda)
    extra = make_deltas(SMALL, 1, 32, cuda)[0]
    st = torch.cuda.Stream(cuda)
    warm(xs, WS, st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        target = extra if pre == "unrelated" else xs[0]
        p = tu.tree_l2_norm(target)
        assert H.solo_info()["pending"] == 1
        with torch.cuda.graph(g, stream=st):
            mean, norms = example_round(xs, WS)
    torch.cuda.synchronize()
    assert all(v._ticket is not p._ticket for v in norms)
    assert all(v._ticket.node is None for v in norms)  # (computed by recorded launches, nothing left pending)
    check_norms([p], [target])  # (before any rewrite: the value at its call)
    for seed in (33, 34):
        rewrite(xs, seed)
        g.replay()
        torch.cuda.synchronize()
        check_norms(norms, xs)
        assert same_mean(mean, want_mean(xs, WS)), seed


@pytest.mark.parametrize("touch", ["stack", "resolve", "evict"])
def test_pre_capture_node_touched_while_capturing(cuda, touch):
    """A3: a pending norm from before the capture is read (torch.stack), resolved (solo_resolve) or
    due for eviction (max_pending) while the stream is capturing. A launch issued then is only
    recorded, so the node must not count as done on its strength: after the capture block and
    before any replay the view reads its delta's norm. The contract: the touch
    raises RuntimeError naming the capture and launches nothing; the node stays pending; norms
    taken inside the capture never become pending, so they force no eviction."""
    xs = make_deltas(SMALL, 6, 41, cuda)
    extras = make_deltas(SMALL, 3, 42, cuda)
    st = torch.cuda.Stream(cuda)
    warm(xs, WS, st)
    g = torch.cuda.CUDAGraph()
    raised = None
    with torch.cuda.stream(st):
        if touch == "evict":
            tu.set_lazy_norms(True, max_pending=4)
            held = [tu.tree_l2_norm(e) for e in extras]
            assert H.solo_info()["pending"] == 3
        else:
            held = [tu.tree_l2_norm(extras[0])]
        p = held[0]
        with torch.cuda.graph(g, stream=st):
            y = xs[0]["a"] * 2.0  # (the graph is never empty)
            before = H.solo_info()["eager_launches"]
            try:
                if touch == "stack":
                    torch.stack([p])
                elif touch == "resolve":
                    H.solo_resolve([p._ticket])
                else:
                    inside = [tu.tree_l2_norm(x) for x in xs]
            except RuntimeError as e:
                raised = str(e)
                assert H.solo_info()["eager_launches"] == before
    torch.cuda.synchronize()
    if raised is not None:
        assert re.search("captur", raised), raised
        assert p._ticket.node is not None  # still pending
    check_norms(held, extras[:len(held)])  # no replay has run
    del y


def test_running_sum_begun_before_the_capture(cuda):
    """A4: a deferred running sum with one client, left unmaterialised, is extended and scaled
    inside a capture. Either those calls raise RuntimeError naming the capture and the chain
    materialises correctly afterwards, or the pre-capture sum reads the oracle's bits for its one
    client and every replay gives the oracle's mean of the rewritten deltas."""
    xs = make_deltas(SMALL, 6, 51, cuda)
    W = float(sum(WS))
    st = torch.cuda.Stream(cuda)

    def rest(s):
        for x, w in zip(xs[1:], WS[1:]):
            s = tu.tree_add(s, tu.tree_weight(x, w))
        return tu.tree_inverse_weight(s, W)

    def np_tree(t):
        return tmap(lambda x: x.cpu().numpy(), t)

    def want_sum(n):
        s = ref.tree_zeros_like(np_tree(xs[0]))
        for x, w in zip(xs[:n], WS[:n]):
            s = ref.tree_add(s, ref.tree_weight(np_tree(x), w))
        return s

    rest(tu.tree_add(tu.tree_zeros_like(xs[0]), tu.tree_weight(xs[0], WS[0])))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    raised, mean = None, None
    with torch.cuda.stream(st):
        rest(tu.tree_add(tu.tree_zeros_like(xs[0]), tu.tree_weight(xs[0], WS[0])))
        torch.cuda.synchronize()
        s = tu.tree_add(tu.tree_zeros_like(xs[0]), tu.tree_weight(xs[0], WS[0]))
        assert isinstance(s, tu.PendingSum)
        with torch.cuda.graph(g, stream=st):
            y = xs[0]["a"] * 2.0
            try:
                mean = rest(s)
            except RuntimeError as e:
                raised = str(e)
    torch.cuda.synchronize()
    del y
    if raised is not None:
        assert re.search("captur", raised), raised
        assert same_mean(rest(s), ref.tree_inverse_weight(want_sum(6), W))
        return
    assert same_mean(s, want_sum(1))
    for seed in (52, 53):
        rewrite(xs, seed)
        g.replay()
        torch.cuda.synchronize()
        assert same_mean(mean, ref.tree_inverse_weight(want_sum(6), W)), seed


# ------------------------------------------------------------------ B. two streams
_DELAY = {}


def _delay(dev):
    """Tens of ms of work on the current stream: a short chain of large matmuls."""
    m = _DELAY.get(dev)
    if m is None:
        m = _DELAY[dev] = torch.full((8192, 8192), 1e-4, device=dev)
        torch.mm(m, m)  # (library initialisation stays outside the race)
        torch.cuda.synchronize()
    a = m
    for _ in range(4):
        a = torch.mm(a, m)
    return a


@pytest.mark.parametrize("mirrored", [False, True])
def test_norms_on_one_stream_mean_on_another(cuda, mirrored):
    """B: the norms are taken on one stream, the mean runs (behind a delay) on another, and the
    views are read at once on the norms' stream with no device-wide synchronize: each reads its
    delta's norm (a reader is ordered behind its own stream only, as with the reference's eager
    norms), and the mean is the oracle's. Round 1 on the norms' stream leaves other values in the
    pooled columns."""
    X = make_deltas(SMALL, 8, 61, cuda)
    Y = [tmap(lambda x: x * 2.0, d) for d in X]
    ws = [2, 7, 1, 8, 2, 8, 1, 8]
    A, B = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    s_norm, s_mean = (B, torch.cuda.default_stream(cuda)) if mirrored else (A, B)
    _delay(cuda)
    with torch.cuda.stream(s_norm):
        mean1, norms1 = example_round(X, ws)
    del norms1
    torch.cuda.synchronize()
    with torch.cuda.stream(s_norm):
        views = [tu.tree_l2_norm(d) for d in Y]
    with torch.cuda.stream(s_mean):
        keep = _delay(cuda)
        mean = tu.tree_mean(list(zip(Y, ws)))
    with torch.cuda.stream(s_norm):
        got = [float(v) for v in views]
        got_bits = [bits(v).clone() for v in views]
    s_mean.synchronize()
    torch.cuda.synchronize()
    del keep
    np.testing.assert_allclose(got, [f64norm(d) for d in Y], rtol=2e-6)
    for k, (b, d) in enumerate(zip(got_bits, Y)):
        assert torch.equal(b, alone_bits(d)), k
    assert same_mean(mean, want_mean(Y, ws))
    assert same_mean(mean1, want_mean(X, ws))


# ------------------------------------------------------------------ C. DLPack leaves
class Producer:
    """A DLPack producer and nothing else (as a jax.Array is to this library): a private torch
    tensor behind __dlpack__ / __dlpack_device__."""

    def __init__(self, t):
        self._t = t

    def __dlpack__(self, stream=None, **kw):
        return self._t.__dlpack__(stream=stream, **kw)

    def __dlpack_device__(self):
        return self._t.__dlpack_device__()


def wrap(tree):
    return tmap(Producer, tree)


def same_tree_bits(a, b):
    la, lb = pytree.leaves_of(a), pytree.leaves_of(b)
    return len(la) == len(lb) and all(x.dtype == y.dtype and x.shape == y.shape and
                                      torch.equal(x.contiguous().view(torch.uint8).cpu(), y.contiguous().view(torch.uint8).cpu())
                                      for x, y in zip(la, lb))


def library_loop(trees, ws):
    s = tu.tree_zeros_like(trees[0])
    for t, w in zip(trees, ws):
        s = tu.tree_add(s, tu.tree_weight(t, w))
    return tu.tree_inverse_weight(s, float(sum(ws)))


@pytest.mark.parametrize("K", [1, 3, 10])
def test_dlpack_leaves_match_torch_leaves(cuda, K):
    """C1 / C2: every route the example and the library loop take, given DLPack producers as
    leaves, returns the bits the same call returns for the underlying tensors; means are the
    oracle's bits and norms within 2e-6 of float64."""
    deltas = make_deltas(SMALL, K, 70 + K, cuda)
    prods = [wrap(d) for d in deltas]
    ws = [k % 7 + 1 for k in range(K)]
    want = want_mean(deltas, ws)
    got = tu.tree_mean(list(zip(prods, ws)))
    assert same_tree_bits(got, tu.tree_mean(list(zip(deltas, ws)))) and same_mean(got, want)
    for fn, power in ((tu.tree_l2_norm, 1), (tu.tree_l2_squared, 2)):
        for p, d in zip(prods, deltas):
            v = fn(p)
            assert torch.equal(bits(v), bits(fn(tmap(lambda x: x.clone(), d))))
            assert float(v) == pytest.approx(f64norm(d) ** power, rel=2e-6 * power)
    mean, norms = example_round(prods, ws)
    mean_t, norms_t = example_round(deltas, ws)
    assert same_tree_bits(mean, mean_t) and same_mean(mean, want)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(norms, norms_t))
    np.testing.assert_allclose([float(v) for v in norms], [f64norm(d) for d in deltas], rtol=2e-6)
    agg = fedjax_amd.aggregators.mean_aggregator()
    m_p, _ = agg.apply([(str(k), p, w) for k, (p, w) in enumerate(zip(prods, ws))], agg.init())
    m_t, _ = agg.apply([(str(k), d, w) for k, (d, w) in enumerate(zip(deltas, ws))], agg.init())
    assert same_tree_bits(m_p, m_t) and same_mean(m_p, want)
    loop = library_loop(prods, ws)
    assert same_tree_bits(loop, library_loop(deltas, ws))
    s_ref = ref.tree_zeros_like(tmap(lambda x: x.cpu().numpy(), deltas[0]))
    for d, w in zip(deltas, ws):
        s_ref = ref.tree_add(s_ref, ref.tree_weight(tmap(lambda x: x.cpu().numpy(), d), w))
    assert same_mean(loop, ref.tree_inverse_weight(s_ref, float(sum(ws))))


@pytest.mark.parametrize("kind", ["mixed", "bf16", "int32", "transposed", "cpu"])
def test_dlpack_other_leaf_kinds(cuda, kind):
    """C3: trees mixing producers and tensors, bfloat16 and int32 producers, a producer over a
    transposed (non-contiguous) tensor and one over a host tensor each give the result of the
    equivalent contiguous device tensors."""
    K = 3
    deltas = make_deltas(SMALL, K, 80, cuda)
    ws = [2, 5, 3]
    if kind == "mixed":
        prods = [{"a": Producer(d["a"]) if k % 2 else d["a"], "b": {"c": d["b"]["c"] if k % 2 else Producer(d["b"]["c"])}}
                 for k, d in enumerate(deltas)]
    elif kind == "bf16":
        deltas = [tmap(lambda x: x.to(torch.bfloat16), d) for d in deltas]
        prods = [wrap(d) for d in deltas]
    elif kind == "int32":
        deltas = [tmap(lambda x: (x * 1e5).to(torch.int32), d) for d in deltas]
        prods = [wrap(d) for d in deltas]
    elif kind == "transposed":
        base = [d["b"]["c"].t().contiguous() for d in deltas]  # [3, 33]; .t() is the [33, 3] leaf, strided
        prods = [{"a": Producer(d["a"]), "b": {"c": Producer(b.t())}} for d, b in zip(deltas, base)]
        assert not base[0].t().is_contiguous()
    else:
        prods = [wrap(tmap(lambda x: x.cpu(), d)) for d in deltas]
    got = tu.tree_mean(list(zip(prods, ws)))
    assert same_tree_bits(got, tu.tree_mean(list(zip(deltas, ws))))
    if kind in ("mixed", "transposed", "cpu"):
        assert same_tree_bits(library_loop(prods, ws), library_loop(deltas, ws))
    if kind != "int32":
        for p, d in zip(prods, deltas):
            assert torch.equal(bits(tu.tree_l2_norm(p).float()), bits(tu.tree_l2_norm(d).float()))
    if kind in ("mixed", "transposed", "cpu"):
        assert same_mean(got, want_mean(deltas, ws))


def test_dlpack_leaves_are_read_at_every_call(cuda):
    """C4: nothing of a producer's earlier contents is kept: after its private tensor is
    rewritten in place the next mean and norm see the new values."""
    deltas = make_deltas(SMALL, 3, 90, cuda)
    prods = [wrap(d) for d in deltas]
    ws = [1, 2, 3]
    first = tu.tree_mean(list(zip(prods, ws)))
    n_first = float(tu.tree_l2_norm(prods[0]))
    assert same_mean(first, want_mean(deltas, ws))
    assert n_first == pytest.approx(f64norm(deltas[0]), rel=2e-6)
    rewrite(deltas, 91)
    second = tu.tree_mean(list(zip(prods, ws)))
    assert same_mean(second, want_mean(deltas, ws)) and not same_tree_bits(first, second)
    n_second = tu.tree_l2_norm(prods[0])
    assert float(n_second) == pytest.approx(f64norm(deltas[0]), rel=2e-6)
    assert torch.equal(bits(n_second), alone_bits(deltas[0]))


# ------------------------------------------------------------------ D. second device
def rounds_on_devices(devices):
    """The dense fused-norm fold and an example round of the same inputs on each device in turn:
    every result's bits, per device."""
    g = torch.Generator().manual_seed(95)
    x_host = (torch.rand(10, 5003, generator=g) - 0.5) * 0.02
    w_host = torch.arange(1, 11, dtype=torch.float32)
    host_deltas = make_deltas(SMALL, 4, 96, torch.device("cpu"))
    ws = [1, 2, 3, 4]
    want = ref.tree_mean([(tmap(lambda t: t.numpy(), h), w) for h, w in zip(host_deltas, ws)])
    outs = []
    for d in devices:
        dev = torch.device("cuda", d)
        with torch.cuda.device(dev):
            out, l2sq = kernels.weighted_sum_l2_dense(x_host.to(dev), w_host.to(dev), scale=1.0 / 55.0)
            deltas = [tmap(lambda t: t.to(dev), h) for h in host_deltas]
            mean, norms = example_round(deltas, ws)
            torch.cuda.synchronize(dev)
            assert same_mean(mean, want), d
            np.testing.assert_allclose([float(v) for v in norms], [f64norm(h) for h in host_deltas], rtol=2e-6)
            np.testing.assert_allclose(l2sq.sqrt().cpu().numpy(), (x_host.double() ** 2).sum(1).sqrt().numpy(), rtol=2e-6)
            outs.append([bits(out), bits(l2sq)] + [bits(v).clone() for v in norms] +
                        [bits(m) for m in pytree.leaves_of(mean)])
    return outs


def test_fused_norm_fold_on_a_second_device():
    """D: the dense fold with fused norms (more than 64 KiB of dynamic LDS: the attribute is per
    device) and an example round, on device 0 and then device 1 of one process: both succeed
    with the same bits for the same inputs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices in one process")
    from fedjax_amd import _lib
    _lib.load()
    first, second = rounds_on_devices((0, 1))
    assert len(first) == len(second) and all(torch.equal(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------ E. past 4096 structures
STRUCTURES_SCRIPT = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, sys.argv[1])
    import numpy as np, torch
    from fedjax_amd import tree_util as tu
    H = tu._HOST
    dev = torch.device("cuda:0")
    R, CUT = 4200, 4096
    g = torch.Generator(device=dev).manual_seed(7)
    base = (torch.rand(R, 2, 2, 16, device=dev, generator=g) - 0.5) * 0.02
    ws = [3, 5]
    fused, all_norms, all_means, seen = [0, 0], [], [], set()
    for r in range(R):
        keys = [f"w{i}" for i in range(2)]  # fresh, non-interned key objects every round
        seen.update(id(k) for k in keys)
        deltas = [{keys[0]: base[r, k, 0], keys[1]: base[r, k, 1]} for k in range(2)]
        f0 = H.solo_info()["fused"]
        norms = [tu.tree_l2_norm(d) for d in deltas]
        mean = tu.tree_mean(list(zip(deltas, ws)))
        fused[r >= CUT] += H.solo_info()["fused"] - f0
        all_norms.append(torch.stack(norms))
        all_means.append(torch.stack([mean["w0"], mean["w1"]]))
    host = base.cpu().numpy()
    got_n = torch.stack(all_norms).cpu().numpy().astype(np.float64)  # [R, 2]
    got_m = torch.stack(all_means).cpu().numpy()  # [R, 2, 16]
    want_n = np.sqrt((host.astype(np.float64) ** 2).sum(axis=(2, 3)))
    bad_n = np.argwhere(np.abs(got_n - want_n) > 2e-6 * want_n)
    s = host[:, 0] * np.float32(ws[0])  # the oracle's order: fl(x0 w0), + fl(x1 w1), * f32(1/W)
    s = s + host[:, 1] * np.float32(ws[1])
    want_m = s * np.float32(1.0 / float(sum(ws)))
    bad_m = np.argwhere(want_m.view(np.uint32) != got_m.view(np.uint32))
    out = {"bad_norms": bad_n[:5].tolist(), "bad_means": bad_m[:5].tolist(), "n_bad": int(len(bad_n) + len(bad_m)),
           "pending": H.solo_info()["pending"], "key_objects": len(seen),
           "fused_fraction_before": fused[0] / (2.0 * CUT), "fused_fraction_after": fused[1] / (2.0 * (R - CUT))}
    line = json.dumps(out)
    path = os.environ.get("FJ_BENCH_JSON")
    if path:
        with open(path, "w") as f:
            f.write(line)
    print(line)
""")


def test_values_stay_right_past_4096_structures(cuda, tmp_path, capfd):
    """E: 4200 example rounds of two clients whose dict keys are fresh objects every round, in one
    fresh child process (solo_structure's table is a process-wide static: filling it here would
    push every later test off the fused route). Every round's norms are within 2e-6 of float64
    and its mean the float32 fold in the oracle's order; nothing is left pending. Past its cap
    the table starts over instead of sending new structures to the Python route for good, so
    the norms stay fused into the mean before and after round 4096 (the fractions are printed)."""
    import bench
    p = tmp_path / "structures.py"
    p.write_text(STRUCTURES_SCRIPT)
    rc = bench.spawn_ranks(1, [ROOT], script=str(p), timeout=170)
    cap = capfd.readouterr()
    assert rc == 0, cap.err[-2000:]
    lines = [ln for ln in cap.out.splitlines() if ln.strip()]
    assert len(lines) == 1, cap.out
    d = json.loads(lines[0])
    print("fused fraction before / after round 4096:", d["fused_fraction_before"], d["fused_fraction_after"])
    assert d["n_bad"] == 0, (d["bad_norms"], d["bad_means"])
    assert d["pending"] == 0
    assert d["key_objects"] >= 2 * 4096  # (fresh key objects every round: the table held a structure per round)
    assert d["fused_fraction_before"] == 1.0 and d["fused_fraction_after"] == 1.0
