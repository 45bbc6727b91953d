"""The mean around the median on the GPU (fjagg_meamed_dense / fjagg_meamed_ptrs and the Python
surface over them) against the numpy restatement in tests/around_median_ref.py, bit for bit.
Bit patterns are compared with every NaN mapped to one pattern, as the trimmed-mean tests do:
the sign and payload of a NaN that an add generates are the implementation's."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, pytree, slab as slab_mod, tree_util as tu
from tests import around_median_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
MS = [1, 2, 3, 15, 16, 17, 32, 33, 64, 65, 127, 128]
PS = [1, 63, 64, 65, 255, 257, 1000]


def assert_bits(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    g, w = ref.canon(got).reshape(-1), ref.canon(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


def betas(M, rng):
    return sorted({1, min(2, M), max(M // 2, 1), max(M - 1, 1), M, int(rng.randint(1, M + 1))})


def on_device(x, dev, ld=None, offset=0):
    """x [K, P] as a device view with row stride ld and a base offset in elements; everything
    around the rows holds NaN (never read)."""
    K, P = x.shape
    ld = P if ld is None else ld
    store = torch.full((offset + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:].view(K, ld)[:, :P]
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def scale_of(beta):
    return float(F32(tu._inverse(beta)))


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def slab_of(x, dev):
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(x.shape[1])}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x)))
    return s


# ------------------------------------------------------- 1. M x P x beta x data on all three routes
@pytest.mark.parametrize("M", MS)
def test_sweep_bitwise(cuda, M):
    rng = np.random.RandomState(900 + M)
    for P in PS:
        for kind in ("normal", "ties", "specials"):
            x = ref.DATA[kind](rng, M, P)
            xd = on_device(x, cuda, ld=P + 3)  # ld > P, NaN in the padding
            s = slab_of(x, cuda)
            clients = [{"w": xd[k]} for k in range(M)]
            for beta in betas(M, rng):
                want = ref.mean_around_median(x, beta)
                what = f"M={M} P={P} {kind} beta={beta}"
                for nt in (False, True):
                    got = kernels.meamed_dense(xd, beta, scale=scale_of(beta), nontemporal=nt)
                    assert_bits(got, want, f"dense {what} nt={nt}")
                assert_bits(s.mean_around_median(beta)["w"], want, f"slab {what}")
                assert_bits(tu.tree_mean_around_median(clients, beta)["w"], want, f"tree {what}")


# ------------------------------------------------------------------------------ 2. row tables
def test_row_table_reads_only_its_rows(cuda):
    """A slab of 200 rows inside one allocation of exactly 200 rows: the table names 128 of them,
    indices >= 128 among them; every other row — the first and the last of the allocation among
    them, so nothing but this allocation makes their addresses valid — holds NaN."""
    K, M, P = 200, 128, 321
    rng = np.random.RandomState(11)
    rows = np.sort(rng.choice(np.arange(1, K - 1), size=M, replace=False))
    assert rows[-1] >= 128 and 0 not in rows and K - 1 not in rows
    x = np.full((K, P), np.nan, F32)
    x[rows] = ref.specials(rng, M, P)
    x[rows[:40]] = ref.integer_ties(rng, 40, P)
    xd = torch.from_numpy(x).to(cuda)
    gathered = on_device(x[rows], cuda)
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    s.rows.copy_(xd)
    for beta in (1, 37, 96, 128):
        want = ref.mean_around_median(x[rows], beta)
        got = kernels.meamed_dense(xd, beta, rows, scale=scale_of(beta))
        assert_bits(got, want, f"table beta={beta}")
        assert_bits(kernels.meamed_dense(xd, beta, rows.tolist(), scale=scale_of(beta), nontemporal=True), want,
                    "list, nt")
        assert_bits(got, kernels.meamed_dense(gathered, beta, scale=scale_of(beta)).cpu().numpy(),
                    f"gathered slab beta={beta}")
        assert_bits(s.mean_around_median(beta, rows=rows)["w"], want, f"slab beta={beta}")
    # small tables at every width, and a table of one row
    for m in (1, 2, 16, 17, 33, 65):
        sub = np.sort(rng.choice(rows, size=m, replace=False))
        beta = max(m // 2, 1)
        assert_bits(kernels.meamed_dense(xd, beta, sub, scale=scale_of(beta)), ref.mean_around_median(x[sub], beta),
                    f"m={m}")


# --------------------------------------------------------------------------------- 3. pytrees
LEAF_SETS = ([0, 1, 3], [5], [255, 257, 0, 1023], [3000, 1, 4 * 7 - 1, 4 * 7 + 1, 256 * 2 - 1, 256 * 2 + 1, 0], [1, 1],
             [1025, 7])


@pytest.mark.parametrize("views", [False, True])
def test_pytree_route_is_the_slab_route(cuda, views):
    rng = np.random.RandomState(21 + views)
    for n, leaves in enumerate(LEAF_SETS):
        K = [5, 16, 33, 70, 128, 2][n]
        P = sum(leaves)
        offs = np.concatenate([[0], np.cumsum(leaves)])
        x = ref.specials(rng, K, P)
        clients = []
        for k in range(K):
            if views:  # one row a client, one element into its buffer: the leaves sit at odd element offsets
                buf = torch.empty(P + 1, dtype=torch.float32, device=cuda)
                buf[1:].copy_(torch.from_numpy(x[k]))
                clients.append({f"l{j}": buf[1 + offs[j]:1 + offs[j + 1]] for j in range(len(leaves))})
            else:
                clients.append({f"l{j}": torch.from_numpy(x[k, offs[j]:offs[j + 1]].copy()).to(cuda)
                                for j in range(len(leaves))})
        s = slab_mod.ClientDeltaSlab({f"l{j}": torch.zeros(leaves[j]) for j in range(len(leaves))}, K, device=cuda)
        s.rows.copy_(torch.from_numpy(x))
        for beta in sorted({1, max(K // 2, 1), K}):
            want = ref.mean_around_median(x, beta)
            got = tu.tree_mean_around_median(iter(clients), beta)  # a one-shot iterable
            assert [got[f"l{j}"].numel() for j in range(len(leaves))] == leaves
            assert_bits(flat_of(got), want, f"tree leaves={leaves} K={K} beta={beta}")
            assert_bits(flat_of(got), flat_of(s.mean_around_median(beta)), "tree against slab")
        agg = fedjax_amd.aggregators.mean_around_median_aggregator(max(K // 2, 1))
        state = agg.init()
        got, state2 = agg.apply(((f"c{k}", c, 1 + k % 3) for k, c in enumerate(clients)), state)
        assert state2 is state
        assert_bits(flat_of(got), ref.mean_around_median(x, max(K // 2, 1)), "aggregator: the weights change nothing")


def test_launch_wide_unaligned_plan(cuda):
    rng = np.random.RandomState(31)
    K, leaves = 40, [257, 3, 64]
    offs = np.concatenate([[0], np.cumsum(leaves)])
    x = ref.specials(rng, K, sum(leaves))
    bufs = [torch.empty(sum(leaves) + 1, dtype=torch.float32, device=cuda) for _ in range(K)]
    for k, b in enumerate(bufs):
        b[1:].copy_(torch.from_numpy(x[k]))
    out = torch.full((sum(leaves) + 1,), -7.0, device=cuda)
    in_ptrs = np.array([[b.data_ptr() + 4 * (1 + offs[j]) for j in range(len(leaves))] for b in bufs], dtype=np.int64)
    out_ptrs = out.data_ptr() + 4 * (1 + offs[:-1].astype(np.int64))
    leaf_n = np.array(leaves, dtype=np.int64)
    blocks = kernels.ptrs_plan(_lib.F32, leaf_n, True)
    image = torch.from_numpy(np.concatenate([in_ptrs.ravel(), out_ptrs, leaf_n, blocks])).to(cuda)
    for beta in (1, 13, 40):
        kernels.meamed_ptrs(image, len(leaves), K, len(blocks) // 2, beta, scale_of(beta), unaligned=True)
        assert_bits(out[1:], ref.mean_around_median(x, beta), f"beta={beta}")
        assert out[0].item() == -7.0


# ------------------------------------------------------------------------------ 4. identities
@pytest.mark.parametrize("M", [1, 2, 16, 17, 33, 65, 127, 128])
def test_identities(cuda, M):
    template = {"w": torch.zeros(1021), "b": torch.zeros(5)}
    s = slab_mod.ClientDeltaSlab(template, M, device=cuda).fill_synthetic(seed=M)
    for a, b in zip(pytree.leaves_of(s.mean_around_median(M)), pytree.leaves_of(s.mean([1] * M))):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if M % 2:
        for a, b in zip(pytree.leaves_of(s.mean_around_median(1)), pytree.leaves_of(s.median())):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_out_and_empty_template(cuda):
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(130), "b": torch.zeros(3)}, 10, device=cuda).fill_synthetic(seed=5)
    x = s.rows.cpu().numpy()
    out = torch.zeros(133, device=cuda)
    got = s.mean_around_median(np.int64(4), out=out)
    assert got["b"].data_ptr() == out.data_ptr()
    assert_bits(out, ref.mean_around_median(x, 4), "out")
    assert torch.equal(s.rows.cpu(), torch.from_numpy(x))  # inputs unchanged
    e = slab_mod.ClientDeltaSlab({"w": torch.zeros(0)}, 4, device=cuda)
    assert e.mean_around_median(2)["w"].numel() == 0 and e.mean_around_median(1, rows=[1, 3])["w"].numel() == 0


# ---------------------------------------------------------------------------- 5. graph capture
def graph_nodes_and_edges(graph):
    """(number of nodes, [(from, to)]) of a graph captured with keep_graph=True, read through the
    HIP runtime that torch itself loaded."""
    import ctypes
    import os

    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n, e = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    assert hip.hipGraphGetEdges(raw, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * max(e.value, 1))(), (ctypes.c_void_p * max(e.value, 1))()
    if e.value:
        assert hip.hipGraphGetEdges(raw, src, dst, ctypes.byref(e)) == 0
    return n.value, [(src[i], dst[i]) for i in range(e.value)]


@pytest.mark.parametrize("with_rows", [False, True])
def test_slab_capture_replays(cuda, with_rows):
    K = 40
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(4099), "b": torch.zeros(5)}, K, device=cuda).fill_synthetic(seed=1)
    rows = list(range(1, K, 3)) if with_rows else None
    beta = 5
    out = torch.zeros(s.num_params, device=cuda)
    s.mean_around_median(beta, rows=rows, out=out)  # eager once: the kernel is loaded before the capture
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = s.mean_around_median(beta, rows=rows, out=out)
    for seed in (2, 3):
        s.fill_synthetic(seed=seed)
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        x = s.rows.cpu().numpy()
        assert_bits(flat_of(res), flat_of(s.mean_around_median(beta, rows=rows)), f"replay with seed {seed}")
        assert_bits(flat_of(res), ref.mean_around_median(x if rows is None else x[rows], beta),
                    f"replay {seed} restatement")


def test_captured_graph_is_linear(cuda):
    """No parallel branches: the nodes form one chain (here: one kernel node, no edge)."""
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(777)}, 20, device=cuda).fill_synthetic(seed=1)
    out = torch.zeros(s.num_params, device=cuda)
    for rows in (None, [0, 3, 19]):
        s.mean_around_median(2, rows=rows, out=out)
        torch.cuda.synchronize()
        g, st = torch.cuda.CUDAGraph(keep_graph=True), torch.cuda.Stream()
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st):
                s.mean_around_median(2, rows=rows, out=out)
        nodes, edges = graph_nodes_and_edges(g)
        assert nodes >= 1 and len(edges) == nodes - 1
        assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges)
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        x = s.rows.cpu().numpy()
        assert_bits(out, ref.mean_around_median(x if rows is None else x[rows], 2), "replay of the kept graph")


def test_tree_route_raises_under_capture(cuda):
    clients = [{"w": torch.randn(100, device=cuda)} for _ in range(5)]
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g, stream=st):
                tu.tree_mean_around_median(clients, 2)
    torch.cuda.synchronize()
    x = np.stack([c["w"].cpu().numpy() for c in clients])
    assert_bits(tu.tree_mean_around_median(clients, 2)["w"], ref.mean_around_median(x, 2),
                "eager after the refused capture")


# -------------------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing(cuda):
    x = torch.zeros(4, 64, device=cuda)
    big = torch.zeros(200, 8, device=cuda)
    with pytest.raises(ValueError, match="128"):
        kernels.meamed_dense(big, 1)
    with pytest.raises(ValueError, match="strictly ascending"):
        kernels.meamed_dense(big, 1, [5, 5])
    with pytest.raises(ValueError, match="strictly ascending"):
        kernels.meamed_dense(big, 1, [5, 200])
    with pytest.raises(TypeError, match="float32"):
        kernels.meamed_dense(x.to(torch.bfloat16), 1)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        kernels.meamed_dense(x, 5)
    b = slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 4, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        b.mean_around_median(1)
    with pytest.raises(TypeError, match="float32"):
        tu.tree_mean_around_median([{"w": torch.zeros(2, device=cuda, dtype=torch.int32)}] * 4, 1)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    bad_rows = np.array([3, 2], np.int32)
    assert lib.fjagg_meamed_dense(_lib.F32, big.data_ptr(), 8, 200, 8, None, 200, 1, 1.0, x.data_ptr(), 0, st) == -3
    assert lib.fjagg_meamed_dense(_lib.F32, big.data_ptr(), 8, 200, 8, bad_rows.ctypes.data, 2, 1, 1.0, x.data_ptr(), 0,
                                  st) == -1
    assert lib.fjagg_meamed_dense(_lib.F32, x.data_ptr(), 64, 4, 64, None, 4, 5, 1.0, x.data_ptr(), 0, st) == -1
    torch.cuda.synchronize()  # no pending HIP error, and a following valid call passes
    y = np.random.RandomState(8).standard_normal((4, 64)).astype(F32)
    assert_bits(kernels.meamed_dense(on_device(y, cuda), 2, scale=0.5), ref.mean_around_median(y, 2), "after the refusals")
