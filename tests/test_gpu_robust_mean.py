"""Coordinate-wise trimmed mean and median on the GPU (fjagg_trim_dense / fjagg_trim_ptrs and the
Python surface over them) against the numpy restatement in tests/robust_mean_ref.py, bit for
bit. Bit patterns are compared with every NaN mapped to one pattern, as the clipped-mean tests
do: the sign and payload of a NaN that an add generates are the implementation's."""
import functools

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import kernels, pytree, slab as slab_mod, tree_util as tu
from tests import robust_mean_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]
PS = [1, 3, 63, 64, 65, 257, 1000]
# the EMNIST-CNN leaf layout with its large leaves at 1/64 scale, a 1-element and an empty leaf
EMNIST_64 = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 1)},
             "linear": {"b": (128,), "w": (144, 128)}, "linear_1": {"b": (62,), "w": (2, 62)},
             "one": (1,), "zero": (0,)}


def assert_bits(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    g, w = ref.canon(got).reshape(-1), ref.canon(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


def trims(K):
    return sorted({0, min(1, (K - 1) // 2), (K - 1) // 2})  # (K-1)//2 is the median and the largest valid t


@functools.lru_cache(maxsize=None)
def normal(K, P, seed=0):
    x = np.random.RandomState(1000 * seed + 7 * K + P).standard_normal((K, P)).astype(F32)
    x.setflags(write=False)
    return x


def on_device(x, dev, ld=None, offset=0):
    """x [K, P] as a device view with row stride ld and a base offset in elements; everything
    around the rows holds NaN (never read)."""
    K, P = x.shape
    ld = P if ld is None else ld
    store = torch.full((offset + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:].view(K, ld)[:, :P]
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def scale_of(K, t):
    return float(F32(tu._inverse(K - 2 * t)))


def tmap(f, t):
    return {k: tmap(f, v) for k, v in t.items()} if isinstance(t, dict) else f(t)


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


# ------------------------------------------------------------------ 1. K x t x P on the wrapper
@pytest.mark.parametrize("K", KS)
def test_dense_sweep_bitwise(cuda, K):
    for P in PS:
        x = normal(K, P)
        xd = on_device(x, cuda, ld=P + 3)
        for t in trims(K):
            got = kernels.trim_dense(xd, t, scale=scale_of(K, t))
            assert_bits(got, ref.trimmed_mean(x, t), f"K={K} P={P} t={t}")


@pytest.mark.parametrize("K", [1, 2, 16, 17, 33, 65, 128])
def test_no_trim_is_slab_mean_with_unit_weights(cuda, K):
    template = {"w": torch.zeros(1021), "b": torch.zeros(5)}
    s = slab_mod.ClientDeltaSlab(template, K, device=cuda).fill_synthetic(seed=K)
    got, want = s.trimmed_mean(0), s.mean([1] * K)
    for a, b in zip(pytree.leaves_of(got), pytree.leaves_of(want)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert_bits(flat_of(got), ref.trimmed_mean(s.rows.cpu().numpy(), 0), "against the restatement")


@pytest.mark.parametrize("K", [1, 2, 3, 4, 9, 16, 31, 32, 64, 127, 128])
def test_median_is_np_median(cuda, K):
    rng = np.random.RandomState(K)
    P = 333
    x = (np.stack([rng.permutation(4 * K)[:K] for _ in range(P)], axis=1).astype(F32) * F32(0.37) - F32(K)).astype(F32)
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    s.rows.copy_(torch.from_numpy(x))
    assert_bits(s.median()["w"], np.median(x, axis=0).astype(F32), f"K={K}")
    assert_bits(s.median()["w"], ref.median(x), f"K={K} restatement")


# ------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("K", [2, 3, 5, 16, 17, 40, 65, 128])
def test_ties_bitwise(cuda, K):
    rng = np.random.RandomState(50 + K)
    P = 300
    three = np.array([-1.5, 0.25, 0.25000003], F32)[rng.randint(0, 3, (K, P))]
    const = np.repeat(rng.standard_normal((1, P)).astype(F32), K, axis=0)
    zeros = np.array([0.0, -0.0], F32)[rng.randint(0, 2, (K, P))]
    # L == U with duplicates on both sides of both cuts: one value fills most of the column
    dup = np.where(rng.random_sample((K, P)) < 0.8, F32(2.0), rng.standard_normal((K, P)).astype(F32)).astype(F32)
    x = np.concatenate([three, const, zeros, dup], axis=1)
    xd = on_device(x, cuda)
    for t in sorted({0, min(1, (K - 1) // 2), (K - 1) // 4, (K - 1) // 2}):
        got = kernels.trim_dense(xd, t, scale=scale_of(K, t))
        assert_bits(got, ref.trimmed_mean(x, t), f"K={K} t={t}")


def test_single_kept_negative_zero_stays(cuda):
    x = np.array([[-1.0, 1.0, -0.0], [-0.0, -0.0, 1.0], [1.0, -1.0, -1.0]], F32)
    got = kernels.trim_dense(on_device(x, cuda), 1, scale=1.0).cpu().numpy()
    assert got.view(np.uint32).tolist() == [0x80000000] * 3
    # the hand-worked tie of the CPU tests: [1, 1, 1, 2, 0] and the signed zeros, t = 1 and t = 2
    y = np.array([[1, 0.0], [1, -0.0], [1, -0.0], [2, 1.0], [0, -1.0]], F32)
    for t in (1, 2):
        got = kernels.trim_dense(on_device(y, cuda), t, scale=scale_of(5, t))
        assert_bits(got, ref.trimmed_mean(y, t), f"t={t}")
    assert kernels.trim_dense(on_device(y, cuda), 2).cpu().numpy().view(np.uint32).tolist() == [0x3F800000, 0x80000000]


# --------------------------------------------------------------------------------- 3. specials
def test_byzantine_clients_are_trimmed(cuda):
    K, P = 16, 777
    x = np.array(normal(K, P, seed=3))
    x[1] = np.nan
    x[5] = np.array([0xFFC00000], np.uint32).view(F32)[0]
    x[7] = np.inf
    x[10] = -np.inf
    x[14] = F32(3e38)
    xd = on_device(x, cuda)
    got = kernels.trim_dense(xd, 3, scale=scale_of(K, 3))
    assert torch.isfinite(got).all()
    assert_bits(got, ref.trimmed_mean(x, 3), "t=3")
    assert_bits(kernels.trim_dense(xd, 2, scale=scale_of(K, 2)), ref.trimmed_mean(x, 2), "t=2")
    # what the mean and a norm-clipped mean make of the same round
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    s.rows.copy_(xd)
    assert not torch.isfinite(s.mean([1] * K)["w"]).any()
    assert torch.isfinite(s.trimmed_mean(3)["w"]).all() and torch.isfinite(s.median()["w"]).all()


@pytest.mark.parametrize("K", [7, 16, 33, 100, 128])
def test_mixed_specials_bitwise(cuda, K):
    x = ref.mixed_data(np.random.RandomState(K), K, 500, special=0.3, ties=0.2)
    xd = on_device(x, cuda)
    for t in sorted({0, 1, (K - 1) // 3, (K - 1) // 2}):
        assert_bits(kernels.trim_dense(xd, t, scale=scale_of(K, t)), ref.trimmed_mean(x, t), f"K={K} t={t}")


# ------------------------------------------------------------------------- 4. alignment, out=
@pytest.mark.parametrize("K", [5, 20, 40, 128])
def test_rows_need_float_alignment_only(cuda, K):
    P, t = 333, (K - 1) // 3
    x = normal(K, P, seed=4)
    want = ref.trimmed_mean(x, t)
    sc = scale_of(K, t)
    assert_bits(kernels.trim_dense(on_device(x, cuda, ld=P + 2), t, scale=sc), want, "odd ld")
    assert_bits(kernels.trim_dense(on_device(x, cuda, ld=P + 4, offset=1), t, scale=sc), want, "base off by one")
    store = torch.full((P + 8,), -7.0, device=cuda)
    out = store[3:3 + P]
    xd = on_device(x, cuda, ld=P + 1, offset=3)
    before = xd.clone()
    assert kernels.trim_dense(xd, t, scale=sc, out=out) is out
    assert_bits(out, want, "out view at an odd offset")
    assert (store[:3] == -7).all() and (store[3 + P:] == -7).all()  # out= is honoured, nothing else written
    assert torch.equal(xd.view(torch.int32), before.view(torch.int32))  # inputs unchanged
    assert_bits(kernels.trim_dense(xd, t, scale=sc, nontemporal=True), want, "nontemporal")


def test_slab_out_and_empty_template(cuda):
    template = {"w": torch.zeros(130), "b": torch.zeros(3)}
    s = slab_mod.ClientDeltaSlab(template, 10, device=cuda).fill_synthetic(seed=5)
    x = s.rows.cpu().numpy()
    out = torch.zeros(133, device=cuda)
    got = s.trimmed_mean(0.2, out=out)
    assert got["b"].data_ptr() == out.data_ptr()  # views into out ("b" sorts first)
    assert_bits(out, ref.trimmed_mean(x, 2), "out")
    assert_bits(flat_of(s.trimmed_mean(np.int64(3))), ref.trimmed_mean(x, 3), "count")
    assert torch.equal(s.rows.cpu(), torch.from_numpy(x))
    e = slab_mod.ClientDeltaSlab({"w": torch.zeros(0)}, 4, device=cuda)
    assert e.trimmed_mean(1)["w"].numel() == 0 and e.median()["w"].numel() == 0


# --------------------------------------------------------------------------------- 5. pytrees
@functools.lru_cache(maxsize=None)
def emnist_round(K):
    """(x [K, P] numpy, offsets) for the scaled EMNIST layout, with specials and ties mixed in."""
    sizes = [z.size for z in pytree.leaves_of(tmap(lambda s: np.zeros(s, F32), EMNIST_64))]
    x = ref.mixed_data(np.random.RandomState(9 + K), K, sum(sizes), special=0.05, ties=0.05)
    x.setflags(write=False)
    return x, np.concatenate([[0], np.cumsum(sizes)])


def separate_clients(x, offs, dev, misalign_leaf=3):
    """K client pytrees of the scaled EMNIST layout, every (client, leaf) its own allocation; one
    leaf of every client is a view one element into its buffer (4-byte aligned only)."""
    template = tmap(lambda s: np.zeros(s, F32), EMNIST_64)
    shapes, td = pytree.flatten(template)
    clients = []
    for k in range(x.shape[0]):
        leaves = []
        for l, z in enumerate(shapes):
            v = torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]]))
            if l == misalign_leaf:
                buf = torch.empty(v.numel() + 1, dtype=torch.float32, device=dev)
                buf[1:].copy_(v)
                leaves.append(buf[1:].view(z.shape))
            else:
                leaves.append(v.to(dev).view(z.shape))
        clients.append(pytree.unflatten(td, leaves))
    return clients


@pytest.mark.parametrize("K", [10, 128])
def test_pytree_route_is_the_slab_route(cuda, K):
    x, offs = emnist_round(K)
    clients = separate_clients(x, offs, cuda)
    assert clients[0]["conv2_d_1"]["w"].data_ptr() % 16 == 4  # the misaligned view
    before = [flat_of(c) for c in clients[:2]]
    template = tmap(lambda s: torch.zeros(s), EMNIST_64)
    s = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    s.rows.copy_(torch.from_numpy(np.array(x)))
    t = tu.kernels.trim_count(0.1, K)
    for trim, tt in ((0.1, t), (0, 0)):
        want = ref.trimmed_mean(x, tt)
        tree = tu.tree_trimmed_mean(iter(clients), trim)  # a one-shot iterable, consumed once
        assert pytree.flatten(tree)[1] == pytree.flatten(template)[1]
        assert tree["zero"].numel() == 0 and tree["one"].numel() == 1
        assert_bits(flat_of(tree), want, f"tree K={K} trim={trim}")
        assert_bits(flat_of(s.trimmed_mean(trim)), want, f"slab K={K} trim={trim}")
    want = ref.median(x)
    assert_bits(flat_of(tu.tree_median(clients)), want, "tree_median")
    assert_bits(flat_of(s.median()), want, "slab median")
    # the aggregators: the same bits, and the weights change nothing
    for agg, w in ((fedjax_amd.aggregators.trimmed_mean_aggregator(0.1), ref.trimmed_mean(x, t)),
                   (fedjax_amd.aggregators.median_aggregator(), want)):
        state = agg.init()
        for weight in (1, 17, 0.5):
            got, state2 = agg.apply(((f"c{k}", c, weight * (1 + k % 3)) for k, c in enumerate(clients)), state)
            assert state2 is state
            assert_bits(flat_of(got), w, f"aggregator weight {weight}")
    for c, b in zip(clients[:2], before):  # inputs unchanged
        assert_bits(flat_of(c), b, "inputs")


def test_pytree_capture_raises_and_slab_capture_replays(cuda):
    K = 12
    template = {"w": torch.zeros(4099), "b": torch.zeros(5)}
    s = slab_mod.ClientDeltaSlab(template, K, device=cuda).fill_synthetic(seed=1)
    out = torch.zeros(s.num_params, device=cuda)
    s.trimmed_mean(2, out=out)  # eager once: the kernel is loaded before the capture
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = s.trimmed_mean(2, out=out)
    for seed in (2, 3):
        s.fill_synthetic(seed=seed)
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert_bits(flat_of(res), flat_of(s.trimmed_mean(2)), f"replay with seed {seed}")
        assert_bits(flat_of(res), ref.trimmed_mean(s.rows.cpu().numpy(), 2), f"replay {seed} restatement")
    clients = [tmap(lambda v: v.clone(), s.client(k)) for k in range(K)]
    g1, st1 = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st1):
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g1, stream=st1):
                tu.tree_trimmed_mean(clients, 2)
    torch.cuda.synchronize()
    assert_bits(flat_of(tu.tree_trimmed_mean(clients, 2)), ref.trimmed_mean(s.rows.cpu().numpy(), 2),
                "eager after the refused capture")


# -------------------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing(cuda):
    x = torch.zeros(4, 64, device=cuda)
    big = torch.zeros(129, 8, device=cuda)
    with pytest.raises(ValueError, match="128"):
        kernels.trim_dense(big, 1)
    with pytest.raises(TypeError, match="float32"):
        kernels.trim_dense(x.to(torch.bfloat16), 1)
    with pytest.raises(ValueError, match="2t < K"):
        kernels.trim_dense(x, 2)
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 129, device=cuda)
    with pytest.raises(ValueError, match="128"):
        s.trimmed_mean(1)
    b = slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 4, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        b.median()
    with pytest.raises(ValueError, match="128"):
        tu.tree_median([{"w": torch.zeros(2, device=cuda)}] * 129)
    with pytest.raises(TypeError, match="float32"):
        tu.tree_trimmed_mean([{"w": torch.zeros(2, device=cuda, dtype=torch.int32)}] * 4, 1)
    from fedjax_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.fjagg_trim_dense(_lib.F32, big.data_ptr(), 8, 129, 8, 1, 1.0, x.data_ptr(), 0, st) == -3
    assert lib.fjagg_trim_dense(_lib.BF16, x.data_ptr(), 64, 4, 64, 1, 1.0, x.data_ptr(), 0, st) == -3
    assert lib.fjagg_trim_dense(_lib.F32, x.data_ptr(), 64, 4, 64, 2, 1.0, x.data_ptr(), 0, st) == -1
    torch.cuda.synchronize()  # no pending HIP error, and a following valid call passes
    y = normal(4, 64, seed=8)
    assert_bits(kernels.trim_dense(on_device(y, cuda), 1, scale=0.5), ref.trimmed_mean(y, 1), "after the refusals")


# ----------------------------------------------------------------------------- 7. seeded sweep
def test_seeded_sweep(cuda):
    cases = ref.sweep_cases()
    assert len(cases) == 60
    for i, (K, t, leaves, seed) in enumerate(cases):
        P = max(sum(leaves), 1)
        x = ref.mixed_data(np.random.RandomState(seed), K, P)
        want = ref.trimmed_mean(x, t)
        assert_bits(kernels.trim_dense(on_device(x, cuda, ld=P + (i % 3)), t, scale=scale_of(K, t)), want,
                    f"case {i} dense K={K} t={t} P={P}")
        if sum(leaves) == 0:
            leaves = leaves + [1]
        offs = np.concatenate([[0], np.cumsum(leaves)])
        clients = []
        for k in range(K):
            row = torch.from_numpy(x[k]).to(cuda)
            # leaves of a client as views into its row (any element offset), or their own tensors
            clients.append({f"l{j}": (row[offs[j]:offs[j + 1]] if (i + k) % 2 else row[offs[j]:offs[j + 1]].clone())
                            for j in range(len(leaves))})
        got = tu.tree_trimmed_mean(clients, t)
        assert_bits(torch.cat([got[f"l{j}"] for j in range(len(leaves))]), want[:offs[-1]],
                    f"case {i} tree K={K} t={t} leaves={leaves}")
