"""Seeded sweep of the compression aggregators (fedjax_amd/aggregators/compression.py over
fedjax_amd/csrc/fjcomp.hip) against the oracle (oracle/compression_ref.py), over the cases of
tests/compression_cases.py: tree structures whose leaf sizes take the rotated and the DRIVE
workspaces off 16-byte alignment, every placement of a leaf, client counts around the load group
and the 256-client staging, num_levels on both sides of the level table and of the LDS
histogram, batches that do not divide K, every kind of weight, and special values.

Bar: two rounds; after each, every element of the mean is NaN where the oracle's is and equal bit
for bit elsewhere (NaN payload and sign are not part of the contract: numpy's 0/0 and the GPU's
0 * inf differ there), ``num_bits`` is equal as a float32 value (or NaN on both sides) and ``rng``
is equal. A case the product refuses fails, unless the oracle refuses it too.
"""
import numpy as np
import numpy.testing as npt
import pytest
import torch

from fedjax_amd import pytree
from fedjax_amd.aggregators import compression as comp
from tests import compression_cases as cc

pytestmark = pytest.mark.gpu
SEEDS = range(7000, 7040)
F32 = np.float32


def product_aggregator(c):
    kw = {} if c["workspace_bytes"] is None else {"workspace_bytes": c["workspace_bytes"]}
    kind, key = c["kind"], c["key"]
    if kind == "uniform":
        return comp.uniform_stochastic_quantizer(c["num_levels"], key)
    if kind == "uniform_arith":
        return comp.uniform_stochastic_quantizer(c["num_levels"], key, "arithmetic")
    if kind == "rotated":
        return comp.rotated_uniform_stochastic_quantizer(cc.ROTATED_LEVELS, key, **kw)
    if kind == "drive":
        return comp.structured_drive_quantizer(key, **kw)
    return comp.terngrad_quantizer(key)


def assert_same_mean(got, want, what):
    """NaN where the oracle has NaN, the same bits everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    npt.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    npt.assert_array_equal(np.where(gn, F32(0), got).view(np.uint32), np.where(wn, F32(0), want).view(np.uint32),
                           err_msg=what)


def assert_same_bits_count(got, want, what):
    g, w = F32(got), F32(want)
    assert (np.isnan(g) and np.isnan(w)) or g == w, f"{what}: num_bits {g!r} != {w!r}"


def check_rounds(agg, clients, expected, what):
    state = agg.init()
    for r, (leaves, num_bits, rng) in enumerate(expected):
        mean, state = agg.apply(iter(clients), state)
        got = [x.cpu().numpy() for x in pytree.leaves_of(mean)]
        assert len(got) == len(leaves), what
        for l, (a, b) in enumerate(zip(got, leaves)):
            assert_same_mean(a, b, f"{what} round {r} leaf {l}")
        assert_same_bits_count(state.num_bits, num_bits, f"{what} round {r}")
        npt.assert_array_equal(np.asarray(state.rng, np.uint32), rng, err_msg=f"{what} round {r}: rng")


@pytest.mark.parametrize("seed", SEEDS)
def test_compression_case(seed, cuda):
    c = cc.case(seed)
    try:
        expected = cc.reference(c)
    except Exception as e:  # the oracle refuses the case: so must the product, with the same kind of error
        with pytest.raises(type(e)):
            check_rounds(product_aggregator(c), [("c", t, w) for t, w in zip(cc.place(c, cuda), c["weights"])],
                         [(None, 0, None)], f"seed {seed}")
        return
    clients = [("c%d" % k, t, w) for k, (t, w) in enumerate(zip(cc.place(c, cuda), c["weights"]))]
    what = (f"seed {seed} {c['kind']} K={c['K']} sizes={c['sizes']} levels={c['num_levels']} batch={c['batch']} "
            f"weights={c['wkind']} special={c['special']}")
    check_rounds(product_aggregator(c), clients, expected, what)
    torch.cuda.synchronize()
