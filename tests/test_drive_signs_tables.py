"""Host tables of DRIVE's transmitted form (fedjax_amd._compress.DriveSignsLayout): byte counts,
workspace offsets, tile prefixes and batch sizes at the GPU test's leaf sizes. No GPU needed."""
import numpy as np

from fedjax_amd import _compress as C
from fedjax_amd import _lib

SIZES = (1, 3, 8, 9, 31, 33, 4097, 8193, 2 ** 16 + 1, 2 ** 21 + 1)


def test_layout_at_the_edge_sizes():
    lay = C.DriveSignsLayout(SIZES)
    assert lay.d.tolist() == [1, 4, 8, 16, 32, 64, 8192, 16384, 2 ** 17, 2 ** 22]
    assert lay.nbytes.tolist() == [1, 1, 1, 2, 4, 8, 1024, 2048, 2 ** 14, 2 ** 19]
    assert lay.words.tolist() == [1, 1, 1, 1, 1, 2, 256, 512, 4096, 2 ** 17]
    # only the leaves above one 8192-element tile own workspace, back to back
    assert lay.ws_off.tolist() == [0] * 8 + [16384, 16384 + 2 ** 17] and lay.D == 16384 + 2 ** 17 + 2 ** 22
    assert lay.client_bytes == 4 * lay.D + 4 * int(lay.words.sum())
    # pass 0 of every multi-pass leaf (d / 8192 tiles); pass 1 only of the three-pass leaf
    assert len(lay.pass_prefix) == 2
    assert np.diff(lay.pass_prefix[0]).tolist() == [0] * 7 + [2, 16, 512]
    assert np.diff(lay.pass_prefix[1]).tolist() == [0] * 9 + [512]
    # the last pass: one workgroup per single-pass leaf, d / 8192 per other leaf
    assert np.diff(lay.single_prefix).tolist() == [1] * 7 + [0] * 3
    assert np.diff(lay.multi_prefix).tolist() == [0] * 7 + [2, 16, 512]
    lib = _lib.load()
    for m, tiles in zip(lay.m, np.diff(lay.multi_prefix) + np.diff(lay.single_prefix)):
        assert tiles == lib.fjcomp_wht_tiles(int(m), C.wht_passes(int(m)) - 1)


def test_batches_follow_the_budget():
    lay = C.DriveSignsLayout(SIZES[:9])
    per = lay.client_bytes
    assert [lay.batch(5, b) for b in (0, per, 2 * per, 3 * per - 1, 1 << 40)] == [1, 1, 2, 2, 5]
    small = C.DriveSignsLayout(SIZES[:7])  # single-pass leaves only: no workspace, the signs alone count
    assert small.D == 0 and small.pass_prefix == [] and small.client_bytes == 4 * int(small.words.sum())
    assert small.batch(300, 2 * small.client_bytes) == 2
