"""The scenes of tests/bwd_batch_scenes.py really are what tests/test_gpu_bwd_batches.py needs them to be (CPU oracle only):
the list of tile (0, 0) has the constructed length and order, every entry blends somewhere (nothing saturates, so the
backward walks the whole list), family 1 is blended by pixels of the upper AND of the lower half of the tile (and, in a
15 x 15 tile, by survivors of both packed waves), family 2 by the lower half only."""
import pytest
import torch

import bwd_batch_scenes as bs
from parity_common import fwd_args


def _ranks_blending(mask_words):
    ranks = []
    for wd in range(8):
        m = int(mask_words[wd]) & 0xFFFFFFFF
        ranks += [32 * wd + b for b in range(32) if (m >> b) & 1]
    return ranks


@pytest.mark.parametrize("tile", bs.TILES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("N", bs.N_VALUES)
def test_lists_have_the_intended_lengths(oracle, N, lower, tile):
    F = 3
    sc, fam = bs.make(N, tile, F, lower, bg=False)
    L = len(fam)
    assert fam.count(1) == N and (L == N if not lower else L == N + (N + 1) // 2 + bs.tail_of(N))
    oracle.TILE = tile
    oracle.lib().oracle_set_record(1)
    try:
        r = oracle.rasterize_language_gaussians(*fwd_args(sc))
    finally:
        oracle.lib().oracle_set_record(0)
    geom = r[4]
    ranges = oracle.get_field(geom, "ranges").view(-1, 2)
    pl = oracle.get_field(geom, "point_list")
    nc = oracle.get_field(geom, "n_contrib").view(2 * tile, 2 * tile)
    cm = oracle.get_field(geom, "contrib_mask").view(-1, 8)
    r0, r1 = int(ranges[0, 0]), int(ranges[0, 1])
    assert r1 - r0 == L
    assert pl[r0:r1].tolist() == list(range(L))            # Gaussian i is list position i
    assert int(nc[:tile, :tile].max()) == L                 # the deepest entry blends: the backward starts at the list's end
    half = 8                                                # rows 0-7: the upper quadrants / the first survivor wave
    rows1, packed_waves = set(), set()
    for i, f in enumerate(fam):
        ranks = _ranks_blending(cm[r0 + i])
        rows = {r // tile for r in ranks}
        assert rows, (i, f)
        if f == 1:
            rows1 |= rows
            # the survivors of the reference's reduction tree (rank % 7 in {0, 1, 3, 4}, rank < 224); ranks below 112 are wave 0
            packed_waves |= {int(r >= 112) for r in ranks if r < 224 and r % 7 in (0, 1, 3, 4)}
        else:
            assert min(rows) > half, (i, rows)
    if N >= 63:
        assert min(rows1) < half <= max(rows1), rows1
        assert tile != 15 or packed_waves == {0, 1}
    oracle.release(geom)
