"""The forward composite's hit records (k_render_fwd.hip): a wave keeps the records of a 128-entry batch in one vector register
- lane l holds entries 2 l and 2 l + 1, written by v_writelane_b32 - zeroes it per batch and writes it to LDS once behind the
entry loop; the flush turns the records into flags[], blended[], n_touched and tile_work.

The scenes of tests/fwd_hit_scenes.py aim at what that storage can get wrong (tests/test_fwd_hit_records_cpu.py proves on the
oracle's record that they produce these conditions): entries at batch positions 62, 63, 64, 65, 126 and 127 - the register's
lane boundaries and the end of a batch - blended by exactly one wave (each of the four), by all four, by none; a wave whose
last pixel saturates at each of those positions; an entry blended at position p of batch 0 and not at position p of batch 1
(records not cleared between batches fail every stale_* case: batch 1 reports batch 0's waves), and the reverse; lists of odd
length throughout, so the last pair of every list is half sentinel.

Both binnings (the positions above are those of the reference's lists, where Gaussian i is list position i; the exact lists
may drop an entry no pixel blends and then hold the others one position earlier), 15 x 15 and 16 x 16 tiles, F = 0, 15, 32: the images, final_T, n_contrib, radii, n_touched, flags, tile_work,
blended and the live-row counts equal the oracle's, by the criteria of tests/test_gpu_fwd_batches.py (whose helpers these are).
"""
import pytest
import torch

import fwd_hit_scenes as hs
from parity_common import run_forward
from test_gpu_fwd_batches import (BINNINGS, DEV, _assert_decisions_equal_oracle, _assert_images_equal, _decisions, _live_rows,
                                  _oracle_forward)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("F", hs.F_VALUES)
@pytest.mark.parametrize("tile", hs.TILES)
def test_hit_records_at_lane_and_batch_boundaries_equal_the_oracle(hip, oracle, tile, F):
    dev = torch.device(DEV)
    n = 0
    for case in hs.cases(tile):
        cid = hs.case_id(tile, F, case)
        sc = hs.make(case, tile, F)
        fo, rec = _oracle_forward(oracle, sc, tile)
        d = {}
        for name, binning in BINNINGS:
            f, _ = run_forward(hip, sc, dev, tile, 0, binning)
            live = _live_rows(hip)
            _assert_images_equal(f, fo, f"{cid}:{name}")
            d[name] = _decisions(hip, f, sc, tile)
            d[name]["live_rows"] = live
        _assert_decisions_equal_oracle(d, fo, rec, sc, tile, cid)
        n += 1
    print(f"hit records: {n} cases")
