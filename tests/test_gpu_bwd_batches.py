"""The backward composite's staging batches (k_render_bwd.hip: 64 list entries per LDS fill for the reference mode with at
most 16 language channels, 128 otherwise).  The per-pixel state lives across batches, so a batch boundary must not show in any
result: lists of 1, 63, 64, 65, 127, 128, 129 and 200 entries that all blend (tests/bwd_batch_scenes.py), alone and
interleaved with entries only the lower half of the tile blends, for every F, both modes, both tile sizes, with and without a
background.

Asserted per case: the parity suite's criteria against the CPU oracle (forward bit-identical; every gradient within 1e-4 of
its tensor's largest magnitude; the composite-level gradients per element, worst element within 2e-4; the ordered kernel
equal to the oracle and the fast kernel within 64 x 2^-24 x condition of it), and bit-equality of every gradient with
tests/golden/bwd_batches.npz, recorded from the build before the batch was a template parameter
(tests/golden/make_golden_bwd_batches.py).
"""
import os

import numpy as np
import pytest
import torch

import bwd_batch_scenes as bs
from parity_common import assert_backward_criteria, run_backend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwd_batches.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {str(i): d for i, d in zip(z["ids"], z["sha256"])}


@pytest.mark.parametrize("F", bs.F_VALUES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tile", bs.TILES)
def test_batch_boundaries_change_no_bit(hip, oracle, golden, tile, mode, F):
    dev = torch.device(DEV)
    for N, lower, bg in bs.cases(tile, F):
        cid = bs.case_id(tile, mode, F, N, lower, bg)
        sc, fam = bs.make(N, tile, F, lower, bg)
        fo, go = run_backend(oracle, sc, None, N, tile, mode)
        fg, gg = run_backend(hip, sc, dev, N, tile, mode)
        torch.cuda.synchronize()
        # the list of tile (0, 0) has the constructed length in the product's exact binning too
        W = H = 2 * tile
        rg = hip.state_field("image", fg["img"], "ranges", W=W, H=H, dtype=torch.int32, count=8).cpu()
        assert int(rg[1] - rg[0]) == len(fam), cid
        for k in ("color", "language", "depth", "opacity"):
            if fo[k] is not None and fo[k].numel():
                assert torch.equal(fg[k].cpu(), fo[k]), f"{cid}: forward {k}"
        assert_backward_criteria(hip, sc, fg, gg, go, N, tile, mode, cid, rtol=RTOL)
        oracle.release(fo["geom"])
        assert np.array_equal(bs.digest(gg), golden[cid]), f"{cid}: gradients differ in bits from the recorded build"
