"""One visit of the backward composite (k_render_bwd.hip) on the scenes of tests/bwd_visit_scenes.py: entries that some lanes of
a wave blend and others skip (by the alpha floor, by `power > 0`, by `k >= last_contributor`), entries a wave visits only for
the language recursion, and entries with an infinite or NaN colour and language row that the skipping lanes must not touch; on
images of one tile, of 2 x 2 tiles and on a 17 x 17 image of 15-pixel tiles; lists of 1, 2, 3, 64 and 65 entries; every F,
both modes, both tiles, with and without a background.

Asserted per case: the parity suite's criteria against the CPU oracle - the forward bit-identical, the ordered kernel equal to
the oracle, the fast kernel within 64 x 2^-24 x condition of the ordered one - and bit-equality of every gradient with
tests/golden/bwd_visit.npz, recorded from the build before the kernel's LDS records and scalar row address
(tests/golden/make_golden_bwd_visit.py).  Where the reference itself is non-finite (the planted variants), the non-finite
positions must be the same and the criteria hold on the rest.
"""
import os

import numpy as np
import pytest
import torch

import bwd_visit_scenes as vs
from parity_common import (COMPOSITE_KEYS, assert_ordered_equals_oracle, assert_rounding_only, ordered_backward, run_backend,
                           same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwd_visit.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {str(i): d for i, d in zip(z["ids"], z["sha256"])}


def _finite_part(gfast, gord, gcond, where):
    """The three gradient sets with the positions zeroed where the ORDERED kernel (== the oracle) is non-finite; the fast kernel
    must be non-finite in exactly those positions."""
    out = ({}, {}, {})
    for k in COMPOSITE_KEYS:
        a, b, c = (t.detach().cpu().float() for t in (gfast[k], gord[k], gcond[k]))
        bad = ~torch.isfinite(b)
        assert torch.equal(~torch.isfinite(a), bad), f"{where}{k}: non-finite positions differ from the reference's"
        bad |= ~torch.isfinite(c)
        for o, t in zip(out, (a, b, c)):
            o[k] = torch.where(bad, torch.zeros_like(t), t)
    return out


@pytest.mark.parametrize("F", vs.F_VALUES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tile", sorted(vs.IMAGES))
def test_a_visit_changes_no_bit(hip, oracle, golden, tile, mode, F):
    dev = torch.device(DEV)
    for N, (W, H), variant, bg in vs.cases(tile):
        cid = vs.case_id(tile, mode, F, N, (W, H), variant, bg)
        sc, kw, info = vs.make(N, tile, F, W, H, variant, bg, plant_language=(mode == 1))
        fo, go = run_backend(oracle, sc, None, N, tile, mode, **kw)
        kwd = {k: v.to(dev) for k, v in kw.items()}
        fg, gg = run_backend(hip, sc, dev, N, tile, mode, **kwd)
        torch.cuda.synchronize()
        # the list of tile (0, 0) has the constructed length in the product's exact binning (on the 17 x 17 image the splats of
        # the two-pixel strips beside it may reach its last pixel column and row as well)
        rg = hip.state_field("image", fg["img"], "ranges", W=W, H=H, dtype=torch.int32, count=2).cpu()
        assert int(rg[1] - rg[0]) == N or ((W, H) == (17, 17) and N <= int(rg[1] - rg[0]) <= 4 * N), cid
        for k in ("color", "language", "depth", "opacity"):
            if fo[k] is not None and fo[k].numel():
                assert same_bits(fg[k], fo[k]), f"{cid}: forward {k}"
        gord = ordered_backward(hip, sc, fg, N, tile, mode, **kwd)
        assert_ordered_equals_oracle(go, gord, where=f"{cid}:ordered:")
        gcond = ordered_backward(hip, sc, fg, N, tile, mode, condition=True, **kwd)
        if variant == "plain":
            assert_rounding_only(gg, gord, gcond, k_bound=64.0, name=f"{cid}:")
        else:
            assert_rounding_only(*_finite_part(gg, gord, gcond, f"{cid}:"), k_bound=64.0, name=f"{cid}:")
        oracle.release(fo["geom"])
        assert np.array_equal(vs.digest(gg), golden[cid]), f"{cid}: gradients differ in bits from the recorded build"
