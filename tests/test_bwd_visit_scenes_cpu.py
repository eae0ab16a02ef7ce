"""The scenes of tests/bwd_visit_scenes.py are what tests/test_gpu_bwd_visit.py needs them to be (CPU oracle only): the list of
tile (0, 0) has the constructed length and order; every entry of a full tile is blended by some pixels and by fewer than a
wave holds (so the wave that visits it has lanes that skip it); anchor A's entries are blended in the upper left quadrant and
by the first survivor wave only, anchor B's in the lower right quadrant and by the second (so an entry on B between two on A
is a recursion-only visit for A's wave, and the other way round); the hyperbolic entries have an indefinite conic, are blended
by some pixel and have `power > 0` in others of the same wave; the plain variant's oracle gradients are finite, and the
planted variants leave the image finite wherever the planted entry is not blended."""
import pytest
import torch

import bwd_visit_scenes as vs
from parity_common import fwd_args, run_backend


def _ranks_blending(mask_words):
    ranks = []
    for wd in range(8):
        m = int(mask_words[wd]) & 0xFFFFFFFF
        ranks += [32 * wd + b for b in range(32) if (m >> b) & 1]
    return ranks


def _forward(oracle, sc, kw, tile):
    oracle.TILE = tile
    oracle.lib().oracle_set_record(1)
    try:
        r = (oracle.rasterize_language_gaussians if sc.F > 0 else oracle.rasterize_gaussians)(*fwd_args(sc, None, **kw))
    finally:
        oracle.lib().oracle_set_record(0)
    return r


@pytest.mark.parametrize("tile", sorted(vs.IMAGES))
def test_lists_and_who_blends_what(oracle, tile):
    F = 3
    for N, (W, H), variant, bg in vs.cases(tile):
        sc, kw, info = vs.make(N, tile, F, W, H, "plain", bg)
        r = _forward(oracle, sc, kw, tile)
        geom = r[4]
        ranges = oracle.get_field(geom, "ranges").view(-1, 2)
        pl = oracle.get_field(geom, "point_list")
        cm = oracle.get_field(geom, "contrib_mask").view(-1, 8)
        conic = oracle.get_field(geom, "conic_opacity").view(-1, 4)
        xy = oracle.get_field(geom, "means2D").view(-1, 2)
        r0, r1 = int(ranges[0, 0]), int(ranges[0, 1])
        where = f"N{N} {W}x{H}"
        # Gaussian i is list position i of tile (0, 0); on the 17 x 17 image the REFERENCE's bounding squares also bring the
        # edge strips' splats into this list (the product's exact lists do not hold them), which blend nothing here
        mine = [k for k in range(r0, r1) if int(pl[k]) < N]
        assert [int(pl[k]) for k in mine] == list(range(N)), where
        assert r1 - r0 == N or (W, H) == (17, 17), where
        for i in range(N):
            ranks = _ranks_blending(cm[mine[i]])
            assert 0 < len(ranks) < 49, (where, i, len(ranks))  # blended, and by fewer lanes than the smallest wave has pixels
            rows, cols = {q // tile for q in ranks}, {q % tile for q in ranks}
            if info["anchor"][i] == 0:
                assert max(rows) < 7 and max(cols) < 7, (where, i, ranks)   # upper left quadrant, ranks below 112
            elif i in info["hyper"]:
                pass  # (blended along its asymptotes, which may cross the whole tile: checked below)
            else:
                assert min(rows) >= 8 and min(cols) >= 8, (where, i, ranks)  # lower right quadrant, ranks from 120
            if i in info["hyper"]:
                a, b, c = (float(conic[i, k]) for k in range(3))
                assert a * c - b * b < 0.0, (where, i)
                # `power > 0` in a pixel of the lower right quadrant (both survivor-wave and quadrant-wave of the blending pixels)
                px = torch.arange(8, tile, dtype=torch.float32)
                dx = float(xy[i, 0]) - px.view(1, -1)
                dy = float(xy[i, 1]) - px.view(-1, 1)
                power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
                assert bool((power > 0).any()) and bool((power <= 0).any()), (where, i)
        assert N < 64 or info["hyper"], where
        oracle.release(geom)


@pytest.mark.parametrize("tile", sorted(vs.IMAGES))
@pytest.mark.parametrize("mode", [0, 1])
def test_what_the_oracle_makes_of_the_planted_rows(oracle, tile, mode):
    F = 3
    for N, (W, H), _variant, bg in vs.cases(tile):
        for variant in vs.VARIANTS:
            sc, kw, info = vs.make(N, tile, F, W, H, variant, bg)
            fo, go = run_backend(oracle, sc, None, N, tile, mode, **kw)
            where = f"N{N} {W}x{H} {variant} m{mode}"
            if variant == "plain":
                for k in ("color", "language", "depth"):
                    assert bool(torch.isfinite(fo[k]).all()), (where, k)
                for k, t in go.items():
                    assert bool(torch.isfinite(t).all()), (where, k)
            else:
                # depth and opacity never see a colour; the image is non-finite in a few pixels only (those that blend a planted row)
                assert bool(torch.isfinite(fo["depth"]).all()), where
                bad = ~torch.isfinite(fo["color"]).all(0)
                assert 0 < int(bad.sum()) <= 9 * len(info["planted"]), (where, int(bad.sum()))  # (a splat reaches 3 x 3 pixels at most)
            oracle.release(fo["geom"])
