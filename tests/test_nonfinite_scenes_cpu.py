"""What the oracle alone says about the planted scenes of tests/nonfinite_scenes.py (CPU; tests/test_gpu_nonfinite.py holds
the HIP rasteriser to it).  Every scene runs forward and backward in both backward modes without an exception and under the
instance cap; the planting is contained (no other Gaussian's radius changes, no pixel outside the planted Gaussians' tile
rects changes a bit); and each class does what the table says, so that a class cannot silently test nothing.

TABLE_TEXT below is the table, per class at P = 257 on 45 x 30, tile 15, F = 15, planted in rows 64 and 256: the oracle's
radii of the two planted rows; instances (num_rendered minus the unplanted scene's 588); (pixel, entry) visits in which a planted
row is blended; and the rows with a non-finite element in dL_dmeans2D / dL_dopacity / dL_dmeans3D (BWD_REFERENCE), first
among the planted rows, then among all others.  A class is either declared CULLED (every planted row has radius 0 although it
was visible before planting: what it tests is that the row disappears without a trace), declared TRANSPARENT (opacity <= 0: it
keeps its instances and passes no alpha test), or its planted rows must reach a pixel.

Two definitions the oracle takes where the reference's result is undefined ("Non-finite inputs"):
a Gaussian whose radius is 0 holds no instance (the reference counts a tile for it and writes no key: an uninitialised list
slot), and exp's float -> int conversion is the device's saturating one (0 for a NaN; `make -C oracle ubsan` runs these scenes
under UBSan + ASan).  A NaN conic (scale_1e12: the covariance has overflowed) makes `power` NaN in every pixel, exp(NaN) is
NaN, alpha = min(0.99, NaN) = 0.99: the Gaussian blends everywhere, as in the reference."""
import pytest
import torch

import nonfinite_scenes as N
from parity_common import run_backend, same_bits

ROWS = N.module_scenes()
IDS = [r[0] for r in ROWS]
CAP = 1 << 16
# classes whose planted rows the oracle culls (radius 0): a NaN or infinite mean fails no frustum test but gives a NaN
# determinant or pixel position; a NaN / infinite / 1e20 scale, a NaN or 1e20 rotation and a NaN or infinite covariance give a
# NaN eigenvalue, hence radius f2i_sat(NaN) = 0
CULLED = {"mean_nan_x", "mean_inf_z", "mean_ninf_y", "mean_negnan_z", "scale_nan", "scale_inf", "scale_1e20", "rot_nan", "rot_1e20",
          "cov_nan", "cov_inf", "raw_scale_89", "raw_nan_mean", "raw_nan_scale", "raw_nan_rot"}
# classes whose planted rows keep their radius and their instances but can pass no alpha test: opacity <= 0
TRANSPARENT = {"op_neg", "op_zero", "raw_op_ninf", "raw_op_m104"}
# classes whose planted rows cover every tile (a radius of 2^20 pixels or more): nothing lies outside their rect
SCREEN_FILLING = {"scale_1e12", "scale_below_2p20", "scale_above_2p20"}
GRAD_COLUMNS = ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D")


def _nonfinite_rows(g, P):
    return (~torch.isfinite(g.reshape(P, -1))).any(1)


def measure(oracle, row):
    """One line of the table."""
    p = N.scene_of(row)
    tile, sc = row[5], p.activated()
    out = N.oracle_forward(sc, tile, **p.kw)
    base = N.oracle_forward(p.activated("base"), tile, **p.base_kw)
    fo, go = run_backend(oracle, sc, None, 3, tile, 0, **p.kw)
    oracle.release(fo["geom"])
    planted = torch.zeros(sc.P, dtype=torch.bool)
    planted[p.idx] = True
    cols = []
    for k in GRAD_COLUMNS:
        nf = _nonfinite_rows(go[k], sc.P)
        cols.append(f"{int((nf & planted).sum())}+{int((nf & ~planted).sum())}")
    return (f"{row[1]:18s} radii {','.join(str(int(r)) for r in out['radii'][p.idx][:2]):>21s}  instances {out['R'] - base['R']:+4d}  "
            f"visits {int(out['reached'][p.idx].sum()):5d}  non-finite rows {' '.join(cols)}")


TABLE_TEXT = """
mean_nan_x         radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
mean_inf_z         radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
mean_ninf_y        radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
mean_negnan_z      radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
scale_nan          radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
scale_inf          radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
scale_1e20         radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
scale_1e12         radii 2147483647,2147483647  instances   +9  visits  1257  non-finite rows 1+0 1+0 2+0
scale_below_2p20   radii       1048575,1048575  instances   +9  visits  2700  non-finite rows 0+0 0+0 0+0
scale_above_2p20   radii       1048576,1048576  instances   +9  visits  2700  non-finite rows 0+0 0+0 0+0
scale_zero         radii                   3,3  instances   +0  visits    16  non-finite rows 0+0 0+0 0+0
scale_negative     radii                   3,5  instances   +0  visits    46  non-finite rows 0+0 0+0 0+0
rot_zero           radii                   3,5  instances   +0  visits    44  non-finite rows 0+0 0+0 0+0
rot_nan            radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
rot_1e20           radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
cov_nan            radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
cov_inf            radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
cov_zero           radii                   3,3  instances   +0  visits    16  non-finite rows 0+0 0+0 0+0
op_nan             radii                   3,5  instances   +0  visits   387  non-finite rows 2+0 0+0 2+0
op_inf             radii                   3,5  instances   +0  visits   387  non-finite rows 2+0 0+0 2+0
op_neg             radii                   3,5  instances   +0  visits     0  non-finite rows 0+0 0+0 0+0
op_zero            radii                   3,5  instances   +0  visits     0  non-finite rows 0+0 0+0 0+0
op_one             radii                   3,5  instances   +0  visits    52  non-finite rows 0+0 0+0 0+0
op_two             radii                   3,5  instances   +0  visits    58  non-finite rows 0+0 0+0 0+0
lang_nan           radii                   3,5  instances   +0  visits    46  non-finite rows 2+85 2+85 2+85
sh_inf             radii                   3,5  instances   +0  visits    46  non-finite rows 2+23 2+23 2+23
color_nan          radii                   3,5  instances   +0  visits    46  non-finite rows 2+23 2+23 2+23
raw_scale_89       radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
raw_scale_m104     radii                   3,3  instances   +0  visits    16  non-finite rows 0+0 0+0 0+0
raw_op_pinf        radii                   3,5  instances   +0  visits    52  non-finite rows 0+0 0+0 0+0
raw_op_ninf        radii                   3,5  instances   +0  visits     0  non-finite rows 0+0 0+0 0+0
raw_op_104         radii                   3,5  instances   +0  visits    52  non-finite rows 0+0 0+0 0+0
raw_op_m104        radii                   3,5  instances   +0  visits     0  non-finite rows 0+0 0+0 0+0
raw_rot_zero       radii                   3,5  instances   +0  visits    44  non-finite rows 0+0 0+0 0+0
raw_nan_mean       radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
raw_nan_scale      radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
raw_nan_rot        radii                   0,0  instances   -3  visits     0  non-finite rows 0+0 0+0 0+0
raw_nan_op         radii                   3,5  instances   +0  visits   387  non-finite rows 2+0 0+0 2+0
"""
TABLE = {line.split()[0]: line for line in TABLE_TEXT.strip().splitlines()}


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_oracle_runs_every_planted_scene_under_the_cap(oracle, row):
    """Forward and backward, both backward modes: no exception, num_rendered <= P x tiles and
    <= 2^16 (a condition, not a measurement: no GPU case of these scenes allocates more than a few MB whatever the library does)."""
    p = N.scene_of(row)
    tile, sc = row[5], p.activated()
    tiles = -(-row[3] // tile) * -(-row[4] // tile)
    for mode in (0, 1):
        fo, go = run_backend(oracle, sc, None, 3, tile, mode, **p.kw)
        oracle.release(fo["geom"])
        assert 0 <= fo["R"] <= min(sc.P * tiles, CAP), (row[0], fo["R"])
        assert all(g.shape[0] == sc.P for g in go.values())


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_planting_is_contained_in_the_oracle(oracle, row):
    """No Gaussian that is not planted changes its radius, and every pixel outside the tiles in which a planted Gaussian holds
    an instance — before or after planting — keeps the unplanted frame's bits."""
    p = N.scene_of(row)
    W, H, tile = row[3], row[4], row[5]
    out = N.oracle_forward(p.activated(), tile, **p.kw)
    base = N.oracle_forward(p.activated("base"), tile, **p.base_kw)
    keep = torch.ones(p.scene.P, dtype=torch.bool)
    keep[p.idx] = False
    assert torch.equal(out["radii"][keep], base["radii"][keep])
    tiles = N.planted_tiles(out, p.idx, p.scene.P) | N.planted_tiles(base, p.idx, p.scene.P)
    outside = ~N.pixel_mask_of_tiles(tiles, W, H, tile)
    for k in ("color", "language", "depth", "opacity"):
        if out[k] is not None and out[k].numel():
            assert same_bits(out[k][:, outside], base[k][:, outside]), (row[0], k)
    assert same_bits(out["final_T"].view(H, W)[outside], base["final_T"].view(H, W)[outside])
    if row[1] in N.KINDS and row[7] == "upper" and row[1] not in SCREEN_FILLING:
        assert int(outside.sum()) > 0, "the containment statement holds nothing: every tile holds a planted Gaussian"


@pytest.mark.parametrize("row", [r for r in ROWS if r[1] in N.KINDS and r[7] == "upper"], ids=lambda r: r[1])
def test_every_class_does_what_the_table_says(oracle, row):
    p = N.scene_of(row)
    out = N.oracle_forward(p.activated(), row[5], **p.kw)
    radii, reached = out["radii"][p.idx], out["reached"][p.idx]
    if row[1] in CULLED:
        assert bool((radii == 0).all()) and int(reached.sum()) == 0, row[1]
    elif row[1] in TRANSPARENT:
        assert bool((radii > 0).all()) and int(reached.sum()) == 0, row[1]
    else:  # (of two screen-filling rows that blend alpha = 0.99 the one behind may find every pixel saturated)
        assert bool((radii > 0).all()) and int(reached.sum()) > 0, f"{row[1]}: no planted Gaussian reaches a pixel"
    line = measure(oracle, row)
    print(line)
    assert line.split() == TABLE[row[1]].split(), f"measured:\n{line}\ntable:\n{TABLE[row[1]]}"


def test_the_table_lists_every_class():
    assert set(TABLE) == set(N.KINDS)
    assert (CULLED | TRANSPARENT | SCREEN_FILLING) <= set(N.KINDS) and not CULLED & TRANSPARENT


def test_radius_edge_is_the_hand_over():
    """The two scales of scale_below_2p20 / scale_above_2p20 are adjacent floats with radii 2^20 - 1 and 2^20 or more."""
    import numpy as np
    p = N.scene_of([r for r in ROWS if r[1] == "scale_below_2p20"][0])
    lo, hi = N.radius_edge(p.base, int(p.idx[0]))
    assert np.nextafter(np.float32(lo), np.float32(np.inf)) == np.float32(hi)
    q = N.scene_of([r for r in ROWS if r[1] == "scale_above_2p20"][0])
    r_lo = N.oracle_forward(p.scene, 15)["radii"][p.idx]
    r_hi = N.oracle_forward(q.scene, 15)["radii"][q.idx]
    assert bool((r_lo < (1 << 20)).all()) and bool((r_hi >= (1 << 20)).all()) and bool((r_lo > (1 << 19)).all())


def test_exp_of_nan_is_defined(oracle):
    """exp(NaN) is NaN through a defined conversion; the finite results did not move (tests/test_oracle_golden.py pins them)."""
    import math
    assert math.isnan(oracle.expf(float("nan")))
    assert oracle.expf(0.0) == 1.0 and oracle.expf(float("-inf")) == oracle.expf(-87.0)
