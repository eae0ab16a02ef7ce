"""tests/bwd_sums_ref.py checks itself (no GPU): every sum of the model agrees with the exact sum within the bound of its
own depth, d * 2^-24 * sum |x|, and the model tells summation orders apart - for inputs of mixed magnitude its bits differ
from those of the orders a wrong kernel would have.  The latter is the evidence that the equalities of
tests/test_gpu_bwd_sums.py would fail for such a kernel."""
import math

import numpy as np
import pytest

import bwd_sums_ref as ref

F32 = np.float32
EPS = 2.0 ** -24


def _mixed(rng, shape):
    """values over twelve binades, both signs: almost every float32 addition of two of them rounds"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-6, 6, size=shape))).astype(F32)


def _cancelling(rng, n, cols):
    """pairs x, -x in random places plus small noise: the exact sum is tiny beside sum |x|"""
    half = _mixed(rng, (n // 2, cols))
    x = np.concatenate([half, -half, (1e-6 * rng.standard_normal((n - 2 * (n // 2), cols))).astype(F32)], 0)
    return x[rng.permutation(x.shape[0])]


def _fsum_cols(x):
    x = np.asarray(x, dtype=np.float64)
    return (np.array([math.fsum(x[:, c].tolist()) for c in range(x.shape[1])]),
            np.array([math.fsum(np.abs(x[:, c]).tolist()) for c in range(x.shape[1])]))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def _sequential(x):
    acc = np.zeros(x.shape[1], dtype=F32)
    for r in x:
        acc = acc + r
    return acc


INPUTS = ("random", "cancelling")


def _make(kind, rng, n, cols):
    return _mixed(rng, (n, cols)) if kind == "random" else _cancelling(rng, n, cols)


@pytest.mark.parametrize("kind", INPUTS)
def test_wave_tree_within_its_bound(kind):
    rng = np.random.default_rng(1)
    x = _make(kind, rng, 64, 40)                       # 40 independent waves, one per column
    got = ref.wave_tree(np.ascontiguousarray(x.T))
    assert got.shape == (40, 64) and (_bits(got) == _bits(got[:, :1])).all(), "the butterfly leaves every lane the same bits"
    exact, mag = _fsum_cols(x)
    assert (np.abs(got[:, 0].astype(np.float64) - exact) <= 6 * EPS * mag).all()


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("n", [1, 2, 12, 48, 63, 64, 65, 129, 700])
def test_row_sums_within_their_bounds(kind, n):
    rng = np.random.default_rng(100 + n)
    ROW = ref.grad_row(15)
    rows = _make(kind, rng, n + 7, ROW)
    first, nrows = np.array([3, 0, 7]), np.array([n, min(n, 5), n])
    for fn, depth in ((ref.inline_row_sum, lambda k: k), (ref.wave_row_sum, lambda k: (k + 63) // 64 + 6)):
        got = fn(rows, first, nrows)
        assert got.dtype == F32 and got.shape == (3, ROW)
        for i in range(3):
            exact, mag = _fsum_cols(rows[first[i]:first[i] + nrows[i]])
            assert (np.abs(got[i].astype(np.float64) - exact) <= depth(int(nrows[i])) * EPS * mag).all(), (fn.__name__, i)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 127, 128, 129, 5000, 32768, 32769, 65613, 300001])
def test_tau_sum_within_its_bound(kind, P):
    rng = np.random.default_rng(P)
    x = _make(kind, rng, P, 6)
    got = ref.tau_sum(x)
    exact, bound = ref.tau_sum_bound(x)
    e2, mag = _fsum_cols(x)
    nb = (P + 127) // 128
    assert ref.tau_sum_depth(P) == 8 + (nb + 255) // 256 + 10
    assert (exact == e2).all() and np.allclose(bound, ref.tau_sum_depth(P) * EPS * mag, rtol=1e-15)
    assert got.dtype == F32 and got.shape == (6,)
    assert (np.abs(got.astype(np.float64) - exact) <= bound).all()


def test_the_model_tells_orders_apart():
    rng = np.random.default_rng(7)
    # the two row sums on 65 rows
    rows = _mixed(rng, (65, ref.grad_row(3)))
    a, b = ref.inline_row_sum(rows, [0], [65]), ref.wave_row_sum(rows, [0], [65])
    assert (_bits(a) != _bits(b)).any()
    # dL_dtau_sum against a plain sequential sum, against a lost tail block and against a final stride of 64
    P = 128 * 300 + 5                                      # 301 partials: the final pass takes two strides, the tail block has 5
    x = _mixed(rng, (P, 6))
    want = ref.tau_sum(x)
    assert (_bits(want) != _bits(_sequential(x))).any()
    part = ref.tau_partials(x)
    assert part.shape == (301, 6) and (_bits(ref.tau_final(part)) == _bits(want)).all()
    assert (_bits(ref.tau_final(part[:-1])) != _bits(want)).any(), "a lost tail block goes unnoticed"
    assert (_bits(ref.tau_final(part, stride=64)) != _bits(want)).any(), "a final stride of 64 goes unnoticed"
    # the lost tail block is far inside the 1e-4 band that held dL_dtau_sum before: only the equality sees it
    small = x.copy()
    small[-5:] *= F32(1e-5)
    w2, p2 = ref.tau_sum(small), ref.tau_partials(small)
    lost = ref.tau_final(p2[:-1])
    assert np.abs(lost.astype(np.float64) - w2).max() <= 1e-4 * np.abs(w2).max()
    assert (_bits(lost) != _bits(w2)).any()


def test_edge_cases():
    ROW = ref.grad_row(0)
    rng = np.random.default_rng(3)
    rows = _mixed(rng, (140, ROW))
    # empty runs give +0.0 in both paths
    for fn in (ref.inline_row_sum, ref.wave_row_sum):
        z = fn(rows, [5, 0], [0, 0])
        assert (_bits(z) == 0).all()
        assert fn(rows, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)).shape == (0, ROW)
    # one row: both paths return it (0 + x, then x + 0 up the tree)
    assert (_bits(ref.inline_row_sum(rows, [9], [1])) == _bits(rows[9:10])).all()
    assert (_bits(ref.wave_row_sum(rows, [9], [1])) == _bits(rows[9:10])).all()
    # 64 rows: one row per lane, the wave sum is the tree of the rows; 65: lane 0 adds its second row first
    t64 = ref.wave_tree(np.ascontiguousarray(rows[3:67].T))[:, 0]
    assert (_bits(ref.wave_row_sum(rows, [3], [64])[0]) == _bits(t64)).all()
    lanes = rows[3:67].copy()
    lanes[0] = lanes[0] + rows[67]
    t65 = ref.wave_tree(np.ascontiguousarray(lanes.T))[:, 0]
    assert (_bits(ref.wave_row_sum(rows, [3], [65])[0]) == _bits(t65)).all()
    assert (_bits(t64) != _bits(t65)).any()
    # -0.0 rows: the sums start from +0.0, so the result is +0.0
    neg = np.full((70, ROW), -0.0, dtype=F32)
    assert (_bits(neg) == 0x80000000).all()
    assert (_bits(ref.inline_row_sum(neg, [0], [12])) == 0).all() and (_bits(ref.wave_row_sum(neg, [0], [70])) == 0).all()
    assert (_bits(ref.tau_sum(np.full((200, 6), -0.0, dtype=F32))) == 0).all()
    # P = 1 and P = 0
    one = _mixed(rng, (1, 6))
    assert (_bits(ref.tau_sum(one)) == _bits(one[0])).all()
    assert (_bits(ref.tau_sum(np.zeros((0, 6), dtype=F32))) == 0).all()
    # float64 input is refused, not silently rounded
    with pytest.raises(TypeError):
        ref.tau_sum(np.zeros((4, 6)))


def _frame(rng, F_rows, tiles, rows_per_tile):
    """a made-up frame: Gaussian i is listed in tiles[i] tiles with rows_per_tile[i][k] live rows in its k-th instance;
    emission order is the reverse index order, so inst_start is not monotonic"""
    P = len(tiles)
    ROW = ref.grad_row(F_rows)
    inst_start = np.zeros(P, dtype=np.int32)
    per_inst = []
    for i in reversed(range(P)):
        inst_start[i] = len(per_inst)
        per_inst += list(rows_per_tile[i])
    rowbase = np.concatenate([[0], np.cumsum(per_inst)]).astype(np.uint32)
    rows = _mixed(rng, (int(rowbase[-1]) + 3, ROW))
    return ROW, inst_start, rowbase, rows


def test_composite_level_paths_and_layout():
    rng = np.random.default_rng(11)
    tiles = [1, 12, 13, 40, 13, 5, 7, 20]
    per = [[2], [1] * 12, [2] * 13, [2] * 40, [0] * 13, [0] * 5, [1] * 7, [2] * 20]
    radii = np.array([3, 9, 9, 30, 9, 4, 0, 9], dtype=np.int32)          # Gaussian 6 culled
    blended = np.array([1, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)         # Gaussian 7 blended nowhere: its rows are not looked up
    for F_rows, F_out in ((0, 0), (3, 3), (15, 15), (0, 15), (32, 32)):
        ROW, inst_start, rowbase, rows = _frame(rng, F_rows, tiles, per)
        out = ref.composite_level(rows.reshape(-1), ROW, F_rows, F_out, len(tiles), radii, blended, np.array(tiles),
                                  inst_start, rowbase)
        assert out["has_rows"].tolist() == [True, True, True, True, False, False, False, False]
        assert out["nrows"].tolist() == [2, 12, 26, 80, 0, 0, 0, 0]
        run = lambda i: rows[rowbase[inst_start[i]]: rowbase[inst_start[i] + tiles[i]]]  # noqa: E731
        acc = np.zeros((len(tiles), ROW), dtype=F32)
        for i in (0, 1):
            acc[i] = _sequential(run(i))
        for i in (2, 3):
            acc[i] = ref.wave_row_sum(rows, [rowbase[inst_start[i]]], [len(run(i))])[0]
        assert (_bits(out["dL_dmeans2D"]) == _bits(np.stack([acc[:, 0], acc[:, 1], np.zeros(len(tiles), dtype=F32)], 1))).all()
        assert (_bits(out["dL_dconic"]) == _bits(np.stack([acc[:, 2], acc[:, 3], np.zeros(len(tiles), dtype=F32), acc[:, 4]], 1))).all()
        assert (_bits(out["dL_dopacity"][:, 0]) == _bits(acc[:, 5])).all()
        assert (_bits(out["dL_dcolors"]) == _bits(acc[:, 6:9])).all() and (_bits(out["dL_ddepths"][:, 0]) == _bits(acc[:, 9])).all()
        assert out["dL_dlanguage"].shape == (len(tiles), F_out)
        if F_rows:
            assert (_bits(out["dL_dlanguage"]) == _bits(acc[:, 10:10 + F_rows])).all()
        else:
            assert (_bits(out["dL_dlanguage"]) == 0).all()
        n = ref.densify_norm(acc[:, 0], acc[:, 1], radii)
        assert n[6] == 0 and n[4] == 0 and n[0] == np.sqrt(F32(acc[0, 0] * acc[0, 0]) + F32(acc[0, 1] * acc[0, 1]))
    with pytest.raises(ValueError):
        ref.composite_level(rows.reshape(-1), ROW, 32, 32, len(tiles), radii, blended, np.array(tiles), inst_start, rowbase,
                            activations=1)
    with pytest.raises(ValueError):
        ref.composite_level(rows.reshape(-1), ROW, 32, 32, len(tiles), radii, blended, np.array(tiles), inst_start, rowbase,
                            conic_opacity=np.array([[1.0, 0.0, np.nan, 0.5]]))
    with pytest.raises(ValueError):
        ref.composite_level(rows.reshape(-1), ROW + 4, 32, 32, len(tiles), radii, blended, np.array(tiles), inst_start, rowbase)


def test_launch_geometry_restated():
    assert ref.rr_nwaves(4000) == 1024 and ref.rr_nwaves(500_000) == 4 * 8192 and ref.rr_nwaves(65536) == 4 * 4096
    assert [ref.grad_row(F) for F in (0, 3, 15, 16, 32)] == [12, 16, 28, 28, 44]


@pytest.mark.parametrize("tile", [15, 16])
def test_the_row_sum_scene_reaches_every_path(oracle, tile):
    """tests/bwd_sums_scenes.py before any GPU sees it: with the oracle's recorded forward (which Gaussian blended in which
    tile) and the float64 model of the ellipse binning (core <= listed <= may), the frame has what tests/test_gpu_bwd_sums.py
    asserts of it - whatever the kernel lists between core and may."""
    import bwd_sums_scenes as bs
    f = bs.facts(tile)
    P, core, may, rec = f["P"], f["n_core"], f["n_may"], f["recorded"]
    sure = core == may                                     # the model leaves the footprint no choice
    assert 3500 <= P <= 4500 and sure.mean() >= 0.99
    for k in bs.TILE_COUNTS:
        assert int((sure & (core == k) & (rec > 0)).sum()) >= 10, k
    nwaves = ref.rr_nwaves(P)
    assert nwaves == 1024
    listed = core > ref.MID_FOOTPRINT                      # listed whatever the kernel decides inside the band
    assert int(listed.sum()) >= 2 * nwaves + 1
    assert int((core > ref.BIG_FOOTPRINT).sum()) > 0 and int((listed & (may <= ref.BIG_FOOTPRINT)).sum()) > 0
    # a row per (instance, wave of pixels) that blended: at least one per recorded tile
    assert int((rec >= 65).sum()) >= 10
    norow = listed & (rec == 0)
    assert int(norow.sum()) >= 50
    has = (rec > 0)[listed | (may > ref.MID_FOOTPRINT)]
    assert int((np.diff(has.astype(np.int8)) != 0).sum()) >= 100, "no-row Gaussians are not interleaved in index order"
    assert int(may.sum()) <= 150_000, "the GPU test's instance capacity"
    print(f"tile {tile}: P={P} listed>={int(listed.sum())} big>={int((core > 32).sum())} without rows>={int(norow.sum())} "
          f"instances<={int(may.sum())}")
