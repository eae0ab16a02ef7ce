"""tests/tsdf_ref.py against tests/golden/tsdf.npz: volumes recorded from the reference's own fusion.TSDFVolume(use_gpu=False)
(tests/golden/make_golden_tsdf.py) on four posed views with noisy depth, zero-depth pixels and random 8-bit colour.  The
restatement is float32 in the kernels' statement order; the reference's CPU path goes through float64 camera coordinates and
rounds half to even, so
  - the weights (the update decisions) must be equal everywhere,
  - the tsdf must agree within twice the largest error measured when the file was made (stored in it; the margin covers
    another libm or numpy),
  - the packed colour with rounding="numpy" may differ on at most 0.05 % of the voxels.
The extraction is held to a triple loop over a tiny volume.  This file validates the yardstick of tests/test_gpu_tsdf.py; it
involves no kernel."""
import numpy as np
import pytest

import tsdf_ref as R


@pytest.fixture(scope="module")
def Z():
    return R.golden()


@pytest.fixture(scope="module")
def fused(Z):
    dim, origin, voxel, _ = R.volume_geometry(Z["vol_bnds"], float(Z["voxel_size"]))
    vols = {r: R.Volume(dim, origin, voxel, "rgb", rounding=r) for r in ("numpy", "cuda")}
    for k in range(Z["depths"].shape[0]):
        for v in vols.values():
            v.integrate(Z["colours"][k], Z["depths"][k], Z["cam_intr"], Z["cam_poses"][k], obs_weight=float(Z["obs_weights"][k]))
    return vols


def test_constructor_arithmetic(Z):
    dim, origin, voxel, trunc = R.volume_geometry(Z["vol_bnds"], float(Z["voxel_size"]))
    assert np.array_equal(dim, Z["vol_dim"]) and origin.dtype == np.float32 and np.array_equal(origin, Z["vol_origin"])
    assert trunc == 5 * float(Z["voxel_size"])
    # the ceil: a bound that is no multiple of the voxel size gains a voxel
    assert tuple(R.volume_geometry([[0, 0.1001], [0, 0.1], [-1, 1]], 0.05)[0]) == (3, 2, 40)


def test_weights_are_the_references(Z, fused):
    _, w, _ = fused["numpy"].arrays()
    assert w.dtype == np.float32 and np.array_equal(w, Z["weight"])
    assert int((w > 0).sum()) > 0.5 * w.size and int((w == 0).sum()) > 0.1 * w.size   # both kinds of voxel are present


def test_tsdf_within_twice_the_recorded_error(Z, fused):
    t, _, _ = fused["numpy"].arrays()
    err = float(np.abs(t.astype(np.float64) - Z["tsdf"].astype(np.float64)).max())
    bound = 2.0 * float(Z["tsdf_max_abs_err"])
    print(f"tsdf max abs err {err:.3e}, recorded {float(Z['tsdf_max_abs_err']):.3e}, bound {bound:.3e}")
    assert 0.0 < bound < 5e-6 and err <= bound
    assert int(((Z["tsdf"][:-1] < 0) != (Z["tsdf"][1:] < 0)).sum()) > 50   # the fixture has a surface


def test_packed_colour_with_numpy_rounding(Z, fused):
    c = fused["numpy"].arrays()[2]
    differs = int((c != Z["colour"]).sum())
    print(f"packed colour: {differs} of {c.size} voxels differ (recorded {int(Z['colour_differs_numpy'])})")
    assert differs <= 0.0005 * c.size
    # half away from zero instead of half to even moves the exact .5 means: expected, recorded, not an error
    cuda = int((fused["cuda"].arrays()[2] != Z["colour"]).sum())
    print(f"packed colour, rounding=\"cuda\": {cuda} voxels differ (recorded {int(Z['colour_differs_cuda'])})")
    assert cuda == int(Z["colour_differs_cuda"])


def test_roundf_is_half_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, -0.49999997, 2.4, -2.6, 8388609.0, 0.0], np.float32)
    want = np.array([1, 2, 3, -1, -2, 0, -0, 2, -3, 8388609, 0], np.float32)
    assert np.array_equal(R.roundf(x), want)


def _brute_force(tsdf, weight, feat, origin, voxel, min_weight, packed):
    X, Y, Z_ = tsdf.shape
    pts, fts, own = [], [], []
    for x in range(X):
        for y in range(Y):
            for z in range(Z_):
                for a, (dx, dy, dz) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                    x1, y1, z1 = x + dx, y + dy, z + dz
                    if x1 >= X or y1 >= Y or z1 >= Z_:
                        continue
                    t0, t1 = tsdf[x, y, z], tsdf[x1, y1, z1]
                    if (t0 < 0) == (t1 < 0):
                        continue
                    if min_weight > 0 and not (weight[x, y, z] >= min_weight and weight[x1, y1, z1] >= min_weight):
                        continue
                    pos = np.array([x, y, z], np.float32)
                    pos[a] = np.float32(pos[a] + np.float32(t0 / np.float32(t0 - t1)))
                    n = tuple(int(v) for v in np.round(pos))
                    pts.append((pos * np.float32(voxel) + origin).astype(np.float32))
                    if packed:
                        b, g, r = R.unpack(feat[n])
                        fts.append(np.array([r, g, b], np.float32))
                    else:
                        fts.append(feat[(slice(None),) + n])
                    own.append((x * Y + y) * Z_ + z)
    F = 3 if packed else feat.shape[0]
    return (np.array(pts, np.float32).reshape(-1, 3), np.array(fts, np.float32).reshape(-1, F), np.array(own, np.int32))


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
@pytest.mark.parametrize("packed", [False, True])
def test_extraction_against_a_triple_loop(min_weight, packed):
    rng = np.random.default_rng(3)
    dim = (5, 4, 6)
    tsdf = rng.uniform(-1, 1, dim).astype(np.float32)
    tsdf[2, 1, 3] = 0.0                                  # a zero counts as non-negative
    weight = rng.integers(0, 3, dim).astype(np.float32)
    feat = (rng.integers(0, 1 << 24, dim).astype(np.float32) if packed else rng.normal(size=(3,) + dim).astype(np.float32))
    origin = np.array([-0.3, 0.2, 1.1], np.float32)
    got = R.surface(tsdf, weight, feat, origin, 0.04, min_weight, packed)
    want = _brute_force(tsdf, weight, feat, origin, 0.04, min_weight, packed)
    assert len(want[2]) > 20
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_extraction_of_a_volume_without_a_crossing():
    dim = (3, 2, 2)
    pts, fts, own = R.surface(np.ones(dim, np.float32), np.zeros(dim, np.float32), np.zeros((15,) + dim, np.float32),
                              np.zeros(3, np.float32), 0.02)
    assert pts.shape == (0, 3) and fts.shape == (0, 15) and own.shape == (0,)
