"""The numpy restatement of keyframe seeding (tests/keyframe_seed_ref.py) against what the reference computes on the CPU
(tests/golden/keyframe_seed.npz, recorded by tests/golden/make_golden_keyframe_seed.py): RGB2SH of the 256 byte colours,
inverse_sigmoid(0.5) and getWorld2View2 of three poses.  Open3D is not installed where the golden file was recorded, so the
back-projection (create_from_rgbd_image) and the count rule of random_down_sample are pinned by the restatement alone — the
GPU tests compare the kernels with it, not with Open3D.  The sampling hash is checked for what the contract needs of it:
unique keys, an exact count, and no gross non-uniformity."""
import os

import numpy as np

import keyframe_seed_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_seed.npz"))


def test_colour_table_and_opacity_equal_the_reference_bit_for_bit():
    table = R.colour_table()
    assert table.dtype == np.float32 and GOLD["rgb2sh_table"].dtype == np.float32
    assert np.array_equal(table.view(np.uint32), GOLD["rgb2sh_table"].view(np.uint32))
    # opacities are 0.0f = inverse_sigmoid(0.5)
    assert GOLD["opacity_half"].dtype == np.float32 and float(GOLD["opacity_half"][0]) == 0.0


def test_w2c_use_matches_getWorld2View2():
    """w2c is row-major world-to-camera, [R | t] as getWorld2View2 builds it: a camera-space point back-projected by the
    restatement (Rt (p - t)) and mapped forward again with the reference's matrix returns to where it started."""
    rng = np.random.default_rng(7)
    W, H, fx, fy, cx, cy = 64, 48, 40.0, 42.0, 30.5, 22.25
    for k in range(3):
        Rm, T, w2c = GOLD[f"pose{k}_R"], GOLD[f"pose{k}_T"], GOLD[f"pose{k}_w2c"]
        assert w2c.dtype == np.float32 and w2c.shape == (4, 4)
        # (the reference inverts twice; its matrix is [R | t] up to that rounding)
        np.testing.assert_allclose(w2c[:3, :3], Rm, atol=2e-6)
        np.testing.assert_allclose(w2c[:3, 3], T, atol=2e-6)
        np.testing.assert_allclose(w2c[3], [0, 0, 0, 1], atol=2e-6)   # (the kernels never read this row)
        u, v = rng.integers(0, W, 200), rng.integers(0, H, 200)
        z = rng.uniform(0.3, 6.0, 200).astype(np.float32)
        world = R.back_project(u, v, z, w2c, fx, fy, cx, cy).astype(np.float64)
        cam = world @ w2c[:3, :3].astype(np.float64).T + w2c[:3, 3].astype(np.float64)
        expect = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z.astype(np.float64)], axis=1)
        # R is orthonormal to float32 only: |R Rt - I| ~ 1e-7 times |p - t| < 10, plus the float32 narrowing of `world`
        np.testing.assert_allclose(cam, expect, atol=2e-5)


def test_keys_are_unique_and_the_sample_has_the_exact_size():
    rng = np.random.default_rng(3)
    for (W, H, factor) in ((40, 24, 8), (67, 45, 8), (64, 48, 1), (200, 150, 32), (1200, 680, 64)):
        N = W * H
        for seed in (0, 1, 12345, 0xFFFFFFFF):
            keys = R.sample_keys(N, seed)
            assert keys.dtype == np.uint32 and np.unique(keys).size == N
        image = np.full((3, H, W), 0.5, dtype=np.float32)
        depth = rng.uniform(0.3, 6.0, (H, W)).astype(np.float32)
        depth[rng.random((H, W)) < 0.2] = 0.0
        ref = R.seed_rows_ref(image, depth, np.eye(4, dtype=np.float32), (W / 2, W / 2, W / 2, H / 2), downsample=factor,
                              seed=5, knn=lambda p: np.ones(p.shape[0], dtype=np.float32))
        assert ref["n_valid"] == int((depth > 0).sum())
        assert ref["n_keep"] == int(ref["n_valid"] * (1.0 / factor)) <= N // factor
        assert int(ref["keep"].sum()) == ref["n_keep"] == ref["pix_index"].size
        assert np.all(np.diff(ref["pix_index"]) > 0) and np.all(depth.ravel()[ref["pix_index"]] > 0)


def test_sample_is_uniform_over_image_blocks():
    """64 x 48, factor 8, seeds 0..7, a 4 x 4 grid of blocks of 16 x 12 pixels: the kept count of a block is hypergeometric
    (n_keep of N without replacement, K = 192 of them in the block).  The worst |z| over the 8 x 16 cells, measured when this
    was written: 3.15.  The bound 4.5 is a guard against a broken hash, not a tolerance."""
    W, H, factor = 64, 48, 8
    N = W * H
    n_keep = R.n_keep_of(N, factor)
    K = (W // 4) * (H // 4)
    mean = n_keep * K / N
    var = n_keep * (K / N) * (1 - K / N) * (N - n_keep) / (N - 1)
    worst = 0.0
    for seed in range(8):
        keys = R.sample_keys(N, seed)
        keep = keys <= np.sort(keys)[n_keep - 1]
        assert int(keep.sum()) == n_keep
        blocks = keep.reshape(4, H // 4, 4, W // 4).sum(axis=(1, 3))
        worst = max(worst, float(np.abs((blocks - mean) / np.sqrt(var)).max()))
    print("worst block |z| =", worst)
    assert worst < 4.5, worst
