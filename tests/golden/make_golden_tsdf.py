"""Generates tests/golden/tsdf.npz: the reference's OWN fusion.TSDFVolume(use_gpu=False) (tsdf-fusion/fusion.py) on a seeded
synthetic scene.  Runs ONLY where the reference checkout exists (OLSR_REFERENCE names it); the committed .npz is data (arrays
only).

What is executed from the reference: the constructor, integrate's CPU path (vox2world, rigid_transform, cam2pix,
integrate_tsdf and the colour statements) and get_volume, unmodified.  numba and skimage are not installed where this file
is made: `numba.njit` is stubbed as the identity and `prange` as range (the decorated functions are plain numpy loops),
`skimage.measure` as an empty module (marching cubes is not called), and pycuda's absence selects the CPU path by itself.
fusion3.py, the 15-channel variant, has no CPU path at all, so the float feature mode is pinned by restatement only: it is
the tsdf update's expression applied per channel.

The scene: a bumpy wall about 0.9 m in front of four cameras (small yaws and shifts), 40 x 30 images, depth with pixel noise
and 6 % zeros, random 8-bit colour, observation weights 1, 1, 0.5, 2; a 24 x 20 x 22 volume of 4 cm voxels.

Recorded: the inputs, the reference's tsdf / weight / colour volumes, and what tests/tsdf_ref.py (float32, the kernels'
statements) differs from them by: `tsdf_max_abs_err`, the number of voxels whose packed colour differs with rounding "numpy"
and with rounding "cuda".  The reference's CPU path computes the camera coordinates in float64 and rounds pixel coordinates
and colour means half to even, so the tsdf differs in the last bits and the "cuda" colour on the exact .5 means."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if "OLSR_REFERENCE" not in os.environ:
    raise SystemExit("set OLSR_REFERENCE to the reference checkout")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.environ["OLSR_REFERENCE"], "tsdf-fusion"))
import tsdf_ref as R  # noqa: E402

numba = types.ModuleType("numba")
numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
numba.prange = range
skimage = types.ModuleType("skimage")
skimage.measure = types.ModuleType("skimage.measure")
sys.modules.update({"numba": numba, "skimage": skimage, "skimage.measure": skimage.measure})

import fusion  # noqa: E402

SEED = 0
H, W = 30, 40
VOXEL = 0.04
BNDS = np.array([[-0.48, 0.48], [-0.40, 0.40], [0.30, 1.18]])
OBS = (1.0, 1.0, 0.5, 2.0)


def make_scene(seed=SEED):
    rng = np.random.default_rng(seed)
    K = np.array([[38.0, 0.0, (W - 1) / 2.0], [0.0, 38.0, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    poses, depths, colours = [], [], []
    for k in range(4):
        yaw = np.radians((k - 1.5) * 7.0)
        pose = np.eye(4)
        pose[:3, :3] = np.array([[np.cos(yaw), 0.0, np.sin(yaw)], [0.0, 1.0, 0.0], [-np.sin(yaw), 0.0, np.cos(yaw)]])
        pose[:3, 3] = [(k - 1.5) * 0.11, 0.03 * (k % 2), -0.05 + 0.04 * k]
        # the wall z = 0.9 + 0.06 sin(5 x) cos(4 y), hit along each pixel's ray (two fixed-point steps are plenty here)
        v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1) @ pose[:3, :3].T
        t = np.full((H, W), 0.9)
        for _ in range(3):
            p = pose[:3, 3] + ray * t[..., None]
            t = (0.9 + 0.06 * np.sin(5.0 * p[..., 0]) * np.cos(4.0 * p[..., 1]) - pose[2, 3]) / ray[..., 2]
        depth = t + rng.normal(0.0, 0.004, (H, W))
        depth[rng.random((H, W)) < 0.06] = 0.0
        poses.append(pose)
        depths.append(depth.astype(np.float32))
        colours.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return K, np.stack(poses), np.stack(depths), np.stack(colours)


def main():
    K, poses, depths, colours = make_scene()
    ref = fusion.TSDFVolume(BNDS.copy(), voxel_size=VOXEL, use_gpu=False)
    dim, origin, voxel, trunc = R.volume_geometry(BNDS, VOXEL)
    assert tuple(dim) == tuple(ref._vol_dim) and np.array_equal(origin, ref._vol_origin) and trunc == ref._trunc_margin
    mine = {r: R.Volume(dim, origin, voxel, "rgb", rounding=r) for r in ("numpy", "cuda")}
    for k in range(4):
        ref.integrate(colours[k], depths[k], K, poses[k], obs_weight=OBS[k])
        for m in mine.values():
            m.integrate(colours[k], depths[k], K, poses[k], obs_weight=OBS[k])
    tsdf, colour = ref.get_volume()
    weight = ref._weight_vol_cpu
    out = dict(seed=SEED, cam_intr=K, cam_poses=poses, depths=depths, colours=colours, vol_bnds=BNDS, voxel_size=VOXEL,
               obs_weights=np.array(OBS), vol_dim=np.asarray(dim), vol_origin=origin, tsdf=tsdf.astype(np.float32),
               weight=weight.astype(np.float32), colour=colour.astype(np.float32))
    t, w, c = mine["numpy"].arrays()
    n = t.size
    assert np.array_equal(w, weight), int((w != weight).sum())
    out["tsdf_max_abs_err"] = np.float64(np.abs(t.astype(np.float64) - tsdf.astype(np.float64)).max())
    out["colour_differs_numpy"] = int((c != colour).sum())
    out["colour_differs_cuda"] = int((mine["cuda"].arrays()[2] != colour).sum())
    print(f"{n} voxels, {int((weight > 0).sum())} updated, {int(((tsdf[:-1] < 0) != (tsdf[1:] < 0)).sum())} x crossings; "
          f"weights equal; tsdf max abs err {out['tsdf_max_abs_err']:.3e}; packed colour differs in "
          f"{out['colour_differs_numpy']} voxels (numpy rounding), {out['colour_differs_cuda']} (cuda rounding)")
    assert out["colour_differs_numpy"] <= 0.0005 * n
    np.savez_compressed(os.path.join(HERE, "tsdf.npz"), **out)


if __name__ == "__main__":
    main()
