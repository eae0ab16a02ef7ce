"""Float32 numpy restatement of olsr_tsdf_integrate and of the surface extraction (include/olsr.h, "TSDF fusion"): the
statements of the reference kernel (tsdf-fusion/fusion.py:93-139, fusion3.py:181-290) one numpy operation each, every operand
float32, so that each intermediate is rounded where the kernel rounds it (no FMA, IEEE division).  The GPU tests hold the
kernels to this bit for bit; tests/test_tsdf_ref_golden.py holds this to arrays recorded from the reference's own CPU path
(tests/golden/tsdf.npz).  With the kernel's divergences from the reference kernel: integer voxel coordinates, cam_z > 0, the
pixel range check on the rounded float, the optional opacity mask.
"""
import os

import numpy as np

f32 = np.float32
COLOR_CONST = f32(256 * 256)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsdf.npz"))


def volume_geometry(vol_bnds, voxel_size):
    """fusion.py:30-42 -> (vol_dim int [3], vol_origin float32 [3], voxel_size, trunc_margin as Python floats)."""
    b = np.array(vol_bnds, dtype=np.float64)
    voxel_size = float(voxel_size)
    dim = np.ceil((b[:, 1] - b[:, 0]) / voxel_size).copy(order="C").astype(int)
    return dim, b[:, 0].copy(order="C").astype(np.float32), voxel_size, 5 * voxel_size


def roundf(x):
    """C roundf on a float32 array: half away from zero (x - trunc(x) is exact)."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        return (t + np.copysign((np.abs(x - t) >= f32(0.5)).astype(np.float32), x)).astype(np.float32)


def fold_colour(color_im):
    """fusion.py:221-222: [H,W,3] -> one float per pixel."""
    c = np.asarray(color_im).astype(np.float32)
    return np.floor(c[..., 2] * COLOR_CONST + c[..., 1] * f32(256) + c[..., 0]).astype(np.float32)


def unpack(v):
    """fusion.py:129-131 -> (b, g, r)."""
    b = np.floor(v / COLOR_CONST)
    g = np.floor((v - b * COLOR_CONST) / f32(256))
    r = v - b * COLOR_CONST - g * f32(256)
    return b, g, r


class Volume:
    """feature_dim: an int (float running means, feat [F,X,Y,Z]) or "rgb" (packed colour, feat [X,Y,Z]).  rounding: "cuda"
    (roundf, the kernels) or "numpy" (np.round, half to even: the reference's CPU path) for the packed colour."""

    def __init__(self, vol_dim, vol_origin, voxel_size, feature_dim, rounding="cuda", trunc_margin=None):
        assert rounding in ("cuda", "numpy")
        self.dim = tuple(int(d) for d in vol_dim)
        self.origin = np.asarray(vol_origin, dtype=np.float32)
        self.voxel_size = f32(voxel_size)
        self.trunc = f32(5 * float(voxel_size) if trunc_margin is None else trunc_margin)
        self.packed = feature_dim == "rgb"
        self.F = 1 if self.packed else int(feature_dim)
        self.rounding = rounding
        n = int(np.prod(self.dim))
        self.tsdf = np.ones(n, np.float32)
        self.weight = np.zeros(n, np.float32)
        self.feat = np.zeros((self.F, n), np.float32)

    def arrays(self):
        """tsdf, weight [X,Y,Z]; feat [F,X,Y,Z] (packed: [X,Y,Z])."""
        feat = self.feat.reshape((self.F,) + self.dim)
        return self.tsdf.reshape(self.dim), self.weight.reshape(self.dim), (feat[0] if self.packed else feat)

    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1.0, opacity=None, min_opacity=0.0, layout="rows",
                  voxels=None):
        """One view.  color_im: [H,W,F] (layout "rows") or [F,H,W] ("channels"); packed: [H,W,3].  voxels: linear indices to
        update (default: all).  -> the indices that were updated."""
        X, Y, Z = self.dim
        idx = np.arange(X * Y * Z, dtype=np.int64) if voxels is None else np.asarray(voxels, dtype=np.int64)
        depth_im = np.asarray(depth_im, dtype=np.float32)
        H, W = depth_im.shape
        K = np.asarray(cam_intr).astype(np.float32)
        P = np.asarray(cam_pose).astype(np.float32)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        obs = f32(obs_weight)
        vx, r = idx // (Y * Z), idx % (Y * Z)
        vy, vz = r // Z, r % Z
        with np.errstate(all="ignore"):
            pt_x = self.origin[0] + vx.astype(np.float32) * self.voxel_size
            pt_y = self.origin[1] + vy.astype(np.float32) * self.voxel_size
            pt_z = self.origin[2] + vz.astype(np.float32) * self.voxel_size
            tx, ty, tz = pt_x - P[0, 3], pt_y - P[1, 3], pt_z - P[2, 3]
            cam_x = P[0, 0] * tx + P[1, 0] * ty + P[2, 0] * tz
            cam_y = P[0, 1] * tx + P[1, 1] * ty + P[2, 1] * tz
            cam_z = P[0, 2] * tx + P[1, 2] * ty + P[2, 2] * tz
            px = roundf(fx * (cam_x / cam_z) + cx)
            py = roundf(fy * (cam_y / cam_z) + cy)
            ok = (cam_z > 0) & (px >= 0) & (px < f32(W)) & (py >= 0) & (py < f32(H))
            pix = np.where(ok, py, 0).astype(np.int64) * W + np.where(ok, px, 0).astype(np.int64)
            depth = depth_im.reshape(-1)[pix]
            ok &= ~(depth == 0)
            if opacity is not None:
                ok &= ~(np.asarray(opacity, dtype=np.float32).reshape(-1)[pix] < f32(min_opacity))
            diff = depth - cam_z
            ok &= ~(diff < -self.trunc)
            dist = np.fmin(f32(1), diff / self.trunc)
            sel, pix, dist = idx[ok], pix[ok], dist[ok]
            w_old = self.weight[sel]
            w_new = w_old + obs
            self.weight[sel] = w_new
            self.tsdf[sel] = (self.tsdf[sel] * w_old + obs * dist) / w_new
            if self.packed:
                rnd = roundf if self.rounding == "cuda" else np.round
                old_b, old_g, old_r = unpack(self.feat[0, sel])
                new_b, new_g, new_r = unpack(fold_colour(color_im).reshape(-1)[pix])
                new_b = np.fmin(rnd((old_b * w_old + obs * new_b) / w_new), f32(255))
                new_g = np.fmin(rnd((old_g * w_old + obs * new_g) / w_new), f32(255))
                new_r = np.fmin(rnd((old_r * w_old + obs * new_r) / w_new), f32(255))
                self.feat[0, sel] = new_b * COLOR_CONST + new_g * f32(256) + new_r
            elif self.F > 0:
                im = np.asarray(color_im, dtype=np.float32)
                im = im.reshape(self.F, H * W) if layout == "channels" else im.reshape(H * W, self.F).T
                for c in range(self.F):
                    self.feat[c, sel] = (self.feat[c, sel] * w_old + obs * im[c, pix]) / w_new
        assert self.tsdf.dtype == self.weight.dtype == self.feat.dtype == np.float32
        return sel

    def surface(self, min_weight=0.0):
        """-> (points [N,3], feats [N,F] (packed: r, g, b), voxel_index int32 [N]) in voxel order, then axis."""
        return surface(*self.arrays(), self.origin, self.voxel_size, min_weight, self.packed)


def surface(tsdf, weight, feat, origin, voxel_size, min_weight=0.0, packed=False):
    """The extraction of include/olsr.h on [X,Y,Z] arrays (feat [F,X,Y,Z], or [X,Y,Z] packed), vectorised."""
    X, Y, Z = tsdf.shape
    origin, voxel_size = np.asarray(origin, dtype=np.float32), f32(voxel_size)
    neg = tsdf < 0
    seen = (weight >= f32(min_weight)) if min_weight > 0 else np.ones_like(neg)
    cross = np.zeros((X, Y, Z, 3), bool)
    cross[:-1, :, :, 0] = (neg[:-1] != neg[1:]) & seen[:-1] & seen[1:]
    cross[:, :-1, :, 1] = (neg[:, :-1] != neg[:, 1:]) & seen[:, :-1] & seen[:, 1:]
    cross[:, :, :-1, 2] = (neg[:, :, :-1] != neg[:, :, 1:]) & seen[:, :, :-1] & seen[:, :, 1:]
    v, axis = np.nonzero(cross.reshape(-1, 3))          # row-major: voxel order, then axis
    stride = np.array([Y * Z, Z, 1], dtype=np.int64)[axis]
    flat = tsdf.reshape(-1)
    t0, t1 = flat[v], flat[v + stride]
    coords = np.stack([v // (Y * Z), (v % (Y * Z)) // Z, v % Z], axis=1).astype(np.float32)
    pos = coords.copy()
    rows = np.arange(len(v))
    with np.errstate(all="ignore"):
        pos[rows, axis] = coords[rows, axis] + t0 / (t0 - t1)
    nearest = np.where(np.rint(pos[rows, axis]) == coords[rows, axis] + f32(1), v + stride, v)
    points = (pos * voxel_size + origin).astype(np.float32)
    if packed:
        b, g, r = unpack(feat.reshape(-1)[nearest])
        feats = np.stack([r, g, b], axis=1).astype(np.float32)
    else:
        feats = feat.reshape(feat.shape[0], -1)[:, nearest].T.copy() if feat is not None and feat.shape[0] else np.zeros((len(v), 0), np.float32)
    assert pos.dtype == points.dtype == np.float32
    return points, feats, v.astype(np.int32)
