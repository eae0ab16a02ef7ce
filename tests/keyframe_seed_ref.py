"""numpy restatement of keyframe seeding (include/olsr.h, "keyframe seeding"; csrc/k_keyframe_seed.hip): float64 where the
contract says double, float32 everywhere else, one rounding per written operation.  The kNN is scene.knn_mean_dist2_host
(the bits of olsr_knn_mean_dist2); log(sqrt(.)) of the scales is float64 here — the tests bound the kernel's logf against it.
exp(a) of the exposure is the library's pinned exp, taken from the CPU oracle (oracle_expf_probe: the same bits for every
argument in [-87, 88])."""
import numpy as np

f32 = np.float32
C0 = f32(0.28209479177387814)
DEPTH_TRUNC = 100.0


def fmix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def sample_keys(N, seed):
    with np.errstate(over="ignore"):
        s = np.uint32((int(seed) & 0xFFFFFFFF) * 0x9E3779B9 & 0xFFFFFFFF)
        return fmix32(np.arange(N, dtype=np.uint32) ^ s)


def n_keep_of(n_valid, downsample):
    return int(np.float64(n_valid) * (np.float64(1.0) / np.float64(downsample)))


def masked_depth(image, depth, rgb_boundary_threshold=0.01):
    """d' = rgb_ok ? depth : 0 (add_new_keyframe), float32 [H,W]."""
    image = np.asarray(image, dtype=f32)
    rgb_ok = ((image[0] + image[1]) + image[2]) > f32(rgb_boundary_threshold)
    return np.where(rgb_ok, np.asarray(depth, dtype=f32), f32(0.0)).astype(f32)


def valid_mask(dp, depth_trunc=DEPTH_TRUNC):
    with np.errstate(invalid="ignore"):
        return (dp > f32(0.0)) & (dp < f32(depth_trunc))


def median_depth(dp):
    """The median of d' over all pixels; non-finite or negative d' counts as 0.  Odd count: the middle element; even:
    fl32(fl32(a + b) / 2)."""
    with np.errstate(invalid="ignore"):
        x = np.where(np.isfinite(dp) & (dp > 0), dp, f32(0.0)).astype(f32).ravel()
    x = np.sort(x)
    N = x.size
    if N % 2:
        return f32(x[N // 2])
    with np.errstate(over="ignore"):
        return f32(f32(x[N // 2 - 1] + x[N // 2]) / f32(2.0))


def point_size_of(median, point_size=0.05, adaptive=True):
    if not adaptive:
        return f32(point_size)
    return f32(min(0.05, float(point_size) * float(np.float64(median))))


def colour_table():
    """f_dc of the 256 byte values: RGB2SH(byte / 255) in float32."""
    colour = np.arange(256, dtype=f32) / f32(255.0)
    return ((colour - f32(0.5)) / C0).astype(f32)


def colour_bytes(img, exposure=None, expf=None):
    """(uint8)(clamp(exp(a) img + b, 0, 1) * 255), truncating; exposure None: the image as it is."""
    c = np.asarray(img, dtype=f32)
    if exposure is not None:
        ea = f32(expf(float(f32(exposure[0]))))
        c = (ea * c).astype(f32) + f32(exposure[1])
        c = np.minimum(np.maximum(c, f32(0.0)), f32(1.0)).astype(f32)
    return (c * f32(255.0)).astype(f32).astype(np.uint8)


def back_project(u, v, z32, w2c, fx, fy, cx, cy):
    """Open3D's back-projection in double, then Rt (p - t) with the float32 entries of w2c widened; narrowed once."""
    w = np.asarray(w2c, dtype=f32).astype(np.float64).reshape(4, 4)
    z = z32.astype(np.float64)
    x = (u.astype(np.float64) - np.float64(cx)) * z / np.float64(fx)
    y = (v.astype(np.float64) - np.float64(cy)) * z / np.float64(fy)
    q = [x - w[0, 3], y - w[1, 3], z - w[2, 3]]
    out = np.empty((z.size, 3), dtype=f32)
    for k in range(3):
        out[:, k] = ((w[0, k] * q[0] + w[1, k] * q[1]) + w[2, k] * q[2]).astype(f32)
    return out


def seed_rows_ref(image, depth, w2c, intrinsics, *, downsample, seed, exposure=None, rgb_boundary_threshold=0.01,
                  point_size=0.05, adaptive_pointsize=True, M=1, depth_trunc=DEPTH_TRUNC, expf=None, knn=None):
    """Everything seed_rows returns, as numpy arrays; `scale_arg` = max(d2, 1e-7) * ps in float32 and `scales64` =
    log(sqrt(scale_arg)) in float64 (n >= 4 only)."""
    image = np.asarray(image, dtype=f32)
    H, W = image.shape[1:]
    fx, fy, cx, cy = intrinsics
    dp = masked_depth(image, depth, rgb_boundary_threshold)
    valid = valid_mask(dp, depth_trunc).ravel()
    n_valid = int(valid.sum())
    median = median_depth(dp)
    ps = point_size_of(median, point_size, adaptive_pointsize)
    n_keep = n_keep_of(n_valid, downsample)
    keys = sample_keys(W * H, seed)
    keep = np.zeros(W * H, dtype=bool)
    if n_keep > 0:
        thr = np.sort(keys[valid])[n_keep - 1]
        keep = valid & (keys <= thr)
    pix = np.nonzero(keep)[0].astype(np.int32)
    table = colour_table()
    flat = image.reshape(3, -1)
    shs = np.zeros((pix.size, M, 3), dtype=f32)
    for c in range(3):
        shs[:, 0, c] = table[colour_bytes(flat[c, pix], exposure, expf)]
    means = back_project(pix % W, pix // W, dp.ravel()[pix], w2c, fx, fy, cx, cy)
    out = dict(n_valid=n_valid, n_keep=n_keep, median_depth=median, point_size=ps, pix_index=pix, means3D=means, shs=shs,
               opacities=np.zeros((pix.size, 1), dtype=f32), keep=keep, keys=keys,
               rotations=np.tile(np.array([1, 0, 0, 0], dtype=f32), (pix.size, 1)))
    if n_keep >= 4:
        if knn is None:
            import torch
            from online_lang_splatting_amd.scene import knn_mean_dist2_host
            knn = lambda p: knn_mean_dist2_host(torch.from_numpy(p)).numpy()  # noqa: E731
        d2 = np.asarray(knn(means), dtype=f32)
        arg = (np.maximum(d2, f32(1e-7)) * ps).astype(f32)
        with np.errstate(divide="ignore"):   # (ps = 0: log(0) = -inf, as in the reference)
            out.update(d2=d2, scale_arg=arg, scales64=np.log(np.sqrt(arg.astype(np.float64))))
    return out
