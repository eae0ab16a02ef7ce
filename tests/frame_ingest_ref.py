"""The numpy restatement of a frame's ingest (include/olsr_frame_ingest.h), the reference of tests/test_gpu_frame_ingest.py;
tests/golden/frame_ingest.npz pins it to the reference's own statements (tests/test_frame_ingest_ref_golden.py).

  image [3,H,W] float32 = float32(clamp(float64(byte) / 255.0, 0, 1))       depth [H,W] float32 = float32(float64(d) / depth_scale)
"""
import numpy as np


def ingest(rgb_u8, depth, depth_scale):
    """rgb_u8 uint8 [H,W,3], depth uint16 or float32 [H,W] -> (image float32 [3,H,W], depth float32 [H,W])."""
    rgb_u8, depth = np.asarray(rgb_u8), np.asarray(depth)
    assert rgb_u8.dtype == np.uint8 and rgb_u8.ndim == 3 and rgb_u8.shape[2] == 3
    assert depth.dtype in (np.uint16, np.float32) and depth.shape == rgb_u8.shape[:2]
    image = np.clip(rgb_u8.astype(np.float64) / np.float64(255.0), 0.0, 1.0).transpose(2, 0, 1).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (depth.astype(np.float64) / np.float64(depth_scale)).astype(np.float32)
    return np.ascontiguousarray(image), d


def synthetic_frame(W, H, depth_dtype, seed):
    """A byte image that holds all 256 values in each channel when W H >= 256, and a depth with the values 0, 1 and the
    largest one of its type (uint16: 65535) among random ones."""
    rng = np.random.default_rng(seed)
    n = W * H
    i = np.arange(n)
    rgb = np.stack([i % 256, (255 - i) % 256, (i * 7 + 3) % 256], axis=1).astype(np.uint8)
    if n > 256:
        rgb[256:] = rng.integers(0, 256, size=(n - 256, 3), dtype=np.uint8)
    if depth_dtype == np.uint16:
        depth = rng.integers(0, 65536, size=n).astype(np.uint16)
        special = [0, 1, 65535]
    else:
        depth = (rng.random(n) * 12.0).astype(np.float32)
        special = [0.0, 1.0, 65535.0]
    for k, v in enumerate(special):
        if k < n:
            depth[(k * 5) % n] = v
    return rgb.reshape(H, W, 3), depth.reshape(H, W)
