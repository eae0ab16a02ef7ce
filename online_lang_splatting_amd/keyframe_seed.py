"""Host side of olsr_keyframe_seed_plan / _finish (include/olsr.h, csrc/k_keyframe_seed.hip): the rows of a keyframe's new
Gaussians from its RGB-D image, on the device.

Replaces FrontEnd.add_new_keyframe (utils/slam_frontend.py:106-132) + BackEnd.add_next_kf (utils/slam_backend.py:187-202) ->
GaussianModel.create_pcd_from_image / create_pcd_from_image_and_depth (gaussian_splatting/scene/gaussian_model.py:135-281),
which go through the host, Open3D and np.median.  Stated deviations from the reference (include/olsr.h has the arithmetic):
the sample is the `n_keep` valid pixels with the smallest hash keys, in pixel order (Open3D's shuffle is not reproduced);
the camera-to-world transform is Rt (p - t), not Eigen's 4x4 inverse; a NaN, infinite or negative depth counts as 0 in the
median (numpy would return NaN); with fewer than four kept pixels distCUDA2 has no three neighbours and no row is returned.
The monocular branch (random synthetic depth, gaussian_model.py:163-169) is out of scope.  GPU only."""
import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _abi
from ._host import stream_ptr
from ._lib import check, lib

DEPTH_TRUNC = 100.0   # create_from_color_and_depth(depth_trunc=100.0), gaussian_model.py:211


def staging_rows(W: int, H: int, downsample: int) -> int:
    """Rows that always hold the sample: n_keep <= (W H) / downsample, known without a host read."""
    return max((int(W) * int(H)) // int(downsample), 1)


def _need(cond, msg):
    if not cond:
        raise ValueError("seed_rows: " + msg)


def seed_rows(image: torch.Tensor, depth: torch.Tensor, w2c: torch.Tensor, intrinsics: Sequence[float], *, downsample: int,
              seed: int, exposure: Optional[torch.Tensor] = None, rgb_boundary_threshold: float = 0.01,
              point_size: float = 0.05, adaptive_pointsize: bool = True, M: int = 1, depth_trunc: float = DEPTH_TRUNC,
              staging: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """image [3,H,W] (rows contiguous, any plane stride), depth [H,W] or [1,H,W], w2c [4,4] world-to-camera (any strides),
    exposure float32[2] = {a, b} or None — float32 device tensors, taken as they lie; intrinsics = (fx, fy, cx, cy).

    Returns device tensors means3D [n,3], shs [n,M,3], opacities [n,1], scales [n,3], rotations [n,4], pix_index int32 [n]
    (the pixel v W + u of every row, ascending), n_valid int32 [], median_depth and point_size float32 [], and the Python
    int n_keep.  n = n_keep, or 0 when n_keep < 4.  Exactly one 4-byte host read (n_keep).

    staging: buffers of at least staging_rows(W, H, downsample) rows to build the rows in (means3D, shs, opacities, scales,
    rotations, pix_index; float32 / int32, contiguous); default: fresh ones."""
    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        raise RuntimeError("seed_rows: image, depth, w2c and exposure must be on the GPU (there is no CPU fallback)")
    dev = image.device
    _need(image.dim() == 3 and image.shape[0] == 3 and image.dtype == torch.float32, "image must be float32 [3,H,W]")
    H, W = int(image.shape[1]), int(image.shape[2])
    _need(H > 0 and W > 0, "image must not be empty")
    _need(image.stride(2) == 1 and image.stride(1) == W and image.stride(0) >= W * H, "image rows must be contiguous")
    _need(depth.device == dev and depth.dtype == torch.float32 and depth.numel() == W * H and depth.is_contiguous() and
          tuple(depth.shape[-2:]) == (H, W), "depth must be a contiguous float32 [H,W] on the image's device")
    _need(w2c.device == dev and w2c.dtype == torch.float32 and tuple(w2c.shape) == (4, 4),
          "w2c must be a float32 [4,4] on the image's device")
    w2c = w2c.contiguous()   # (torch.linalg.inv, which getWorld2View2 ends with, returns a column-major matrix: 64 bytes)
    if exposure is not None:
        _need(exposure.device == dev and exposure.dtype == torch.float32 and exposure.numel() == 2 and
              exposure.is_contiguous(), "exposure must be a contiguous float32 [2] = {a, b} on the image's device")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    _need(int(downsample) > 0 and int(M) >= 1, "downsample must be > 0 and M >= 1")
    cap = staging_rows(W, H, downsample)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    if staging is None:
        staging = dict(means3D=torch.empty(cap, 3, **f32), shs=torch.empty(cap, M, 3, **f32), opacities=torch.empty(cap, 1, **f32),
                       scales=torch.empty(cap, 3, **f32), rotations=torch.empty(cap, 4, **f32),
                       pix_index=torch.empty(cap, **i32))
    else:
        for k, tail in (("means3D", (3,)), ("shs", (M, 3)), ("opacities", (1,)), ("scales", (3,)), ("rotations", (4,)),
                        ("pix_index", ())):
            t = staging[k]
            _need(t.device == dev and t.is_contiguous() and t.shape[0] >= cap and tuple(t.shape[1:]) == tail and
                  t.dtype == (torch.int32 if k == "pix_index" else torch.float32), f"staging[{k!r}] does not fit")
        cap = min(int(staging[k].shape[0]) for k in ("means3D", "shs", "opacities", "scales", "rotations", "pix_index"))
    p = _abi.OlsrKeyframeSeedParams(W=W, H=H, plane_stride=int(image.stride(0)), M=int(M), downsample=int(downsample),
                                    seed=int(seed) & 0xFFFFFFFF, fx=fx, fy=fy, cx=cx, cy=cy,
                                    rgb_boundary_threshold=float(rgb_boundary_threshold), depth_trunc=float(depth_trunc),
                                    point_size=float(point_size), adaptive_pointsize=1 if adaptive_pointsize else 0,
                                    capacity=cap)
    rows = _abi.OlsrMapBuffers(**{k: staging[k].data_ptr() for k in ("means3D", "shs", "opacities", "scales", "rotations")})
    L = lib()
    scratch = torch.empty(int(L.olsr_keyframe_seed_scratch_bytes(W, H)), dtype=torch.uint8, device=dev)
    status, aux = torch.empty(8, **i32), torch.empty(4, **f32)
    with torch.cuda.device(dev):
        stream = stream_ptr(dev)
        check(L.olsr_keyframe_seed_plan(C.byref(p), image.data_ptr(), depth.data_ptr(),
                                        exposure.data_ptr() if exposure is not None else None, w2c.data_ptr(), C.byref(rows),
                                        staging["pix_index"].data_ptr(), scratch.data_ptr(), status.data_ptr(), aux.data_ptr(),
                                        stream))
        n_keep = int(status[1].item())   # the one host read: it sizes the kNN and the returned views
        n = n_keep if n_keep >= 4 else 0
        knn = torch.empty(int(L.olsr_knn_scratch_bytes(n)), dtype=torch.uint8, device=dev) if n else None
        # (n_keep < 4: finish writes nothing and says so with OLSR_OK)
        check(L.olsr_keyframe_seed_finish(C.byref(p), n_keep, C.byref(rows), aux.data_ptr(), scratch.data_ptr(),
                                          knn.data_ptr() if n else None, stream))
    out = {k: staging[k][:n] for k in ("means3D", "shs", "opacities", "scales", "rotations", "pix_index")}
    out.update(n_valid=status[0], median_depth=aux[0], point_size=aux[1], n_keep=n_keep)
    return out
