"""Host side of the front end's frame step (include/olsr.h, "front end: the frame step"; csrc/k_frontend.hip): the tracking
mask, the median depth after tracking, and the keyframe test with the window policy — and of the frame's ingest ahead of
them (include/olsr_frame_ingest.h; csrc/k_frame_ingest.hip).

Replaces what the reference's front end does once per frame in PyTorch ops with host reads (utils/slam_frontend.py:577-676):
Camera.compute_grad_mask (utils/camera_utils.py:123-152), get_median_depth (utils/slam_utils.py:168-179), is_keyframe /
add_to_window and the small-window rule (utils/slam_frontend.py:279-430, 633-645).  A tracked frame needs ONE host read (the
192-byte decision record); the tracking mask costs one launch in block mode.  Stated deviations (the header has the
arithmetic): with no valid pixel the median depth is NaN and the count 0 (the reference raises); with nothing left to score
the window policy removes nothing (the reference's np.argmax raises).  GPU only."""
import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _abi
from ._host import stream_ptr
from ._lib import check, lib

MODES = {"blocks": _abi.GRAD_MASK_BLOCKS, "global": _abi.GRAD_MASK_GLOBAL}


def _gpu(what, *tensors):
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{what}: every tensor must be on the GPU (there is no CPU fallback)")


def _need(what, cond, msg):
    if not cond:
        raise ValueError(f"{what}: {msg}")



def tracking_mask(image: torch.Tensor, edge_threshold: float, mode: str = "blocks", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """image float32 [3,H,W] (rows contiguous, any plane stride) -> the grad_mask [1,H,W] float32 that TrackingLoop,
    losses.tracking_loss and the fused forward consume.  mode "blocks": the reference's Replica branch (0 / 1 inside the
    32 x 32 image blocks, the raw intensity on the margins); "global": every other dataset (0 / 1 against the image's median).
    out: a contiguous float32 tensor of H W elements to write into."""
    _gpu("tracking_mask", image)
    _need("tracking_mask", mode in MODES, "mode must be 'blocks' or 'global'")
    _need("tracking_mask", image.dim() == 3 and image.shape[0] == 3 and image.dtype == torch.float32, "image must be float32 [3,H,W]")
    H, W = int(image.shape[1]), int(image.shape[2])
    _need("tracking_mask", image.stride(2) == 1 and image.stride(1) == W and image.stride(0) >= W * H, "image rows must be contiguous")
    dev = image.device
    if out is None:
        out = torch.empty(1, H, W, dtype=torch.float32, device=dev)
    else:
        _gpu("tracking_mask", out)
        _need("tracking_mask", out.device == dev and out.dtype == torch.float32 and out.numel() == W * H and out.is_contiguous(),
              "out must be a contiguous float32 tensor of H W elements on the image's device")
    L = lib()
    scratch = None
    if mode == "global":
        scratch = torch.empty(int(L.olsr_frontend_scratch_bytes(W * H)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_grad_mask(W, H, int(image.stride(0)), MODES[mode], float(edge_threshold), image.data_ptr(), out.data_ptr(),
                               scratch.data_ptr() if scratch is not None else None, stream_ptr(dev)))
    return out


def ingest_frame(rgb_u8: torch.Tensor, depth: torch.Tensor, depth_scale: float, out_image: Optional[torch.Tensor] = None,
                 out_depth: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A frame as the dataset decodes it -> what every other entry consumes, in one launch (include/olsr_frame_ingest.h):
    rgb_u8 uint8 [H,W,3] (interleaved, contiguous, any byte address), depth [H,W] uint16 or float32 (contiguous) ->
    (image float32 [3,H,W] = float32(clamp(float64(byte) / 255, 0, 1)), depth float32 [H,W] = float32(float64(d) / depth_scale)),
    the statements of ReplicaDataset / TUMDataset.__getitem__ and of the depth conversion in get_loss_tracking /
    add_new_keyframe.  out_image: float32 [3,H,W] with contiguous rows and any plane stride; out_depth: contiguous float32 of
    H W elements.  The datasets' undistortion (cv2.remap) is not part of it."""
    _gpu("ingest_frame", rgb_u8, depth)
    _need("ingest_frame", rgb_u8.dim() == 3 and rgb_u8.shape[2] == 3 and rgb_u8.dtype == torch.uint8, "rgb_u8 must be uint8 [H,W,3]")
    H, W = int(rgb_u8.shape[0]), int(rgb_u8.shape[1])
    _need("ingest_frame", H > 0 and W > 0, "the frame must not be empty")
    _need("ingest_frame", rgb_u8.is_contiguous(), "rgb_u8 must be contiguous")
    dev = rgb_u8.device
    _need("ingest_frame", depth.dtype in (torch.uint16, torch.float32), "depth must be uint16 or float32")
    _need("ingest_frame", depth.device == dev and tuple(depth.shape) == (H, W) and depth.is_contiguous(),
          "depth must be a contiguous [H,W] tensor on the image's device")
    depth_scale = float(depth_scale)
    _need("ingest_frame", depth_scale > 0.0 and depth_scale != float("inf"), "depth_scale must be finite and > 0")
    if out_image is None:
        out_image = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    else:
        _gpu("ingest_frame", out_image)
        _need("ingest_frame", out_image.device == dev and out_image.dtype == torch.float32 and tuple(out_image.shape) == (3, H, W)
              and out_image.stride(2) == 1 and out_image.stride(1) == W and out_image.stride(0) >= W * H,
              "out_image must be float32 [3,H,W] with contiguous rows on the image's device")
    if out_depth is None:
        out_depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    else:
        _gpu("ingest_frame", out_depth)
        _need("ingest_frame", out_depth.device == dev and out_depth.dtype == torch.float32 and out_depth.numel() == W * H and
              out_depth.is_contiguous(), "out_depth must be a contiguous float32 tensor of H W elements on the image's device")
    p = _abi.OlsrFrameIngestParams(W=W, H=H, depth_type=_abi.INGEST_DEPTH_U16 if depth.dtype == torch.uint16 else _abi.INGEST_DEPTH_F32,
                                   plane_stride=int(out_image.stride(0)), depth_scale=depth_scale)
    with torch.cuda.device(dev):
        check(lib().olsr_frame_ingest(C.byref(p), rgb_u8.data_ptr(), depth.data_ptr(), out_image.data_ptr(), out_depth.data_ptr(),
                                      stream_ptr(dev)))
    return out_image, out_depth


def median_depth(depth: torch.Tensor, opacity: torch.Tensor, mask: Optional[torch.Tensor] = None,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """get_median_depth(depth, opacity, mask): -> (median float32 [1], count int32 [1]), both left on the device.  depth and
    opacity: contiguous float32 of the same number of elements; mask: bool or uint8 of that many, or None."""
    _gpu("median_depth", depth, opacity)
    dev = depth.device
    N = depth.numel()
    _need("median_depth", depth.dtype == torch.float32 and depth.is_contiguous() and N > 0, "depth must be contiguous float32, not empty")
    _need("median_depth", opacity.device == dev and opacity.dtype == torch.float32 and opacity.is_contiguous() and opacity.numel() == N,
          "opacity must be contiguous float32 with depth's number of elements, on its device")
    if mask is not None:
        _gpu("median_depth", mask)
        _need("median_depth", mask.device == dev and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous() and
              mask.numel() == N, "mask must be contiguous bool or uint8 with depth's number of elements, on its device")
    if out is None:
        out = (torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    L = lib()
    scratch = torch.empty(int(L.olsr_frontend_scratch_bytes(N)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_median_depth(N, depth.data_ptr(), opacity.data_ptr(), mask.data_ptr() if mask is not None else None,
                                  scratch.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), stream_ptr(dev)))
    return out


def _pose16(pose, dev):
    """PoseState (its state[0:16] is T_w2c row-major) or a [4,4] world-to-camera tensor -> contiguous float32 [16] on dev."""
    state = getattr(pose, "state", None)
    t = state[0:16] if state is not None else pose
    _gpu("KeyframeSelector", t)
    _need("KeyframeSelector", t.numel() == 16 and t.dtype == torch.float32 and t.device == dev, "a pose is float32 [4,4] on the device")
    return t.reshape(16).contiguous()


class KeyframeSelector:
    """The front end's keyframe test and window policy on the device.  Owns the window (frame ids, newest first) and each
    keyframe's uint8 visibility and pose."""

    def __init__(self, window_size: int, kf_interval: int, kf_translation: float, kf_min_translation: float, kf_overlap: float,
                 kf_cutoff: float = 0.4, single_thread: bool = False):
        if not 1 <= int(window_size) < _abi.COVIS_MAX_VIEWS + 1:
            raise ValueError("KeyframeSelector: window_size must lie in 1 ... 16")
        self.window_size, self.kf_interval = int(window_size), int(kf_interval)
        self.kf_translation, self.kf_min_translation = float(kf_translation), float(kf_min_translation)
        self.kf_overlap, self.kf_cutoff, self.single_thread = float(kf_overlap), float(kf_cutoff), bool(single_thread)
        self.window: List[int] = []
        self.visibility: Dict[int, torch.Tensor] = {}
        self.poses: Dict[int, torch.Tensor] = {}
        self._counts = self._record = self._median = None

    def add_keyframe(self, kf_id: int, pose, visibility: torch.Tensor) -> None:
        """Puts a keyframe at the front of the window without a test (initialisation: the first frame)."""
        _gpu("KeyframeSelector", visibility)
        self.poses[kf_id] = _pose16(pose, visibility.device).clone()
        self.window = [kf_id] + self.window
        self.set_visibility(kf_id, visibility)

    def set_visibility(self, kf_id: int, mask: torch.Tensor) -> None:
        """The back end's (n_touched > 0) of a keyframe after mapping: bool or uint8 [P]."""
        _gpu("KeyframeSelector", mask)
        _need("KeyframeSelector", mask.dim() == 1 and mask.dtype in (torch.bool, torch.uint8), "a visibility is bool or uint8 [P]")
        if kf_id not in self.poses:
            raise KeyError(f"KeyframeSelector: {kf_id} is no keyframe of the window")
        self.visibility[kf_id] = mask.to(torch.uint8).contiguous().clone()

    def prune(self, keep_mask: torch.Tensor) -> None:
        """After a map prune: every visibility keeps the rows of keep_mask (bool [P])."""
        _gpu("KeyframeSelector", keep_mask)
        for k, v in self.visibility.items():
            self.visibility[k] = v[keep_mask].contiguous()

    def observe(self, frame_idx: int, n_touched: torch.Tensor, pose, depth: torch.Tensor, opacity: torch.Tensor):
        """One tracked frame: median depth -> covisibility -> decision, enqueued on the current stream, then ONE host read of
        the record.  -> (create, new_window, removed, record): new_window / removed (frame ids) are what the window becomes /
        loses when the frame is made a keyframe; the window is committed only when create is true.  record: dict with the
        record's fields (include/olsr.h) and the device tensors `median_depth`, `count`."""
        _gpu("KeyframeSelector.observe", n_touched, depth, opacity)
        _need("KeyframeSelector.observe", n_touched.dim() == 1 and n_touched.dtype == torch.int32 and n_touched.is_contiguous() and
              n_touched.numel() > 0, "n_touched must be a contiguous int32 [P], P > 0")
        dev, P, K = n_touched.device, int(n_touched.numel()), len(self.window)
        for k in self.window:
            _need("KeyframeSelector.observe", k in self.visibility and self.visibility[k].numel() == P and self.visibility[k].device == dev,
                  f"keyframe {k} has no visibility of {P} rows on the device")
        cur_pose = _pose16(pose, dev)
        if self._counts is None or self._counts.device != dev:
            self._counts = torch.empty(_abi.COVIS_COUNTS, dtype=torch.int64, device=dev)
            self._record = torch.empty(_abi.KEYFRAME_RECORD_BYTES // 4, dtype=torch.int32, device=dev)
            self._median = (torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
        median, count = median_depth(depth, opacity, out=self._median)
        cur_vis = torch.empty(P, dtype=torch.uint8, device=dev)
        views = _abi.OlsrCovisViews(K=K)
        for i, k in enumerate(self.window):
            views.vis[i] = self.visibility[k].data_ptr()
        kf_poses = torch.stack([self.poses[k] for k in self.window]) if K else None
        check_time = bool(self.window) and (int(frame_idx) - int(self.window[0])) >= self.kf_interval
        p = _abi.OlsrKeyframeDecideParams(window_len=K, window_size=self.window_size, check_time=int(check_time),
                                          single_thread=int(self.single_thread), kf_translation=self.kf_translation,
                                          kf_min_translation=self.kf_min_translation, kf_overlap=self.kf_overlap,
                                          kf_cutoff=self.kf_cutoff)
        L = lib()
        with torch.cuda.device(dev):
            st = stream_ptr(dev)
            check(L.olsr_covisibility(P, n_touched.data_ptr(), C.byref(views), cur_vis.data_ptr(), self._counts.data_ptr(), st))
            check(L.olsr_keyframe_decide(C.byref(p), self._counts.data_ptr(), median.data_ptr(), cur_pose.data_ptr(),
                                         kf_poses.data_ptr() if K else None, self._record.data_ptr(), st))
            raw = self._record.cpu().numpy()   # the one host read
        rec = decode_record(raw)
        rec.update(median_depth=median, count=count)
        gone = [p_ for p_ in (rec["removed_a"], rec["removed_b"]) if p_ >= 0]
        removed = [self.window[p_] for p_ in gone]
        new_window = [int(frame_idx)] + [k for i, k in enumerate(self.window) if i not in gone]
        if rec["create"]:
            for k in removed:
                self.visibility.pop(k, None)
                self.poses.pop(k, None)
            self.window = new_window
            self.visibility[int(frame_idx)] = cur_vis
            self.poses[int(frame_idx)] = cur_pose.clone()
        return rec["create"], new_window, removed, rec


def decode_record(raw: np.ndarray) -> Dict:
    """The int32 words of olsr_keyframe_decide's record (int32[8] + float32[40]) as a dict."""
    ri, rf = raw[:8], raw[8:].view(np.float32)
    n = _abi.COVIS_MAX_VIEWS
    return dict(create=bool(ri[0]), removals=int(ri[1]), removed_a=int(ri[2]), removed_b=int(ri[3]), is_kf=bool(ri[4]),
                n_cur=int(ri[5]), inter0=int(ri[6]), n_vis0=int(ri[7]), dist=float(rf[0]), median=float(rf[1]),
                ratio_u=float(rf[2]), cut=rf[4:4 + n].copy(), score=rf[4 + n:4 + 2 * n].copy())
