"""Host side of olsr_mask_smooth / olsr_query_eval / olsr_image_psnr (include/olsr.h): the figures the reference's 2-D
evaluation reports, from the maps LanguageQuery.relevancy() leaves on the device.

eval/evaluate_onlinelangslam.py turns a phrase's mask into an IoU (activate_stream, :152-163: `smooth`, a 7 x 7 majority vote
written as a Python loop over the pixels, then logical_and / logical_or against the annotated mask) and the smoothed relevancy
into a localisation hit (lerf_localization, :203-223: every pixel that attains the maximum is tested against the phrase's
boxes); process_single_eval (:294-296) averages them per image and evaluate_per_image (:347-348) over the images.
`QueryEvaluator` does the same with one 16-byte row per phrase read back.  `psnr` / `frame_metrics` are the masked PSNR and
the SSIM of eval_rendering (utils/eval_utils.py:171-174).

One head only (the online pipeline has one level).  The annotated masks are taken at the map's size: the reference's
cv2.resize of the annotation (:157) stays with the caller.  The colour maps and every file the reference writes are not part
of this.  GPU only; there is no torch fallback.
"""
import math

import numpy as np
import torch

from . import _abi
from ._host import scratch_for, stream_ptr
from ._lib import check, lib
from .lang_query import LanguageQuery


def _planes(who, name, t, dtype, shape=None, device=None):
    """A contiguous [P,H,W] device tensor of `dtype` (with H, W >= 2), of `shape` and on `device` if given."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a tensor on the GPU (there is no torch fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if device is not None and t.device != device:
        raise RuntimeError(f"{who}: {name} is on {t.device}, expected {device}")
    if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] < 2 or t.shape[2] < 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "[P,H,W] with P >= 1 and H, W >= 2" if shape is None else f"{list(shape)}"
        raise RuntimeError(f"{who}: {name} has shape {tuple(t.shape)}, expected {want}")
    return t.detach().contiguous()


def smooth_masks(mask):
    """`smooth` of eval/utils.py on the device (olsr_mask_smooth): mask [H,W] or [P,H,W] uint8 on the GPU, any byte != 0 set
    -> the 7 x 7 majority vote of the same shape, 0 / 1.  The reference's windows are kept, the last row and column that never
    enter one included; H, W >= 2."""
    who = "smooth_masks"
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError(f"{who}: mask must be a tensor on the GPU (there is no torch fallback)")
    if mask.dim() not in (2, 3):
        raise RuntimeError(f"{who}: mask has shape {tuple(mask.shape)}, expected [H,W] or [P,H,W]")
    m = _planes(who, "mask", mask if mask.dim() == 3 else mask.unsqueeze(0), torch.uint8)
    out = torch.empty_like(m)
    P, H, W = m.shape
    with torch.cuda.device(m.device):
        check(lib().olsr_mask_smooth(P, H, W, m.data_ptr(), out.data_ptr(), stream_ptr(m.device)))
    return out if mask.dim() == 3 else out[0]


def _box_offsets(who, off, P, n_boxes):
    if isinstance(off, torch.Tensor):
        if off.dtype not in (torch.int32, torch.int64):
            raise RuntimeError(f"{who}: box_offsets must be an integer tensor, got {off.dtype}")
        off = off.detach().cpu().numpy()
    off = np.asarray(off)
    if off.ndim != 1 or off.size != P + 1 or not np.issubdtype(off.dtype, np.integer):
        raise RuntimeError(f"{who}: box_offsets must be P + 1 = {P + 1} integers, got shape {tuple(off.shape)} of {off.dtype}")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] < 0 or np.any(np.diff(off) < 0):
        raise RuntimeError(f"{who}: box_offsets must start at >= 0 and not decrease")
    if off[-1] > n_boxes:
        raise RuntimeError(f"{who}: box_offsets ends at {int(off[-1])}, but there are {n_boxes} boxes")
    return off.astype(np.int32)


class QueryEvaluator:
    """Mean IoU and localisation accuracy of a LanguageQuery's positives against an image's annotation, image after image."""

    def __init__(self, query: LanguageQuery):
        if not isinstance(query, LanguageQuery):
            raise RuntimeError("QueryEvaluator: a LanguageQuery is expected")
        self.query, self.device = query, query.device
        self.reset()

    def reset(self):
        """Forgets the images seen so far."""
        self._mean_iou, self._accuracy = [], []

    def evaluate(self, codes_or_result, gt_masks, boxes, box_offsets, out_hw=None, decode_hw=None):
        """codes_or_result: codes [15,h,w] (queried here: relevancy(codes, out_hw, decode_hw)), or the dict relevancy() /
        localise() returned.  gt_masks uint8 [P,H,W] on the GPU at the map's size, != 0 set; boxes float32 [B,4] =
        (x1, y1, x2, y2) on the GPU; box_offsets: P + 1 integers (a list, an array or a tensor), phrase p owns boxes
        box_offsets[p] : box_offsets[p+1], possibly none.
        -> dict: iou float64 [P] = intersection / union (NaN where the union is 0, as numpy's 0 / 0), intersection, union,
        n_max (pixels that attain the smoothed relevancy's maximum), hit (1: one of them lies in one of the phrase's boxes):
        numpy arrays from one read of 16 P bytes; mask_smoothed uint8 [P,H,W] on the device; mean_iou and accuracy = hits / P
        as process_single_eval forms them.  The image counts towards summary()."""
        who = "evaluate"
        if isinstance(codes_or_result, dict):
            if out_hw is not None or decode_hw is not None:
                raise RuntimeError(f"{who}: out_hw and decode_hw belong to a query made here; a result dict has its size")
            r = codes_or_result
            missing = [k for k in ("mask", "smoothed", "score") if k not in r]
            if missing:
                raise RuntimeError(f"{who}: the result lacks {missing} (the dict of relevancy() or localise() is expected)")
        else:
            r = self.query.relevancy(codes_or_result, out_hw=out_hw, decode_hw=decode_hw)
        mask = _planes(who, "mask", r["mask"], torch.uint8, device=self.device)
        P, H, W = mask.shape
        smoothed = _planes(who, "smoothed", r["smoothed"], torch.float32, (P, H, W), self.device)
        score = r["score"]
        if not isinstance(score, torch.Tensor) or score.dtype != torch.float32 or score.device != self.device or tuple(score.shape) != (P,):
            raise RuntimeError(f"{who}: score must be a float32 [{P}] tensor on {self.device}")
        gt = _planes(who, "gt_masks", gt_masks, torch.uint8, (P, H, W), self.device)
        if not isinstance(boxes, torch.Tensor) or not boxes.is_cuda or boxes.dtype != torch.float32 or boxes.device != self.device:
            raise RuntimeError(f"{who}: boxes must be a float32 tensor on the GPU ({self.device})")
        if boxes.dim() != 2 or boxes.shape[1] != 4:
            raise RuntimeError(f"{who}: boxes has shape {tuple(boxes.shape)}, expected [B,4]")
        boxes = boxes.detach().contiguous()
        off = _box_offsets(who, box_offsets, P, boxes.shape[0])
        L = lib()
        scratch = scratch_for(self.device, "query_eval", L.olsr_query_eval_scratch_bytes(P, H, W))
        result = torch.empty((P, 4), dtype=torch.int32, device=self.device)
        mask_smoothed = torch.empty_like(mask)
        with torch.cuda.device(self.device):
            check(L.olsr_query_eval(P, H, W, mask.data_ptr(), smoothed.data_ptr(), score.detach().contiguous().data_ptr(),
                                    gt.data_ptr(), boxes.data_ptr() if boxes.numel() else None, off.ctypes.data,
                                    result.data_ptr(), mask_smoothed.data_ptr(), scratch.data_ptr(), stream_ptr(self.device)))
        host = result.cpu().numpy().astype(np.int64)
        inter, union, n_max, hit = (host[:, k] for k in range(4))
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = inter.astype(np.float64) / union.astype(np.float64)
        mean_iou = sum(iou.tolist()) / P
        accuracy = int(hit.sum()) / P
        self._mean_iou.append(mean_iou)
        self._accuracy.append(accuracy)
        return dict(iou=iou, intersection=inter, union=union, n_max=n_max, hit=hit, mask_smoothed=mask_smoothed,
                    mean_iou=mean_iou, accuracy=accuracy)

    def summary(self):
        """The means over the images seen since reset(), as evaluate_per_image forms them (0 without any)."""
        n = len(self._mean_iou)
        return dict(mean_iou=sum(self._mean_iou) / n if n else 0, accuracy=sum(self._accuracy) / n if n else 0, images=n)


def _image_pair(who, image, gt, channels=None):
    for name, t in (("image", image), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a tensor on the GPU (there is no torch fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
    if image.dim() != 3 or min(image.shape) < 1 or (channels is not None and image.shape[0] != channels):
        raise RuntimeError(f"{who}: image has shape {tuple(image.shape)}, expected [{'C' if channels is None else channels},H,W]")
    if tuple(gt.shape) != tuple(image.shape):
        raise RuntimeError(f"{who}: gt has shape {tuple(gt.shape)}, expected {tuple(image.shape)}")
    if gt.device != image.device:
        raise RuntimeError(f"{who}: gt is on {gt.device}, expected {image.device}")
    return image.detach().contiguous(), gt.detach().contiguous()


def psnr_sums(image, gt):
    """olsr_image_psnr: image, gt float32 [C,H,W] on the GPU -> float64 [2] on the device: the sum of
    (clamp(image, 0, 1) - gt)^2 over the elements with gt > 0, and their number."""
    image, gt = _image_pair("psnr", image, gt)
    dev = image.device
    L = lib()
    out = torch.empty(2, dtype=torch.float64, device=dev)
    scratch = scratch_for(dev, "psnr", L.olsr_image_psnr_scratch_bytes())
    Cn, H, W = image.shape
    with torch.cuda.device(dev):
        check(L.olsr_image_psnr(Cn, H, W, image.data_ptr(), gt.data_ptr(), out.data_ptr(), scratch.data_ptr(), stream_ptr(dev)))
    return out


def psnr(image, gt):
    """The evaluation's masked PSNR (utils/eval_utils.py:153, :171-173): psnr(clamp(image, 0, 1)[gt > 0], gt[gt > 0]) with
    the mask taken per element.  -> a float (one 16-byte read), NaN if no element of gt is positive."""
    s, n = psnr_sums(image, gt).tolist()
    if n == 0:
        return math.nan
    mse = s / n
    return 20.0 * math.log10(1.0 / math.sqrt(mse)) if mse > 0 else (math.inf if mse == 0 else math.nan)


def frame_metrics(image, gt):
    """What eval_rendering reports per frame next to LPIPS: {"psnr": the masked PSNR above, "ssim": losses.ssim of the
    clamped image and gt (values only)}; image, gt float32 [3,H,W] on the GPU."""
    from .losses import refinement_loss
    image, gt = _image_pair("frame_metrics", image, gt, channels=3)
    ssim = refinement_loss(torch.clamp(image, 0.0, 1.0), gt, lambda_dssim=1.0, want_grad=False)["loss"][3]
    return dict(psnr=psnr(image, gt), ssim=float(ssim))
