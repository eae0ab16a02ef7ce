"""Host side of olsr_mapping_loss / olsr_tracking_loss / olsr_refinement_loss (include/olsr.h): the loss of one view and
the cotangents the rasterizer backward consumes, in one HIP pass (the colour-refinement loss
with SSIM in two).

Mirrors what utils/slam_backend.py:579-597 + utils/slam_utils.py:124-165 of the reference compute with
PyTorch ops + autograd:  loss, d loss / d (image, depth, language), d loss / d (exposure_a, exposure_b).
GPU only; there is no CPU fallback.
"""
import ctypes as C

import torch

from . import _abi
from ._host import ptr, stream_ptr
from ._lib import check, lib


def _rendered(name, t, shape, dev=None):
    """A rendered image handed over by the rasterizer: float32, on the GPU, of the expected shape (no conversion:
    these are the arrays whose cotangents are returned)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be a float32 tensor on the GPU")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, expected {dev}")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.contiguous()


def _image3(name, image):
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or image.shape[0] != 3:
        raise RuntimeError(f"{name} must be a [3, H, W] tensor")
    return _rendered(name, image, image.shape)


def _target(name, t, shape, dev):
    """A target / side input (ground truth, exposure, mask): the reference keeps some of these on the CPU or in other
    dtypes (viewpoint.gt_lang_feat, utils/slam_backend.py:576; bool masks), so they are converted to float32 on
    the device of the rendered image; the shape must match (`None` entries of `shape` are free)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if len(t.shape) != len(shape) or any(e is not None and int(s_) != int(e) for s_, e in zip(t.shape, shape)):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple('*' if e is None else e for e in shape)}")
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _exposure(exposure, dev):
    """{exposure_a, exposure_b} as one device float32[2]; accepts a [2] tensor or the reference's pair of
    1-element parameters (viewpoint.exposure_a, viewpoint.exposure_b)."""
    if exposure is None:
        return None
    if isinstance(exposure, (tuple, list)):
        if len(exposure) != 2:
            raise RuntimeError("exposure must be a [2] tensor or a pair (exposure_a, exposure_b)")
        exposure = torch.cat([e.detach().reshape(1) for e in exposure])
    return _target("exposure", exposure.reshape(-1), (2,), dev)


def _exposure_slot(who, t, dev):
    if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or t.numel() != 2
            or not t.is_contiguous()):
        raise RuntimeError(f"{who}: dL_dexposure_out must be a contiguous float32[2] on {dev}")
    return t


def mapping_loss(image, depth, language, gt_image, gt_depth, gt_language=None, exposure=None, *, alpha=0.95,
                 rgb_boundary_threshold=0.01, lamda_lang=1.0, initialization=False, dL_dexposure_out=None):
    """image [3,H,W], depth [1,H,W], language [F,H,W] or None, gt_image [3,H,W], gt_depth [H,W],
    gt_language [F,h,w] or None, exposure = device tensor [2] {exposure_a, exposure_b} or None.
    Returns dict(loss[4] = {total, rgb, depth, language terms}, dL_dimage, dL_ddepth, dL_dlanguage, dL_dexposure[2]).
    dL_dexposure_out: a contiguous float32[2] on the image's device that receives dL_dexposure instead of a fresh tensor (a
    view's slot of slam_iterations.KeyframeWindow)."""
    image = _image3("mapping_loss: image", image)
    dev = image.device
    H, W = image.shape[1], image.shape[2]
    depth = _rendered("mapping_loss: depth", depth, (1, H, W), dev)
    F = 0 if language is None else int(language.shape[0])
    if language is not None:
        language = _rendered("mapping_loss: language", language, (F, H, W), dev)
    gt_image = _target("mapping_loss: gt_image", gt_image, (3, H, W), dev)
    if gt_depth is not None and gt_depth.dim() == 3:
        gt_depth = gt_depth.reshape(gt_depth.shape[-2], gt_depth.shape[-1])
    gt_depth = _target("mapping_loss: gt_depth", gt_depth, (H, W), dev)
    if gt_image is None or gt_depth is None:
        raise RuntimeError("mapping_loss: gt_image and gt_depth are required")
    gt_language = _target("mapping_loss: gt_language", gt_language, (F, None, None), dev) if F > 0 else None
    exposure = _exposure(exposure, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    p = _abi.OlsrLossParams(width=W, height=H, F=F, lang_width=0 if gt_language is None else gt_language.shape[2],
                            lang_height=0 if gt_language is None else gt_language.shape[1],
                            initialization=int(bool(initialization)), alpha=float(alpha),
                            rgb_boundary_threshold=float(rgb_boundary_threshold), lamda_lang=float(lamda_lang),
                            one_minus_alpha=1.0 - float(alpha))   # in double, as the reference forms it
    out = dict(loss=torch.empty(4, **f32), dL_dimage=torch.empty(3, H, W, **f32), dL_ddepth=torch.empty(1, H, W, **f32),
               dL_dlanguage=torch.empty(F, H, W, **f32),
               dL_dexposure=(torch.empty(2, **f32) if dL_dexposure_out is None
                             else _exposure_slot("mapping_loss", dL_dexposure_out, dev)))
    L = lib()
    scratch = torch.empty(L.olsr_mapping_loss_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_mapping_loss(C.byref(p), ptr(image), ptr(depth), ptr(language), ptr(gt_image), ptr(gt_depth),
                                  ptr(gt_language), ptr(exposure), ptr(out["dL_dimage"]), ptr(out["dL_ddepth"]),
                                  ptr(out["dL_dlanguage"]), ptr(out["loss"]), ptr(out["dL_dexposure"]),
                                  scratch.data_ptr(), stream_ptr(dev)))
    return out


def tracking_loss(image, depth, opacity, gt_image, gt_depth, grad_mask=None, exposure=None, *, alpha=0.95,
                  rgb_boundary_threshold=0.01):
    """get_loss_tracking (utils/slam_utils.py:92-121) and its image cotangents in one pass.
    image [3,H,W], depth [1,H,W], opacity [1,H,W], gt_image [3,H,W], gt_depth [H,W], grad_mask [1,H,W] or [H,W]
    (bool or float) or None, exposure = device tensor [2] or None.
    Returns dict(loss[4] = {total, rgb term, depth term, 0}, dL_dimage, dL_ddepth, dL_dexposure[2])."""
    image = _image3("tracking_loss: image", image)
    dev = image.device
    H, W = image.shape[1], image.shape[2]
    depth = _rendered("tracking_loss: depth", depth, (1, H, W), dev)
    opacity = _rendered("tracking_loss: opacity", opacity, (1, H, W), dev)
    gt_image = _target("tracking_loss: gt_image", gt_image, (3, H, W), dev)
    if gt_depth is not None and gt_depth.dim() == 3:
        gt_depth = gt_depth.reshape(gt_depth.shape[-2], gt_depth.shape[-1])
    gt_depth = _target("tracking_loss: gt_depth", gt_depth, (H, W), dev)
    if gt_image is None or gt_depth is None:
        raise RuntimeError("tracking_loss: gt_image and gt_depth are required")
    if grad_mask is not None and grad_mask.dim() == 3:
        grad_mask = grad_mask.reshape(grad_mask.shape[-2], grad_mask.shape[-1])
    gm = _target("tracking_loss: grad_mask", grad_mask, (H, W), dev)
    exposure = _exposure(exposure, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    p = _abi.OlsrLossParams(width=W, height=H, F=0, lang_width=0, lang_height=0, initialization=0, alpha=float(alpha),
                            rgb_boundary_threshold=float(rgb_boundary_threshold), lamda_lang=0.0,
                            one_minus_alpha=1.0 - float(alpha))
    out = dict(loss=torch.empty(4, **f32), dL_dimage=torch.empty(3, H, W, **f32), dL_ddepth=torch.empty(1, H, W, **f32),
               dL_dexposure=torch.empty(2, **f32))
    L = lib()
    scratch = torch.empty(L.olsr_mapping_loss_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_tracking_loss(C.byref(p), ptr(image), ptr(depth), ptr(opacity), ptr(gt_image), ptr(gt_depth), ptr(gm),
                                   ptr(exposure), ptr(out["dL_dimage"]), ptr(out["dL_ddepth"]), ptr(out["loss"]),
                                   ptr(out["dL_dexposure"]), scratch.data_ptr(),
                                   stream_ptr(dev)))
    return out


def refinement_loss(image, gt_image, *, lambda_dssim=0.2, want_grad=True, buffers=None):
    """The colour-refinement loss (utils/slam_backend.py:798-801) of one view and its image cotangent (olsr_refinement_loss):
    (1 - lambda_dssim) * l1_loss(image, gt_image) + lambda_dssim * (1 - ssim(image, gt_image)), image / gt_image [3,H,W].
    Returns dict(loss[4] = {total, (1 - lambda) L1, lambda (1 - SSIM), SSIM}, dL_dimage [3,H,W] or None);
    want_grad=False evaluates the values only (the SSIM of the reference's evaluation, utils/eval_utils.py:174).
    buffers: a dict the caller keeps between calls on images of one size (a loop): outputs and scratch are allocated into it
    once and reused, so the returned tensors are overwritten by the next call."""
    image = _image3("refinement_loss: image", image)
    dev = image.device
    H, W = image.shape[1], image.shape[2]
    gt_image = _target("refinement_loss: gt_image", gt_image, (3, H, W), dev)
    if gt_image is None:
        raise RuntimeError("refinement_loss: gt_image is required")
    f32 = dict(dtype=torch.float32, device=dev)
    L = lib()
    b = buffers if buffers is not None else {}
    if b.get("key") != (H, W, dev):
        b.clear()
        b.update(key=(H, W, dev), loss=torch.empty(4, **f32), dL_dimage=None,
                 scratch=torch.empty(L.olsr_refinement_loss_scratch_bytes(W, H), dtype=torch.uint8, device=dev))
    if want_grad and b["dL_dimage"] is None:
        b["dL_dimage"] = torch.empty(3, H, W, **f32)
    out = dict(loss=b["loss"], dL_dimage=b["dL_dimage"] if want_grad else None)
    scratch = b["scratch"]
    with torch.cuda.device(dev):
        check(L.olsr_refinement_loss(W, H, float(lambda_dssim), image.data_ptr(), gt_image.data_ptr(),
                                     out["dL_dimage"].data_ptr() if want_grad else None, out["loss"].data_ptr(),
                                     scratch.data_ptr(), stream_ptr(dev)))
    return out


def isotropic_loss(scales, activations=0, weight=10.0, want_grad=False):
    """The mapping loss's isotropic regulariser (utils/slam_backend.py:664-667) on its own (olsr_isotropic_reg):
    weight * |s - s.mean(dim=1)|.mean() of scales [P,3], contiguous float32 on the GPU; activations & ACT_SCALE_EXP: `scales`
    holds log(scale) and the gradient is with respect to it.  Returns the loss, a 0-d float64 tensor on the device (the same
    bits on every run), or with want_grad (loss, gradient [P,3]).  Inside a mapping iteration the Adam step forms the same
    gradient itself (FusedAdam.step(isotropic=...)): this entry is for the value and for tests."""
    if (not isinstance(scales, torch.Tensor) or not scales.is_cuda or scales.dtype != torch.float32 or scales.dim() != 2
            or scales.shape[1] != 3 or not scales.is_contiguous()):
        raise RuntimeError("isotropic_loss: scales must be a contiguous float32 [P,3] tensor on the GPU")
    dev, P = scales.device, int(scales.shape[0])
    L = lib()
    loss = torch.empty((), dtype=torch.float64, device=dev)
    grad = torch.empty_like(scales) if want_grad else None
    scratch = torch.empty(L.olsr_isotropic_reg_scratch_bytes(P), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_isotropic_reg(P, scales.data_ptr() if P else None, int(activations), float(weight),
                                   grad.data_ptr() if want_grad and P else None, loss.data_ptr(), scratch.data_ptr(),
                                   stream_ptr(dev)))
    return (loss, grad) if want_grad else loss


class _Ssim(torch.autograd.Function):
    """SSIM through olsr_refinement_loss at lambda = 1: the value is loss[3]; d SSIM / d img1 = -dL_dimage."""

    @staticmethod
    def forward(ctx, img1, img2):
        out = refinement_loss(img1.detach(), img2, lambda_dssim=1.0, want_grad=ctx.needs_input_grad[0])
        ctx.shape = img1.shape
        ctx.save_for_backward(out["dL_dimage"])
        return out["loss"][3].clone()

    @staticmethod
    def backward(ctx, grad):
        (d,) = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise RuntimeError("ssim: no gradient is produced for img2 (the target is a constant of olsr_refinement_loss)")
        return (d * (-grad)).reshape(ctx.shape), None


def ssim(img1, img2, window_size=11, size_average=True):
    """ssim of gaussian_splatting/utils/loss_utils.py:61-69 on the fused entry: img1, img2 [3,H,W] or [1,3,H,W] float32 on
    the GPU, a 0-d tensor back; differentiable with respect to img1.  Only what the reference's callers use exists: anything
    else raises (there is no torch fallback)."""
    if window_size != 11:
        raise NotImplementedError(f"ssim: window_size must be 11 (the kernel's window is compiled in), got {window_size}")
    if not size_average:
        raise NotImplementedError("ssim: size_average=False (per-image means) is not implemented")
    if not isinstance(img1, torch.Tensor) or not isinstance(img2, torch.Tensor):
        raise RuntimeError("ssim: img1 and img2 must be tensors")
    if img2.requires_grad:
        raise RuntimeError("ssim: no gradient is produced for img2 (detach the target)")
    shape = tuple(img1.shape)
    if tuple(img2.shape) != shape or not (len(shape) == 3 or (len(shape) == 4 and shape[0] == 1)) or shape[-3] != 3:
        raise RuntimeError(f"ssim: img1 and img2 must both be [3,H,W] or [1,3,H,W], got {shape} and {tuple(img2.shape)}")
    if len(shape) == 4:
        img1, img2 = img1.reshape(shape[1:]), img2.reshape(shape[1:])
    return _Ssim.apply(img1, img2)
