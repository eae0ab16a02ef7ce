"""Generates tests/golden/loss_edges.npz by calling the REFERENCE's own loss code on inputs that sit ON the loss's decisions.

Run in the authoring container only (needs /root/reference):  python tests/golden/make_golden_loss_edges.py

Same construction as make_golden_loss.py: utils.slam_utils.get_loss_mapping / get_loss_tracking are called unmodified on a stub
viewpoint whose .cuda() is the identity; the language term is the three reference lines of utils/slam_backend.py:579-590;
gradients are autograd's through exactly these calls.  What differs is the input.  Planted, each at pixels of its own:
  gt_image.sum(0) == thr exactly, and one float32 ulp either side (the sum is exact in any order: two channels are 0, or the
      three are 0.25 + 0.25 + {0, 2^-24} at thr = 0.5)
  gt_depth == float32(0.01), and its two neighbours
  tracking: opacity == float32(0.95), and its two neighbours
  ties v == 0 in RGB, depth and language (cases with a = b = 0, or initialization: the tie is exact)
  grad_mask == 0 on an otherwise live pixel
  language targets larger than, smaller than and equal to the image, and 1 x 1
  a rendered pixel that is NaN, one that is +inf, a NaN under a zero mask (colour), and a NaN language value
alpha is 0.9375 or 0.875, which float32 holds exactly: the reference keeps alpha as a Python double, the C ABI as a float, and at
0.95 the depth weight 1 - alpha differs by alpha's own rounding enlarged 19 times (3 ulp; mapping_loss.npz shows it,
tests/test_loss_ref_cpu.py).  This fixture pins decisions and arithmetic, not that representation.
Recorded as the reference returns them — on this torch sign(NaN) = 0 and NaN * 0 = NaN: a NaN pixel has a zero cotangent and
poisons the mean, masked or not.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, "/root/reference")
from utils.slam_utils import get_loss_mapping, get_loss_tracking  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
INF = f32(np.inf)


def around(v):
    v = f32(v)
    return [float(np.nextafter(v, -INF)), float(v), float(np.nextafter(v, INF))]


class _StaysHere(torch.Tensor):
    def cuda(self, *a, **k):
        return torch.Tensor(self)


class _Viewpoint:
    pass


def _viewpoint(gt_image, gt_depth, a, b):
    vp = _Viewpoint()
    vp.original_image = gt_image.as_subclass(_StaysHere)
    vp.depth = gt_depth.numpy()
    vp.exposure_a = torch.tensor([a], requires_grad=True)
    vp.exposure_b = torch.tensor([b], requires_grad=True)
    return vp


def _plant_common(image, depth, gt_image, gt_depth, thr, W, exact_tie):
    """The edges both losses share; pixel p is (p // W, p % W).  Returns the next free pixel."""
    px = lambda p: (p // W, p % W)  # noqa: E731
    p = 0
    for ch in range(3):                                   # the threshold itself and its neighbours, in each channel
        for val in around(thr):
            gt_image[:, px(p)[0], px(p)[1]] = 0.0
            gt_image[ch, px(p)[0], px(p)[1]] = val
            p += 1
    if thr == 0.5:                                        # the same with three live channels, sums exact in any order
        for trio in ((0.25, 0.25, 0.0), (0.25, 0.25, 2.0 ** -24), (0.25, float(np.nextafter(f32(0.25), f32(0))), 0.0)):
            gt_image[:, px(p)[0], px(p)[1]] = torch.tensor(trio)
            p += 1
    for val in around(0.01):
        gt_depth[px(p)] = val
        p += 1
    if exact_tie:                                         # v == 0: |0| has gradient 0
        y, x = px(p)
        image[:, y, x] = torch.tensor([0.3, 0.4, 0.5])
        gt_image[:, y, x] = image[:, y, x]
        p += 1
        y, x = px(p)
        gt_depth[y, x] = 1.75
        depth[0, y, x] = 1.75
        p += 1
    return p


def _plant_nonfinite(image, gt_image, p, W, zero_mask):
    """A NaN and a +inf on live pixels, a NaN under a zero mask (zero_mask(y, x) makes the pixel's mask zero)."""
    y, x = p // W, p % W
    gt_image[:, y, x] = 0.4
    image[0, y, x] = float("nan")
    y, x = (p + 1) // W, (p + 1) % W
    gt_image[:, y, x] = 0.4
    image[1, y, x] = float("inf")
    y, x = (p + 2) // W, (p + 2) % W
    zero_mask(y, x)
    image[2, y, x] = float("nan")
    return p + 3


def case(seed, H, W, Fch, lh, lw, a, b, alpha, thr, init, nonfinite=None):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(3, H, W, generator=g)
    depth = torch.rand(1, H, W, generator=g) * 4
    lang = torch.randn(Fch, H, W, generator=g).mul(0.3)
    gt_image = torch.rand(3, H, W, generator=g)
    gt_depth = torch.rand(H, W, generator=g) * 4
    gt_lang = torch.randn(Fch, lh, lw, generator=g).mul(0.3)
    exact = init or (a == 0.0 and b == 0.0)
    p = _plant_common(image, depth, gt_image, gt_depth, thr, W, exact)
    if exact and (lh, lw) in ((H, W), (1, 1)):            # the resized target IS the texel: a language tie per channel
        for ch in range(Fch):
            y, x = (p + ch) // W, (p + ch) % W
            lang[ch, y, x] = gt_lang[ch, y if lh == H else 0, x if lw == W else 0]
        p += Fch
    if nonfinite == "colour":
        def zero(y, x):
            gt_image[:, y, x] = 0.0
        p = _plant_nonfinite(image, gt_image, p, W, zero)
    elif nonfinite == "language":
        lang[1, p // W, p % W] = float("nan")
        p += 1
    assert p < H * W
    image.requires_grad_(True), depth.requires_grad_(True), lang.requires_grad_(True)
    vp = _viewpoint(gt_image, gt_depth, a, b)
    cfg = {"Training": {"alpha": alpha, "rgb_boundary_threshold": thr}}
    loss_map = get_loss_mapping(cfg, image, depth, vp, None, initialization=init)        # the reference
    resized = F.interpolate(gt_lang.unsqueeze(0), size=(H, W), mode="bilinear", align_corners=False).squeeze(0)
    l_lang = torch.abs(lang - resized).mean()                                              # l1_loss
    loss = loss_map + 1.0 * l_lang                                                         # lamda_lang = 1.0
    loss.backward()
    z = torch.zeros(1)
    return dict(image=image.detach(), depth=depth.detach(), lang=lang.detach(), gt_image=gt_image, gt_depth=gt_depth,
                gt_lang=gt_lang, a=torch.tensor([a]), b=torch.tensor([b]), alpha=torch.tensor(alpha, dtype=torch.float64),
                thr=torch.tensor(thr, dtype=torch.float64), init=torch.tensor(int(init)), loss=loss.detach(),
                loss_map=loss_map.detach(), loss_lang=l_lang.detach(), d_image=image.grad, d_depth=depth.grad, d_lang=lang.grad,
                d_a=vp.exposure_a.grad if vp.exposure_a.grad is not None else z,
                d_b=vp.exposure_b.grad if vp.exposure_b.grad is not None else z)


def tracking_case(seed, H, W, a, b, alpha, thr, nonfinite=False):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(3, H, W, generator=g)
    depth = torch.rand(1, H, W, generator=g) * 4
    opacity = torch.rand(1, H, W, generator=g)
    opacity[:, :, W // 2:] = 0.96 + 0.04 * opacity[:, :, W // 2:]
    gt_image = torch.rand(3, H, W, generator=g)
    gt_depth = torch.rand(H, W, generator=g) * 4
    grad_mask = torch.rand(1, H, W, generator=g) > 0.25
    exact = a == 0.0 and b == 0.0
    p = _plant_common(image, depth, gt_image, gt_depth, thr, W, exact)
    grad_mask[0].view(-1)[:p] = True                      # the planted pixels are decided by what was planted
    opacity[0].view(-1)[:p] = 0.97
    for val in around(0.95):                              # opacity > 0.95 on a pixel whose depth is valid
        y, x = p // W, p % W
        opacity[0, y, x] = val
        gt_depth[y, x] = 2.0
        p += 1
    y, x = p // W, p % W                                  # grad_mask zero on an otherwise live pixel
    gt_image[:, y, x] = 0.4
    opacity[0, y, x] = 0.97
    grad_mask[0, y, x] = False
    p += 1
    if nonfinite:
        first = p

        def zero(y, x):
            gt_image[:, y, x] = 0.4
            grad_mask[0, y, x] = False
        p = _plant_nonfinite(image, gt_image, p, W, zero)
        grad_mask[0].view(-1)[first:first + 2] = True
        opacity[0].view(-1)[first:p] = 0.97
    assert p < H * W
    image.requires_grad_(True), depth.requires_grad_(True)
    vp = _viewpoint(gt_image, gt_depth, a, b)
    vp.grad_mask = grad_mask
    cfg = {"Training": {"alpha": alpha, "rgb_boundary_threshold": thr}}
    loss = get_loss_tracking(cfg, image, depth, opacity, vp)                                # the reference
    loss.backward()
    return dict(image=image.detach(), depth=depth.detach(), opacity=opacity, gt_image=gt_image, gt_depth=gt_depth,
                grad_mask=grad_mask.to(torch.float32), a=torch.tensor([a]), b=torch.tensor([b]),
                alpha=torch.tensor(alpha, dtype=torch.float64), thr=torch.tensor(thr, dtype=torch.float64),
                loss=loss.detach(), d_image=image.grad, d_depth=depth.grad, d_a=vp.exposure_a.grad,
                d_b=vp.exposure_b.grad)


def main():
    out = {}
    tcases = [(21, 12, 20, 0.0, 0.0, 0.875, 0.01, False),             # exact ties
              (22, 9, 13, -0.2, 0.04, 0.875, 0.5, False),            
              (23, 9, 13, 0.07, -0.02, 0.875, 0.01, True)]            # NaN, +inf, NaN under grad_mask == 0
    for i, c in enumerate(tcases):
        for k, v in tracking_case(*c).items():
            out[f"t{i}_{k}"] = v.numpy()
    out["n_tracking_cases"] = np.array(len(tcases))
    cases = [(31, 12, 20, 3, 12, 20, 0.0, 0.0, 0.9375, 0.01, False),          # identity target, a = b = 0: exact ties
             (32, 9, 13, 3, 20, 30, 0.07, -0.02, 0.875, 0.5, False),          # target larger than the image
             (33, 9, 13, 3, 4, 5, 0.0, 0.0, 0.875, 0.5, True),              # smaller; initialization
             (34, 9, 13, 3, 1, 1, 0.0, 0.0, 0.9375, 0.01, False),             # 1 x 1
             (35, 9, 13, 3, 7, 6, 0.07, -0.02, 0.9375, 0.01, False, "colour"),
             (36, 9, 13, 3, 7, 6, -0.3, 0.05, 0.875, 0.01, False, "language")]
    for i, c in enumerate(cases):
        for k, v in case(*c).items():
            out[f"c{i}_{k}"] = v.numpy()
    out["n_cases"] = np.array(len(cases))
    path = os.path.join(HERE, "loss_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote loss_edges.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
