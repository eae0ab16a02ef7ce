"""Torch restatement of the colour-refinement loss, dtype-generic: the full-size yardstick of tests/test_gpu_ssim.py.

    loss = (1 - lambda) * mean|image - gt| + lambda * (1 - SSIM(image, gt))

SSIM as the reference evaluates it (gaussian_splatting/utils/loss_utils.py:42-101): gaussian(11, 1.5) computed in Python
doubles, stored and normalised in FLOAT32, the 2-D window the float32 outer product, only then cast to the images' dtype
(so a float64 evaluation still uses float32-rounded weights); grouped conv2d with zero padding 5; C1 = 0.01^2, C2 = 0.03^2;
mean over all elements.  tests/test_ssim_ref_golden.py pins this module to arrays recorded from the reference itself
(tests/golden/ssim.npz) in float64.  Runs on the CPU or the GPU, wherever its inputs live.
"""
import os
from math import exp

import numpy as np
import torch
import torch.nn.functional as F


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim.npz"))


def golden_case(z, i):
    """-> (kind, lambda, image, gt) of case i of tests/golden/ssim.npz; float32 inputs (multiples of 2^-16, exact)."""
    image = torch.from_numpy(z[f"c{i}_image_q"].astype(np.float32)) / 65536.0
    gt = torch.from_numpy(z[f"c{i}_gt_q"].astype(np.float32)) / 65536.0 if f"c{i}_gt_q" in z else image.clone()
    return str(z[f"c{i}_kind"]), float(z[f"c{i}_lambda"]), image, gt


def smooth_image(H, W, seed):
    """A smooth [3,H,W] image in [0.1, 0.9] (low-frequency sinusoids, one phase per channel)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H).view(1, H, 1)
    x = torch.linspace(0, 1, W).view(1, 1, W)
    ph = torch.rand(3, 1, 1, generator=g) * 6.28
    return 0.5 + 0.25 * torch.sin(4.0 * x + ph) * torch.cos(3.0 * y + 0.5 * ph) + 0.15 * torch.sin(9.0 * (x + y) + ph)


def window_1d():
    """The eleven normalised float32 weights."""
    g = torch.tensor([exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    return g / g.sum()


def window_2d(channels, like):
    w = window_1d().unsqueeze(1)
    w2 = w.mm(w.t()).float()                      # float32 outer product, rounded per element
    return w2.expand(channels, 1, 11, 11).contiguous().to(device=like.device, dtype=like.dtype)


def ssim(img1, img2):
    ch = img1.shape[-3]
    win = window_2d(ch, img1)
    blur = lambda t: F.conv2d(t, win, padding=5, groups=ch)  # noqa: E731
    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = blur(img1 * img1) - mu1_sq
    sigma2_sq = blur(img2 * img2) - mu2_sq
    sigma12 = blur(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean()


def refinement_loss(image, gt, lambda_dssim=0.2):
    """-> (total, (1 - lambda) L1, lambda (1 - SSIM), SSIM), 0-d tensors of the inputs' dtype."""
    l1 = torch.abs(image - gt).mean()
    s = ssim(image, gt)
    t_l1, t_ssim = (1.0 - lambda_dssim) * l1, lambda_dssim * (1.0 - s)
    return t_l1 + t_ssim, t_l1, t_ssim, s


def loss_and_grad(image, gt, lambda_dssim=0.2, dtype=None):
    """dict(loss[4], dL_dimage) through autograd, evaluated in `dtype` (default: the inputs')."""
    dtype = dtype or image.dtype
    x = image.detach().to(dtype).clone().requires_grad_(True)
    terms = refinement_loss(x, gt.detach().to(dtype), lambda_dssim)
    terms[0].backward()
    return dict(loss=torch.stack([t.detach() for t in terms]), dL_dimage=x.grad)
