"""Generates tests/golden/ssim.npz by calling the REFERENCE's own loss code.

Run in the authoring container only (needs /root/reference):  python tests/golden/make_golden_ssim.py

  gaussian_splatting.utils.loss_utils (l1_loss, ssim) and gaussian_splatting.utils.general_utils (helper) are imported from
  the reference and called unmodified.  loss_utils imports cv2, which is absent here and which neither function uses: an
  empty module of that name is put into sys.modules first.
  Per case the colour-refinement loss of utils/slam_backend.py:798-801,
      (1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt)),
  is evaluated twice through autograd: on float64 copies of the inputs (the truth: `*_f64`) and on the float32 inputs (what
  the reference computes: `*_f32`).  Recorded: the four scalars {total, (1 - lambda) L1, lambda (1 - SSIM), SSIM} and
  d total / d image.
  Inputs are multiples of 2^-16 in [0, 1), stored as uint16 (value = q / 65536, exact in float32): the file stays below the
  largest existing fixture.  Also recorded: the eleven float32 window weights gaussian(11, 1.5) and
  helper(step, 1.6e-4, 1.6e-6, max_steps=30000) at a few steps (the golden of slam_iterations.position_lr).
"""
import os
import sys
import types

import numpy as np
import torch

sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, "/root/reference")
from gaussian_splatting.utils.general_utils import helper  # noqa: E402
from gaussian_splatting.utils.loss_utils import gaussian, l1_loss, ssim  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def quantise(t):
    return torch.clamp(torch.round(t.clamp(0, 1) * 65536.0), 0, 65535).to(torch.int32)


def smooth_image(H, W, g):
    y = torch.linspace(0, 1, H).view(1, H, 1)
    x = torch.linspace(0, 1, W).view(1, 1, W)
    ph = torch.rand(3, 1, 1, generator=g) * 6.28
    return 0.5 + 0.25 * torch.sin(4.0 * x + ph) * torch.cos(3.0 * y + 0.5 * ph) + 0.15 * torch.sin(9.0 * (x + y) + ph)


def inputs(kind, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        image, gt = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    elif kind == "smooth":      # a smooth image + 2 % noise against the smooth image
        gt = smooth_image(H, W, g)
        image = gt + 0.02 * torch.randn(3, H, W, generator=g)
    elif kind == "constant":    # a constant region + 0.2 % noise: sigma^2 cancels almost completely
        gt = smooth_image(H, W, g)
        gt[:, H // 4:, W // 5:] = 0.6
        image = gt + 0.002 * torch.randn(3, H, W, generator=g)
    elif kind == "identical":
        gt = torch.rand(3, H, W, generator=g)
        image = gt.clone()
    elif kind == "ties":        # noise with a block of exact ties (|0| has gradient 0)
        image, gt = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
        image[:, : H // 3, W // 2:] = gt[:, : H // 3, W // 2:]
    else:
        raise ValueError(kind)
    qi, qg = quantise(image), quantise(gt)
    if kind == "identical":
        qg = qi.clone()
    return qi, qg


def evaluate(qi, qg, lam, dtype):
    image = (qi.to(torch.float32) / 65536.0).to(dtype).requires_grad_(True)
    gt = (qg.to(torch.float32) / 65536.0).to(dtype)
    Ll1 = l1_loss(image, gt)                                  # the reference
    s = ssim(image, gt)                                       # the reference
    t_l1, t_ssim = (1.0 - lam) * Ll1, lam * (1.0 - s)
    loss = t_l1 + t_ssim                                      # utils/slam_backend.py:799-801
    loss.backward()
    return torch.stack([loss.detach(), t_l1.detach(), t_ssim.detach(), s.detach()]), image.grad


CASES = [("noise", 40, 56, 0.2, 1), ("smooth", 64, 48, 0.2, 2), ("constant", 33, 21, 1.0, 3), ("identical", 33, 21, 1.0, 4),
         ("noise", 7, 9, 0.2, 5), ("ties", 33, 21, 0.0, 6)]


def main():
    out = {"n_cases": np.array(len(CASES))}
    w = gaussian(11, 1.5)
    assert w.dtype == torch.float32
    out["window"] = w.numpy()
    print("window:", [np.format_float_scientific(v, unique=True) for v in w.numpy()])
    for i, (kind, H, W, lam, seed) in enumerate(CASES):
        qi, qg = inputs(kind, H, W, seed)
        l64, d64 = evaluate(qi, qg, lam, torch.float64)
        l32, d32 = evaluate(qi, qg, lam, torch.float32)
        assert d64.dtype == torch.float64 and d32.dtype == torch.float32
        out[f"c{i}_kind"] = np.array(kind)
        out[f"c{i}_lambda"] = np.array(lam, dtype=np.float64)
        out[f"c{i}_image_q"] = qi.numpy().astype(np.uint16)
        if kind != "identical":
            out[f"c{i}_gt_q"] = qg.numpy().astype(np.uint16)
        out[f"c{i}_loss_f64"], out[f"c{i}_loss_f32"] = l64.numpy(), l32.numpy()
        out[f"c{i}_d_image_f64"], out[f"c{i}_d_image_f32"] = d64.numpy(), d32.numpy()
        print(i, kind, (H, W), lam, "loss", l64.tolist(), "|d|max", float(d64.abs().max()),
              "ref32 err max", float((d32.double() - d64).abs().max()))
    steps = [0, 1, 15000, 30000, 40000]
    out["lr_steps"] = np.array(steps)
    out["lr_values"] = np.array([helper(s, 1.6e-4, 1.6e-6, max_steps=30000) for s in steps], dtype=np.float64)
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
