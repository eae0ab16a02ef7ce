"""Scenes that put the backward composite's staging-batch boundaries where a test wants them (k_render_bwd.hip stages 64 or
128 list entries per fill of its LDS tables, walking a tile's list from its far end).

One tile of a 2 x 2-tile image carries the whole scene:
  family 1: N tiny Gaussians of opacity 0.01 stacked at distinct depths within 1.5 pixels of the tile's centre.  Nothing
            saturates and every entry blends; each one reaches one to four pixels, and between them they reach the upper and
            the lower half of the tile, i.e. every wave of the composite kernels, each wave blending its own subset;
  family 2 (lower=True): Gaussians of the same kind 4.5 pixels further down, which reach only rows 10 and below: the waves of
            the upper half never blend them.  One of them follows every second family-1 Gaussian in depth, and a run of `tail`
            of them lies behind everything else - so that, for the upper waves, visits that only advance the language
            recursion and the visits skipped before a wave has met its first own entry fall on both sides of a batch boundary.
The tile's list is [family 1 and 2 interleaved ..., tail], front to back: Gaussian i is list position i.

Why tiny: the gradient tensors here have a few hundred elements, in which the element-wise criterion (1e-4 of the element +
1e-6 of the tensor's largest) allows no outlier.  A sum over a dozen pixels whose terms cancel is off by a few 2^-24 of the
terms' magnitudes whatever the order of summation, which is above that floor when the tensor's largest element is itself such
a sum; over one to four pixels the rounding of a sum stays several times below it.
"""
import hashlib

import numpy as np
import torch

from online_lang_splatting_amd.scene import Scene, default_camera

N_VALUES = (1, 63, 64, 65, 127, 128, 129, 200)
F_VALUES = (0, 3, 15, 16, 32)
TILES = (15, 16)
# (lower, background): the plain stack (list length == N), the two families, the two families over a background
VARIANTS = ((False, False), (True, False), (True, True))
BG = (0.3, 0.6, 0.1)
SIGMA_PX = 0.3   # before the rasterizer's 0.3 px^2 low-pass: alpha >= 1/255 within 0.85 pixels of the centre
JITTER_PX = 1.5
LOWER_DY = 4.5


def tail_of(N):
    """family-2 Gaussians behind everything else: longer than a 128-entry batch, longer than a 64-entry one, or two"""
    return (130, 66, 2)[N % 3]


def layout(N, lower):
    """family (1 or 2) per list position, front to back"""
    if not lower:
        return [1] * N
    fam = []
    for j in range(N):
        fam.append(1)
        if j % 2 == 1 or j == N - 1:
            fam.append(2)
    return fam + [2] * tail_of(N)


def make(N, tile, F, lower, bg, seed=None):
    """The scene (CPU tensors; Gaussian i is list position i of the tile (0, 0)) and its family layout."""
    fam = layout(N, lower)
    L = len(fam)
    W = H = 2 * tile
    cam = default_camera(W, H)
    g = torch.Generator().manual_seed(7919 * N + 131 * tile + 17 * F + 2 * int(lower) + int(bg) if seed is None else seed)
    z = 1.0 + 2.0 * (torch.arange(L, dtype=torch.float32) + 0.25 * torch.rand(L, generator=g)) / max(L, 1)
    centre = tile / 2.0
    fam_t = torch.tensor(fam)
    u = centre + 2.0 * JITTER_PX * (torch.rand(L, generator=g) - 0.5)
    v = centre + 2.0 * JITTER_PX * (torch.rand(L, generator=g) - 0.5) + torch.where(fam_t == 2, LOWER_DY, 0.0)
    x = (u - cam.cx) * z / cam.fx
    y = (v - cam.cy) * z / cam.fy
    means3D = torch.stack([x, y, z], dim=1).contiguous()
    scales = (SIGMA_PX * z / cam.fx).unsqueeze(1).repeat(1, 3).contiguous()
    rotations = torch.zeros(L, 4)
    rotations[:, 0] = 1.0
    opacities = torch.full((L, 1), 0.01)
    shs = (torch.rand(L, 1, 3, generator=g) * 3.0 - 1.5).contiguous()
    language = None
    if F > 0:
        l = torch.randn(L, F, generator=g)
        language = (l / l.norm(dim=1, keepdim=True)).contiguous()
    bgt = torch.tensor(BG) if bg else torch.zeros(3)
    return Scene(cam, means3D, opacities, scales, rotations, shs, language, 0, bgt, F), fam


def cases(tile, F):
    for N in N_VALUES:
        for lower, bg in VARIANTS:
            yield N, lower, bg


def case_id(tile, mode, F, N, lower, bg):
    return f"t{tile}_m{mode}_F{F}_N{N}_l{int(lower)}_b{int(bg)}"


def digest(grads):
    """SHA-256 over every gradient tensor's fp32 bits (keys in sorted order; -0 counts as +0)."""
    h = hashlib.sha256()
    for k in sorted(grads):
        t = grads[k]
        if t is None or not torch.is_tensor(t) or t.numel() == 0:
            continue
        a = np.ascontiguousarray(t.detach().cpu().float().numpy()) + np.float32(0.0)
        h.update(k.encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()
