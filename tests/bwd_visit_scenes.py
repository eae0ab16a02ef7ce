"""Small scenes for one VISIT of the backward composite (k_render_bwd.hip): what a wave does with one list entry when only some
of its lanes blend it, when none of them does, and when the entry carries a colour nobody may touch.

Every tile of the image carries a list of N entries, front to back, alternating between two anchors of the tile: A in its
upper left quadrant and B in its lower right one (different quadrants = different waves of the 256-thread kernels; rows below
and above rank 112 = the two survivor waves of the packed 15 x 15 reference kernel).  All entries are tiny (0.3 px before the
rasteriser's low-pass), so each is blended by one to four pixels and skipped by every other lane of the wave that visits it:
  (a) partial skips.  A lane whose pixel the entry does not reach skips it by the alpha floor; a lane whose last blended entry
      lies in front of it skips it by `k >= last_contributor`; every tenth entry (positions 3, 13, ... on anchor B of a full-size tile) is
      a HYPERBOLIC splat - a 3D covariance with one negative variance, whose conic is indefinite - which the lanes above and
      below its axis skip by `power > 0` while the lanes on the axis blend it;
  (b) recursion-only visits.  An entry on anchor B between two entries on anchor A is skipped by every lane of A's wave, but
      not by the tile: in reference mode with language channels A's wave visits it only to advance the language recursion;
  (c) variant "inf" / "nan": the SECOND entry of each list (the first one for N = 1) carries +inf, or NaN, in its colour and,
      with plant_language, in its whole language row.  The lanes that skip it must keep their state bit for bit; where the
      reference itself ends up non-finite (the pixels that blend it), the non-finite positions are what is compared.  The
      GPU test plants the language row in the exact mode only: the reference mode's recursion is unguarded, a non-finite row
      turns accum_rec into NaN in EVERY pixel of the tile through 0 * inf, also where last_alpha is still zero, and the fast
      kernel - which carries the recursion as a dot product and skips visits that cannot change it - has never reproduced
      that pixel by pixel.  That is how the kernel was before this test and no subject of it.
Images: one tile and 2 x 2 tiles of 15 and of 16 pixels, and 17 x 17 with 15-pixel tiles, whose three edge tiles are 2 pixels
wide or high: most lanes of their waves lie outside the image.  There the anchors sit inside the strip that exists.

Colours come in through colors_precomp and covariances through cov3D_precomp (the hyperbolic splats need one), the same
arrays for the oracle and the product.  Gaussian i of tile t is list position i of that tile.
"""
import hashlib

import numpy as np
import torch

from online_lang_splatting_amd.scene import Scene, default_camera

N_VALUES = (1, 2, 3, 64, 65)
F_VALUES = (0, 3, 15, 16, 32)
IMAGES = {15: ((15, 15), (30, 30), (17, 17)), 16: ((16, 16), (32, 32))}  # tile -> (W, H)
VARIANTS = ("plain", "inf", "nan")
BG = (0.3, 0.6, 0.1)
SIGMA_PX = 0.3
HYPER_SIGMA2_PX = 0.5   # variance (px^2) of a hyperbolic splat's positive axis; the other axis gets minus that
HYPER_EVERY = 10


def tiles_of(W, H, tile):
    """(x0, y0, x1, y1) of every tile, clipped to the image, in tile-id order"""
    out = []
    for y0 in range(0, H, tile):
        for x0 in range(0, W, tile):
            out.append((x0, y0, min(x0 + tile, W), min(y0 + tile, H)))
    return out


def make(N, tile, F, W, H, variant="plain", bg=False, plant_language=True):
    """(scene, kw, info): kw = dict(colors_precomp, cov3D_precomp) for run_backend / ordered_backward; info = dict(per_tile=N,
    planted=[Gaussian ids], hyper=[Gaussian ids], anchor=[0 (A) / 1 (B) per Gaussian])."""
    cam = default_camera(W, H)
    g = torch.Generator().manual_seed(10007 * N + 101 * tile + 13 * F + 7 * W + VARIANTS.index(variant))
    us, vs, zs, anchor, hyper, planted = [], [], [], [], [], []
    for (x0, y0, x1, y1) in tiles_of(W, H, tile):
        w, h = x1 - x0, y1 - y0
        full = (w == tile and h == tile)
        base = len(us)
        for j in range(N):
            b = j % 2  # A, B, A, B, ...
            is_h = full and j % HYPER_EVERY == 3  # (j odd: anchor B)
            r = (torch.rand(2, generator=g) - 0.5) * 2.0
            # pixel centres are integers: the strip [x0, x1) holds the pixels x0 .. x1 - 1
            # (anchors at 0.3 and 0.7 of a full tile, half a pixel of jitter: a splat's rect - radius 3, 4 for a hyperbolic one -
            #  stays inside its tile, so the reference's lists have the constructed lengths too; a strip 2 pixels wide gets its
            #  entries on its centre line)
            cx = x0 + ((0.3 + 0.4 * b) * w - 0.5 if w == tile else 0.5 * (w - 1)) + float(r[0]) * (0.5 if w == tile else 0.2)
            cy = y0 + ((0.3 + 0.4 * b) * h - 0.5 if h == tile else 0.5 * (h - 1)) + float(r[1]) * (0.5 if h == tile else 0.2)
            us.append(cx)
            vs.append(cy)
            zs.append(1.0 + 2.0 * (j + 0.25 * float(torch.rand(1, generator=g))) / N)
            anchor.append(b)
            if is_h:
                hyper.append(base + j)
        planted.append(base + (1 if N > 1 else 0))
    P = len(us)
    u, v, z = (torch.tensor(t, dtype=torch.float32) for t in (us, vs, zs))
    means3D = torch.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], dim=1).contiguous()
    s2 = (SIGMA_PX * z / cam.fx) ** 2
    cov = torch.zeros(P, 6)
    cov[:, 0] = cov[:, 3] = cov[:, 5] = s2
    for i in hyper:
        h2 = HYPER_SIGMA2_PX * float(z[i] / cam.fx) ** 2
        cov[i, 0], cov[i, 3], cov[i, 5] = h2, -h2, float(s2[i])
    opac = 0.01 + 0.04 * torch.rand(P, 1, generator=g)
    colors = torch.rand(P, 3, generator=g).contiguous()
    language = None
    if F > 0:
        l = torch.randn(P, F, generator=g)
        language = (l / l.norm(dim=1, keepdim=True)).contiguous()
    if variant != "plain":
        bad = float("inf") if variant == "inf" else float("nan")
        for i in planted:
            colors[i, :] = bad
            if language is not None and plant_language:
                language[i, :] = bad
    scales = torch.full((P, 3), 1e-3)  # (unused: cov3D_precomp)
    rotations = torch.zeros(P, 4)
    rotations[:, 0] = 1.0
    shs = torch.zeros(P, 1, 3)         # (unused: colors_precomp)
    bgt = torch.tensor(BG) if bg else torch.zeros(3)
    sc = Scene(cam, means3D, opac.contiguous(), scales, rotations, shs, language, 0, bgt, F)
    kw = dict(colors_precomp=colors, cov3D_precomp=cov.contiguous())
    return sc, kw, dict(per_tile=N, planted=planted, hyper=hyper, anchor=anchor)


def cases(tile):
    """(N, (W, H), variant, bg) of one kernel instantiation's run: every list length on every image, the variants and the
    background dealt round so that each N, each image, each variant and both backgrounds occur."""
    k = 0
    for W, H in IMAGES[tile]:
        for N in N_VALUES:
            yield N, (W, H), VARIANTS[k % 3], bool((k // 3 + k) % 2)
            k += 1


def case_id(tile, mode, F, N, WH, variant, bg):
    return f"t{tile}_m{mode}_F{F}_N{N}_{WH[0]}x{WH[1]}_{variant}_b{int(bg)}"


def digest(grads):
    """SHA-256 over every gradient tensor's fp32 bits (keys in sorted order; -0 counts as +0, every NaN as one NaN: which
    payload a NaN carries out of an fma depends on the order the compiler gives its operands, which is no arithmetic)."""
    h = hashlib.sha256()
    for k in sorted(grads):
        t = grads[k]
        if t is None or not torch.is_tensor(t) or t.numel() == 0:
            continue
        a = np.ascontiguousarray(t.detach().cpu().float().numpy()) + np.float32(0.0)
        a = np.where(np.isnan(a), np.float32("nan"), a).astype(np.float32)
        h.update(k.encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()
