"""Scenes that aim the alpha-floor contour of a Gaussian at the places where the exact tile binning (cull_* in
csrc/olsr_device.h) can go wrong: tile-corner pixels, the half-pixel gap between two tile rows, the rightmost point as the
only contact with a band, the image borders, far-away centres, opacities at the 1/255 floor, and the `exact` gate.

Every family is built the same way: place the Gaussians (all lie in planes facing the camera, rotated about the view axis,
so that the 2-D covariance is what the family asks for), run the oracle's preprocess, read means2D, conic_opacity and radii
- none of which depends on the opacity - and then set the opacities in closed form from those fp32 values.  The opacity is
a direct input of the rasteriser: the contour lands where the family wants it to an ulp of the opacity.

  at(target, eps)  puts the composite's own contour, alpha = 1/255, at the signed margin eps from the pixel `target`,
                   measured in ln(255 alpha) there: opacity = exp(eps - power) / 255 with `power` evaluated in the
                   composite's fp32 operation order.  eps > 0: the pixel blends.
  t2(value)        puts the kernel's contour {q <= t2} by inverting cull_threshold (tile_cull_ref.opacity_for_t2).

A Gaussian is aimed at `target` along a unit normal n: its centre is target - d with d = r Sigma n (Sigma the 2-D covariance),
so that the contour's outward normal at the target is n and, with n pointing into a tile, the target is the tile's only
contact with the contour when the contour passes through it.

Families (FAMILIES; make(name, tile) -> Family, cached; 157 x 101 pixels unless stated, F = 3 for 15-pixel tiles and F = 0
for 16-pixel ones):
  graze    a tile-corner pixel of a random tile (the partial tiles of the last row and column included), all four corner
           kinds, eps = +-1e-6, +-1e-4, +-1e-2, anisotropy 1:1, 10:1, 100:1, 1000:1 at 12 orientations: 1152 Gaussians.
  gap      faint needles, horizontal and vertical, centred at t T + T - 0.5 between the last pixel line of one tile row
           (column) and the first of the next; the kernel's contour is 0.2 - 0.9 pixels wide on either side
           and 10 - 30 pixels long (a longer needle meets a pixel line at so shallow an angle that any pad in y moves its end by
           pixels).
  extreme  small blobs wholly inside one band whose rightmost (leftmost) point is aimed at the first (last) pixel column of
           a tile: n = (+-1, 0), eps = +-1e-4, +-5e-2 (at 0.8 pixels sigma, 1e-2 is 4e-3 pixels: inside the pads).  A third of
           them aim the KERNEL's contour instead (t2): its star point lies 2e-4 pixels past the column - inside core, closer
           than any pad - or 5e-3 pixels short of it - outside may.
  border   centres 0.5 - 300 pixels outside each side and corner of the image; the contour ends on the last real pixel line
           (eps = +-1e-2) or 0.5, 1, 2.5 pixel lines beyond it: lines the last, partial tile spans but the image does not have.
  far      huge round splats 1e3 - 1e5 pixels away whose contour cuts off a corner pixel of the image (the splat covers the
           corner alone, or all but the corner); the margin is +-0.25 and +-2.5 PIXELS along the normal.  256 x 192 pixels.
  floor    255 opacity within +-4 ulp of 1, and 1.001; centres on a pixel and on a pixel corner.
  gate     needles at 30, 45 and 135 degrees, 1e3 - 2e6 pixels long: the fp32 conic loses its positive determinant, t2
           passes 1e6 and the radius 2^20 - cull_setup's `exact` gate - among ordinary blobs.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

import tile_cull_ref as ref
from parity_common import fwd_args  # (first: it puts the repository root on sys.path)
from online_lang_splatting_amd.scene import Scene, default_camera

FAMILIES = ("graze", "gap", "extreme", "border", "far", "floor", "gate")
TILES = (15, 16)
SIZE = {"far": (256, 192)}
RAGGED = (157, 101)
GRAZE_EPS = (1e-6, -1e-6, 1e-4, -1e-4, 1e-2, -1e-2)
GRAZE_ANISO = (1.0, 10.0, 100.0, 1000.0)
ORIENTATIONS = 12
EXTREME_EPS = (1e-4, -1e-4, 5e-2, -5e-2)
EXTREME_CORE_PX = (2e-4, -5e-3)            # the kernel's own contour, in pixels past the aimed column
BORDER_BEYOND = (0.0, 0.5, 1.0, 2.5)       # pixel lines beyond the last real one (0: the last real one)
FAR_EPS_PX = (0.25, -0.25, 2.5, -2.5)
GAP_HALF = (0.2, 0.3, 0.4, 0.45, 0.55, 0.7, 0.9)
FLOOR_ULPS = tuple(range(-4, 5))
TINY_OPACITY = 1e-6                        # the preprocess passes blend nothing

Family = namedtuple("Family", "name tile W H scene pre info")
Pre = namedtuple("Pre", "means2D conic_opacity radii")


def F_of(tile):
    return 3 if tile == 15 else 0


def size_of(name):
    return SIZE.get(name, RAGGED)


def _oracle():
    from oracle import oracle_C
    oracle_C.lib()
    return oracle_C


def oracle_run(sc, tile, record=False):
    """The oracle's forward: dict(R, radii, means2D, conic_opacity, point_list, ranges, contrib_mask (record only))."""
    O = _oracle()
    O.TILE = tile
    if record:
        O.lib().oracle_set_record(1)
    try:
        a = fwd_args(sc, None)
        r = O.rasterize_language_gaussians(*a) if sc.F > 0 else O.rasterize_gaussians(*a)
    finally:
        O.lib().oracle_set_record(0)
    geom = r[4] if sc.F > 0 else r[3]
    out = dict(R=r[0], radii=(r[3] if sc.F > 0 else r[2]).numpy().copy())
    for k in ("means2D", "conic_opacity", "point_list", "ranges", "tiles_touched") + (("contrib_mask",) if record else ()):
        out[k] = O.get_field(geom, k).numpy().copy()
    O.release(geom)
    return out


def _scene(W, H, F, centres, sM, sm, theta, seed):
    """N flat Gaussians at the pixel positions `centres`: in-plane sigmas sM, sm pixels, major axis at `theta`, depths
    increasing with the index."""
    cam = default_camera(W, H)
    N = centres.shape[0]
    g = torch.Generator().manual_seed(seed)
    z = 1.0 + torch.arange(N, dtype=torch.float64) / max(N, 1)
    c = torch.from_numpy(np.asarray(centres, dtype=np.float64))
    # ndc2Pix puts the pinhole point u = fx x / z + cx at pixel coordinate u - 0.5 (tests/fwd_batch_scenes.py: HALF_PIXEL)
    x = (c[:, 0] + 0.5 - cam.cx) * z / cam.fx
    y = (c[:, 1] + 0.5 - cam.cy) * z / cam.fy
    means3D = torch.stack([x, y, z], dim=1).float().contiguous()
    s = torch.stack([torch.from_numpy(np.asarray(sM, dtype=np.float64)) * z / cam.fx,
                     torch.from_numpy(np.asarray(sm, dtype=np.float64)) * z / cam.fx,
                     1e-3 * z / cam.fx], dim=1).float().contiguous()
    th = torch.from_numpy(np.asarray(theta, dtype=np.float64))
    rot = torch.stack([torch.cos(th / 2), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64),
                       torch.sin(th / 2)], dim=1).float().contiguous()
    shs = (torch.rand(N, 1, 3, generator=g) * 3.0 - 1.5).contiguous()
    language = None
    if F > 0:
        l = torch.randn(N, F, generator=g)
        language = (l / l.norm(dim=1, keepdim=True)).contiguous()
    return Scene(cam, means3D, torch.full((N, 1), TINY_OPACITY), s, rot, shs, language, 0, torch.zeros(3), F)


def _preprocess(sc, tile, culled_ok=False):
    o = oracle_run(sc, tile)
    assert culled_ok or (o["radii"] > 0).all(), "a Gaussian of an aimed family was culled"
    return Pre(o["means2D"].reshape(-1, 2), o["conic_opacity"].reshape(-1, 4), o["radii"])


def _sigma0(sM, sm, theta):
    cs, sn = np.cos(theta), np.sin(theta)
    return (sM ** 2 * cs * cs + sm ** 2 * sn * sn + 0.3, (sM ** 2 - sm ** 2) * cs * sn, sM ** 2 * sn * sn + sm ** 2 * cs * cs + 0.3)


def _offset(sxx, sxy, syy, n, q0):
    """d = r Sigma n with q(d) = r^2 n' Sigma n = q0"""
    dx, dy = sxx * n[:, 0] + sxy * n[:, 1], sxy * n[:, 0] + syy * n[:, 1]
    r = np.sqrt(q0 / (n[:, 0] * dx + n[:, 1] * dy))
    return np.stack([r * dx, r * dy], 1)


def _aim(W, H, tile, target, n, q0, sM, sm, theta, seed, culled_ok=False):
    """The scene whose Gaussian i passes its q = q0 contour through target[i] with outward normal n[i] there (two preprocess
    passes: the second places the centre with the covariance the first one read back), and its final preprocess."""
    F = F_of(tile)
    d = _offset(*_sigma0(sM, sm, theta), n, q0)
    sc = _scene(W, H, F, target - d, sM, sm, theta, seed)
    pre = _preprocess(sc, tile, culled_ok)
    a, b, c = (pre.conic_opacity[:, k].astype(np.float64) for k in range(3))
    det = a * c - b * b
    ok = det > 0
    with np.errstate(all="ignore"):
        d2 = _offset(np.where(ok, c / det, 1.0), np.where(ok, -b / det, 0.0), np.where(ok, a / det, 1.0), n, q0)
    d = np.where(ok[:, None], d2, d)
    sc = _scene(W, H, F, target - d, sM, sm, theta, seed)
    return sc, _preprocess(sc, tile, culled_ok)


def power_fp32(pre, target):
    """the composite's `power` at the pixel `target`, in its fp32 operation order (oracle.cpp: render_forward)"""
    f = np.float32
    m, co = pre.means2D.astype(f), pre.conic_opacity.astype(f)
    dx, dy = m[:, 0] - target[:, 0].astype(f), m[:, 1] - target[:, 1].astype(f)
    return f(-0.5) * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy


def opacity_at(pre, target, eps):
    """the fp32 opacity that gives ln(255 alpha) = eps at the pixel `target`"""
    return np.exp(np.asarray(eps, dtype=np.float64) - power_fp32(pre, target).astype(np.float64)) / 255.0


def _with_opacity(sc, op):
    op = np.asarray(op, dtype=np.float64)
    assert np.isfinite(op).all() and (op > 0).all() and (op <= 1.0).all(), "an aimed opacity left (0, 1]"
    sc.opacities = torch.from_numpy(op.astype(np.float32)).reshape(-1, 1).contiguous()
    return sc


def _corner_pixel(tx, ty, sx, sy, W, H, T):
    """the corner pixel of tile (tx, ty) that a contour coming from the (-sx, -sy) side meets first"""
    x = np.where(sx > 0, tx * T, np.minimum(tx * T + T - 1, W - 1))
    y = np.where(sy > 0, ty * T, np.minimum(ty * T + T - 1, H - 1))
    return np.stack([x, y], 1).astype(np.float64)


def _graze(tile, rng, W, H):
    gx, gy = -(-W // tile), -(-H // tile)
    eps, sx, sy, an, k = (v.reshape(-1) for v in np.meshgrid(np.array(GRAZE_EPS), np.array([1.0, -1.0]), np.array([1.0, -1.0]),
                                                            np.array(GRAZE_ANISO), np.arange(ORIENTATIONS), indexing="ij"))
    N = eps.size
    tx, ty = rng.integers(0, gx, N), rng.integers(0, gy, N)
    target = _corner_pixel(tx, ty, sx, sy, W, H, tile)
    n = np.stack([sx, sy], 1) / math.sqrt(2.0)
    # sigma 2 across: |eps| = 1e-2 is then at least 5e-3 pixels, outside the pads (about 3e-3).  The 1000:1 needles are 300 x 0.3
    # pixels instead: the composite's fp32 `power` carries an error of 6e-8 (|d| / sigma_minor)^2, which at 2000 x 2 pixels
    # (0.4) decides the needle's tip pixels at random
    sm = np.where(an >= 1000.0, 0.3, 2.0)
    sc, pre = _aim(W, H, tile, target, n, rng.uniform(4.5, 8.0, N), an * sm, sm, k * math.pi / ORIENTATIONS, 11 + tile)
    sc = _with_opacity(sc, opacity_at(pre, target, eps))
    return sc, pre, dict(target=target, eps=eps, aimed_tile=ty * gx + tx, aniso=an)


def _gap(tile, rng, W, H):
    gx, gy = -(-W // tile), -(-H // tile)
    half, horiz, rep = (v.reshape(-1) for v in np.meshgrid(np.array(GAP_HALF), np.array([1, 0]), np.arange(50), indexing="ij"))
    N = half.size
    lines = np.where(horiz == 1, gy - 1, gx - 1)         # gaps that lie inside the image
    t = (rng.integers(0, 1 << 30, N) % lines)
    along = np.where(horiz == 1, rng.uniform(5.0, W - 6.0, N), rng.uniform(5.0, H - 6.0, N))
    across = t * tile + tile - 0.5
    centres = np.where(horiz[:, None] == 1, np.stack([along, across], 1), np.stack([across, along], 1))
    theta = np.where(horiz == 1, 0.0, math.pi / 2)
    sc = _scene(W, H, F_of(tile), centres, rng.uniform(3.0, 10.0, N), np.full(N, 1e-2), theta, 21 + tile)
    pre = _preprocess(sc, tile)
    a, b, c = (pre.conic_opacity[:, k].astype(np.float64) for k in range(3))
    det = a * c - b * b
    # half-width of {q <= t2} across the needle: sqrt(a t2 / det) in y for a horizontal one, sqrt(c t2 / det) in x
    t2 = half * half * det / np.where(horiz == 1, a, c)
    sc = _with_opacity(sc, ref.opacity_for_t2(t2, pre.conic_opacity, pre.radii, tile))
    return sc, pre, dict(half=half, horizontal=horiz == 1, gap_after=t)


def _extreme(tile, rng, W, H):
    gx, gy = -(-W // tile), -(-H // tile)
    margins = [(e, np.nan) for e in EXTREME_EPS] + [(0.0, d) for d in EXTREME_CORE_PX]
    mi, side, ratio, k = (v.reshape(-1) for v in np.meshgrid(np.arange(len(margins)), np.array([1.0, -1.0]), np.array([1.0, 1.5, 2.0]),
                                                            np.arange(ORIENTATIONS), indexing="ij"))
    mi, side, ratio, k = (np.tile(v, 2) for v in (mi, side, ratio, k))
    eps, core_px = np.array(margins)[mi, 0], np.array(margins)[mi, 1]
    N = eps.size
    ty = rng.integers(0, gy - 1, N)                      # whole bands only
    tx = np.where(side > 0, rng.integers(1, gx, N), rng.integers(0, gx - 1, N))
    x = np.where(side > 0, tx * tile, tx * tile + tile - 1)
    y = ty * tile + rng.integers(6, tile - 6, N)
    target = np.stack([x, y], 1).astype(np.float64)
    n = np.stack([side, np.zeros(N)], 1)
    sm = np.full(N, 0.6)
    sc, pre = _aim(W, H, tile, target, n, rng.uniform(2.0, 5.0, N), ratio * sm, sm, k * math.pi / ORIENTATIONS, 31 + tile)
    # the kernel's contour: xstar = sqrt(t2 c / det) reaches core_px pixels past the aimed column
    a, b, c = (pre.conic_opacity[:, j].astype(np.float64) for j in range(3))
    reach = np.abs(x - pre.means2D[:, 0].astype(np.float64)) + np.nan_to_num(core_px)
    op_core = ref.opacity_for_t2(reach * reach * (a * c - b * b) / c, pre.conic_opacity, pre.radii, tile)
    sc = _with_opacity(sc, np.where(np.isnan(core_px), opacity_at(pre, target, eps), op_core))
    return sc, pre, dict(target=target, eps=eps, core_px=core_px, aimed_tile=ty * gx + tx, side=side)


def _border(tile, rng, W, H):
    gx, gy = -(-W // tile), -(-H // tile)
    rows = []
    # (normal, target as a function of how many pixel lines beyond the border the contour ends)
    for name, n in (("right", (-1, 0)), ("left", (1, 0)), ("bottom", (0, -1)), ("top", (0, 1)),
                    ("rb", (-1, -1)), ("lb", (1, -1)), ("rt", (-1, 1)), ("lt", (1, 1))):
        for beyond in BORDER_BEYOND:
            for eps in ((1e-2, -1e-2) if beyond == 0.0 else (0.0,)):
                for dist in (0.5, 2.0, 8.0, 30.0, 100.0, 300.0):
                    for _ in range(3):
                        x = (W - 1 + beyond) if n[0] < 0 else (-beyond if n[0] > 0 else float(rng.integers(0, W)))
                        y = (H - 1 + beyond) if n[1] < 0 else (-beyond if n[1] > 0 else float(rng.integers(0, H)))
                        rows.append((x, y, n[0], n[1], beyond, eps, dist))
    r = np.array(rows, dtype=np.float64)
    N = r.shape[0]
    target, n = r[:, 0:2], r[:, 2:4] / np.linalg.norm(r[:, 2:4], axis=1, keepdims=True)
    beyond, eps, dist = r[:, 4], r[:, 5], r[:, 6]
    q0 = rng.uniform(3.0, 8.0, N)
    # round, sigma at least 2 (a margin of 1e-2 is then well outside the pads); the centre lies `dist` pixels from the target
    sM = np.maximum(dist / np.sqrt(q0), 2.0)
    q0 = dist * dist / (sM * sM + 0.3)
    sc, pre = _aim(W, H, tile, target, n, q0, sM, sM, np.zeros(N), 41 + tile, culled_ok=True)   # (left of / above the image a rect may be empty)
    sc = _with_opacity(sc, np.minimum(opacity_at(pre, target, eps), 1.0))
    # the tile that spans the target (the last, partial one for right / bottom; none for targets left of or above the image)
    tx, ty = np.floor(target[:, 0] / tile), np.floor(target[:, 1] / tile)
    inside = (target[:, 0] >= 0) & (target[:, 1] >= 0) & (tx < gx) & (ty < gy)
    return sc, pre, dict(target=target, eps=eps, beyond=beyond, aimed_tile=np.where(inside, ty * gx + tx, -1).astype(np.int64),
                         past_far_edge=(beyond > 0) & ((n[:, 0] < 0) | (n[:, 1] < 0)) & (n[:, 0] <= 0) & (n[:, 1] <= 0) & inside)


def _far(tile, rng, W, H):
    gx, gy = -(-W // tile), -(-H // tile)
    rows = []
    for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        into = np.array([1.0 if cx == 0 else -1.0, 1.0 if cy == 0 else -1.0])   # towards the image's interior
        for sense in (1.0, -1.0):                        # the splat covers the corner alone / all but the corner
            for ang in (10.0, 45.0, 80.0):
                for eps_px in FAR_EPS_PX:
                    for _ in range(3):
                        nn = sense * into * np.array([math.cos(math.radians(ang)), math.sin(math.radians(ang))])
                        rows.append((cx, cy, nn[0], nn[1], eps_px, sense))
    r = np.array(rows, dtype=np.float64)
    N = r.shape[0]
    target, n, eps_px = r[:, 0:2], r[:, 2:4], r[:, 4]
    q0 = rng.uniform(3.0, 8.0, N)
    dist = 10.0 ** rng.uniform(3.0, 5.0, N)
    sM = dist / np.sqrt(q0)
    sc, pre = _aim(W, H, tile, target, n, q0, sM, sM, np.zeros(N), 51 + tile)
    # a margin of eps_px pixels along the normal: ln(255 alpha) falls by |grad q| / 2 per pixel there
    a, b, c = (pre.conic_opacity[:, k].astype(np.float64) for k in range(3))
    dx, dy = target[:, 0] - pre.means2D[:, 0].astype(np.float64), target[:, 1] - pre.means2D[:, 1].astype(np.float64)
    slope = np.abs((a * dx + b * dy) * n[:, 0] + (b * dx + c * dy) * n[:, 1])
    sc = _with_opacity(sc, opacity_at(pre, target, slope * eps_px))
    tx, ty = target[:, 0] // tile, target[:, 1] // tile
    return sc, pre, dict(target=target, eps=eps_px, aimed_tile=(ty * gx + tx).astype(np.int64), sense=r[:, 5], dist=dist)


def _floor(tile, rng, W, H):
    ulps = np.array(FLOOR_ULPS + (None,), dtype=object)
    rows = []
    for u in ulps:
        for corner in (0, 1):
            for sigma in (0.8, 2.0):
                for _ in range(10):
                    # pixels at tile corners as well as anywhere else
                    x = float(rng.integers(0, W - 1)) if rng.random() < 0.5 else float(min(rng.integers(0, -(-W // tile)) * tile, W - 2))
                    y = float(rng.integers(0, H - 1)) if rng.random() < 0.5 else float(min(rng.integers(0, -(-H // tile)) * tile, H - 2))
                    rows.append((x + 0.5 * corner, y + 0.5 * corner, sigma, 1.001 if u is None else 1.0 + u * 2.0 ** -23, corner))
    r = np.array(rows, dtype=np.float64)
    N = r.shape[0]
    sc = _scene(W, H, F_of(tile), r[:, 0:2], r[:, 2], r[:, 2], np.zeros(N), 61 + tile)
    pre = _preprocess(sc, tile)
    sc = _with_opacity(sc, r[:, 3] / 255.0)
    return sc, pre, dict(o255=r[:, 3], on_corner=r[:, 4] == 1)


def _gate(tile, rng, W, H):
    n_needles, n_blobs = 210, 90
    N = n_needles + n_blobs
    needle = np.arange(N) < n_needles
    theta = np.where(needle, np.radians(np.array([30.0, 45.0, 135.0]))[np.arange(N) % 3], rng.uniform(0, math.pi, N))
    sM = np.where(needle, 10.0 ** rng.uniform(3.0, 6.3, N), rng.uniform(1.0, 6.0, N))
    sm = np.where(needle, 0.5, rng.uniform(0.6, 2.0, N))
    centres = np.stack([rng.uniform(0, W - 1, N), rng.uniform(0, H - 1, N)], 1)
    sc = _scene(W, H, F_of(tile), centres, sM, sm, theta, 71 + tile)
    o = oracle_run(sc, tile)
    pre = Pre(o["means2D"].reshape(-1, 2), o["conic_opacity"].reshape(-1, 4), o["radii"])
    sc = _with_opacity(sc, np.where(needle, 0.02, rng.uniform(0.05, 0.6, N)))
    return sc, pre, dict(needle=needle)


_BUILD = dict(graze=_graze, gap=_gap, extreme=_extreme, border=_border, far=_far, floor=_floor, gate=_gate)


@functools.lru_cache(maxsize=None)
def make(name, tile):
    W, H = size_of(name)
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + tile)
    sc, pre, info = _BUILD[name](tile, rng, W, H)
    assert sc.P <= 3000
    return Family(name, tile, W, H, sc, pre, info)


def pairs_of_lists(ranges, point_list, P, keep=None):
    """tile * P + Gaussian of every list position (sorted, unique), or of the positions `keep` marks"""
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    lens = rg[:, 1] - rg[:, 0]
    tile_of = np.zeros(int(np.asarray(point_list).shape[0]), dtype=np.int64)
    for t in np.nonzero(lens)[0]:
        tile_of[rg[t, 0]:rg[t, 1]] = t
    keys = tile_of * max(P, 1) + np.asarray(point_list, dtype=np.int64)
    if keep is not None:
        keys = keys[keep]
    return np.unique(keys)


@functools.lru_cache(maxsize=None)
def reference(name, tile):
    """The oracle's recorded run of make(name, tile) and the model of its preprocess: dict(rect, record, model, pre) - rect:
    the pairs of the oracle's lists, record: those whose entry some pixel blended."""
    fam = make(name, tile)
    o = oracle_run(fam.scene, tile, record=True)
    P = fam.scene.P
    mask = o["contrib_mask"].reshape(-1, 8)
    rect = pairs_of_lists(o["ranges"], o["point_list"], P)
    record = pairs_of_lists(o["ranges"], o["point_list"], P, keep=(mask != 0).any(axis=1))
    mdl = ref.model(o["means2D"], o["conic_opacity"], o["radii"], fam.W, fam.H, tile)
    return dict(rect=rect, record=record, model=mdl, tiles_touched=o["tiles_touched"], R=o["R"],
                pre=Pre(o["means2D"].reshape(-1, 2), o["conic_opacity"].reshape(-1, 4), o["radii"]))
