"""Scenes that put the FORWARD composite's structural edges where a test wants them (k_render_fwd.hip stages 128 list entries
per fill of its LDS tables and evaluates two entries per iteration; each of its four waves owns one quadrant of the tile and
leaves a batch at the entry where its last pixel saturates).

The layout is that of tests/bwd_batch_scenes.py: tile (0, 0) of a 2 x 2-tile image carries the scene, Gaussian i is list
position i of that tile (depths increase with i), and an entry is "faint" (sigma 0.3 px, opacity 0.01, within 1.5 px of the
tile's centre: it blends one to four pixels and never saturates anything) unless stated otherwise.

Families (cases(tile) lists them, case_id names them):
  stop   s faint entries, then n_walls "gradient walls" at consecutive depths, then `tail` faint entries.  A wall is an
         isotropic Gaussian of sigma 12 px centred on pixel (0, 0) of the tile, opacity 0.999: its alpha falls from the 0.99 cap
         at that corner towards the far corner, so the four quadrants saturate at DIFFERENT walls.  A pixel's terminating entry
         is the wall at 0-based list position n_contrib (the walls follow one another, every one before it blended).  The walls
         are isotropic in 3-D like every Gaussian of bwd_batch_scenes; the perspective Jacobian at the tile's corner, one focal
         length off the axis, stretches their footprint along the tile's diagonal.  With it the largest n_contrib per quadrant is
         s + {4, 9, 9, 10} for 15 x 15 tiles and s + {4, 10, 10, 11} for 16 x 16 tiles (tests/test_fwd_batch_scenes_cpu.py pins
         the coverage these offsets give, not the offsets).  s runs over 0-3 (both pair parities at the head of a list), 114-126
         (every quadrant's stop at list positions 126, 127, 128 and 129: the last pair of the first batch, the first of the
         second) and 242-252 (the same at the second batch boundary); tail is 2 or 300 (saturated waves then leave more than
         two whole batches unread).
  never  100 walls of sigma 5 px between 3 and 200 faint entries: quadrant 0 saturates inside the first batch, the far corner
         of quadrant 3 never does and walks the list of 303 entries to its end while other waves have left.  The 200 entries
         behind the walls lie within 0.4 px of that corner pixel, (tile - 1, tile - 1), which blends every one of them.
  after  s faint entries, then exactly as many walls as quadrant 0 needs (5: its last pixels terminate at the fifth, list position
         s + 4, and (7, 7) is one of them), then 10 faint entries within 0.4 px of pixel (7, 7).  That pixel would blend every
         one of them had it not terminated (with four walls it does; its neighbours terminate at the same wall): the entry that follows a wave's stop entry - the second
         half of its pair, or the first entry of the next batch - must blend nothing and record nothing in that wave, while
         the other three waves, which 5 walls do not saturate, go on.  s = 0, 1 (both halves of a pair), 122, 123, 124 (stop at
         126, at 127 = the last entry of a batch, at 128 = the first).
  skips  a faint stack of N entries in which the entries at chosen positions have opacity 0.003 - below 1/255, they blend
         nowhere: both parities of a pair next to a blending partner, positions 127 and 128, the last entry of an odd list (the
         partner of the odd-tail sentinel), runs longer than a whole batch.  The reference's bounding-square binning lists
         them, the product's exact binning drops them.
  edge   stop(120, 48, 200) on images of 1 x 1, 8 x 8, 9 x 7, (tile + 1) x (tile + 1) and 2 tile x 8 pixels, seen through the
         intrinsics of the 2 x 2-tile image: two or three waves of tile (0, 0) own no pixel inside the image, and the other
         tiles of the (tile + 1)-image are strips one pixel wide.  (The image is far narrower than the field of view the
         intrinsics were made for, so the reference's clamp of x / z at 1.3 tan(fov) takes the stretch out of the walls:
         they are round here, and the quadrants stop at other walls than in `stop`.)
  plain  bwd_batch_scenes.make(N, tile, F, lower, bg) unchanged: lists in which nothing saturates.
"""
from collections import namedtuple

import torch

import bwd_batch_scenes as bs
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import Camera, Scene

TILES = bs.TILES
F_DEFAULT = (0, 3, 15, 16, 32)     # the default instantiation
F_OTHER = (0, 15, 32)              # the accumulation variants, the cut-off instantiation
STOP_S = (0, 1, 2, 3) + tuple(range(114, 127)) + tuple(range(242, 253))
STOP_TAILS = (2, 300)
STOP_WALLS = 48
WALL_SIGMA_PX = 12.0
WALL_OPACITY = 0.999
NEVER_WALLS, NEVER_SIGMA_PX, NEVER_S, NEVER_TAIL = 100, 5.0, 3, 200
NEVER_TAIL_JITTER_PX = 0.4
SKIP_OPACITY = 0.003               # 255 x 0.003 < 1: alpha stays below 1/255 everywhere
EDGE_STOP = (120, 48, 200)
# The pinhole formula u = fx x / z + cx with cx = (W - 1) / 2 (default_camera) names a point that the rasteriser's ndc2Pix puts
# at pixel coordinate u - 0.5.  bwd_batch_scenes places its Gaussians with that formula, and so do the faint entries and the
# walls here: "the tile's centre" and "pixel (0, 0)" above are half a pixel further up and left (the walls' centre lies at
# (-0.5, -0.5), just outside the tile's corner pixel).  The two tails that must sit ON a pixel add the half pixel back.
HALF_PIXEL = 0.5
AFTER_S, AFTER_WALLS, AFTER_TAIL_N, AFTER_PIXEL = (0, 1, 122, 123, 124), 5, 10, (7, 7)
AFTER_TAIL = (7.0, 7.0, 0.4)       # centre and jitter of the entries behind the walls

FAINT, WALL, SKIP = 0, 1, 2
# the forward's other accumulations (include/olsr.h), as the golden file names them
ACCUM_VARIANTS = (("mfma", _abi.FLAG_FWD_ACCUM_MFMA), ("weight", _abi.FLAG_FWD_ACCUM_WEIGHT))
IMAGE_KEYS = ("color", "language", "depth", "opacity")

# family, list description, image size (None: 2 x 2 tiles), the plain stack's (N, lower, bg)
Case = namedtuple("Case", "family name s n_walls tail sigma N skips wh plain")


def _case(family, name, s=0, n_walls=0, tail=0, sigma=WALL_SIGMA_PX, N=0, skips=(), wh=None, plain=None):
    return Case(family, name, s, n_walls, tail, sigma, N, tuple(skips), wh, plain)


def _skip_patterns(N):
    """name -> positions of the 0.003 entries in a list of N"""
    even, odd = tuple(range(0, N, 2)), tuple(range(1, N, 2))
    pats = {
        1: {"none": (), "p0": (0,)},
        2: {"p0": (0,), "p1": (1,)},
        3: {"p0": (0,), "p1": (1,), "p2": (2,), "even": even},
        4: {"p1": (1,), "p2": (2,), "p0p3": (0, 3)},
        5: {"p4": (4,), "even": even, "odd": odd},
        127: {"p126": (126,), "even": even, "odd": odd},
        128: {"p127": (127,), "p126": (126,), "even": even, "odd": odd},
        129: {"p127": (127,), "p128": (128,), "p127p128": (127, 128), "even": even, "odd": odd},
        130: {"p128": (128,), "p129": (129,), "p127p128": (127, 128)},
        255: {"p254": (254,), "p127": (127,), "p128": (128,), "run100": tuple(range(100, 241))},
        256: {"p255": (255,), "run64": tuple(range(64, 201)), "even": even, "odd": odd},
        257: {"p256": (256,), "run126": tuple(range(126, 257)), "p127p128": (127, 128)},
    }
    return pats[N]


SKIP_N = (1, 2, 3, 4, 5, 127, 128, 129, 130, 255, 256, 257)


def edge_sizes(tile):
    return ((1, 1), (8, 8), (9, 7), (tile + 1, tile + 1), (2 * tile, 8))


def cases(tile, families=("stop", "never", "after", "skips", "edge", "plain")):
    out = []
    if "stop" in families:
        for s in STOP_S:
            for tail in STOP_TAILS:
                out.append(_case("stop", f"stop_s{s}_w{STOP_WALLS}_t{tail}", s=s, n_walls=STOP_WALLS, tail=tail))
    if "never" in families:
        out.append(_case("never", "never", s=NEVER_S, n_walls=NEVER_WALLS, tail=NEVER_TAIL, sigma=NEVER_SIGMA_PX))
    if "after" in families:
        for s in AFTER_S:
            out.append(_case("after", f"after_s{s}", s=s, n_walls=AFTER_WALLS, tail=AFTER_TAIL_N))
    if "skips" in families:
        for N in SKIP_N:
            for name, pos in _skip_patterns(N).items():
                out.append(_case("skips", f"skips_N{N}_{name}", N=N, skips=pos))
    if "edge" in families:
        s, n_walls, tail = EDGE_STOP
        for w, h in edge_sizes(tile):
            out.append(_case("edge", f"edge_{w}x{h}", s=s, n_walls=n_walls, tail=tail, wh=(w, h)))
    if "plain" in families:
        for N in bs.N_VALUES:
            for lower, bg in bs.VARIANTS:
                out.append(_case("plain", f"plain_N{N}_l{int(lower)}_b{int(bg)}", N=N, plain=(N, lower, bg)))
    return out


def case_id(tile, F, case, inst=""):
    return f"t{tile}_F{F}_{case.name}" + (f"_{inst}" if inst else "")


def kinds(case):
    """FAINT / WALL / SKIP per list position, front to back (None for the plain stacks: bwd_batch_scenes.layout has them)"""
    if case.family == "plain":
        return None
    if case.family == "skips":
        k = [FAINT] * case.N
        for p in case.skips:
            k[p] = SKIP
        return k
    return [FAINT] * case.s + [WALL] * case.n_walls + [FAINT] * case.tail


def make(case, tile, F):
    """The scene (CPU tensors; Gaussian i is list position i of tile (0, 0)) and kinds(case)."""
    if case.family == "plain":
        N, lower, bg = case.plain
        sc, _ = bs.make(N, tile, F, lower, bg)
        return sc, None
    kind = kinds(case)
    L = len(kind)
    W, H = case.wh if case.wh is not None else (2 * tile, 2 * tile)
    # the intrinsics of default_camera(2 tile, 2 tile), whatever the image's size
    cam = Camera(W, H, float(tile), float(tile), (2 * tile - 1) / 2.0, (2 * tile - 1) / 2.0)
    seed = 104729 * tile + 31 * F + sum(ord(c) * (i + 1) for i, c in enumerate(case.name))
    g = torch.Generator().manual_seed(seed)
    z = 1.0 + 2.0 * (torch.arange(L, dtype=torch.float32) + 0.25 * torch.rand(L, generator=g)) / max(L, 1)
    kt = torch.tensor(kind)
    centre = tile / 2.0
    u = centre + 2.0 * bs.JITTER_PX * (torch.rand(L, generator=g) - 0.5)
    v = centre + 2.0 * bs.JITTER_PX * (torch.rand(L, generator=g) - 0.5)
    wall = kt == WALL
    u = torch.where(wall, torch.zeros(L), u)
    v = torch.where(wall, torch.zeros(L), v)
    if case.family in ("never", "after"):
        # the tail sits on one pixel: the far corner of quadrant 3, the only one still live / the last one of quadrant 0 to stop
        px, py, jit = (tile - 1, tile - 1, NEVER_TAIL_JITTER_PX) if case.family == "never" else AFTER_TAIL
        behind = torch.arange(L) >= case.s + case.n_walls
        u = torch.where(behind, px + HALF_PIXEL + 2.0 * jit * (torch.rand(L, generator=g) - 0.5), u)
        v = torch.where(behind, py + HALF_PIXEL + 2.0 * jit * (torch.rand(L, generator=g) - 0.5), v)
    x = (u - cam.cx) * z / cam.fx
    y = (v - cam.cy) * z / cam.fy
    means3D = torch.stack([x, y, z], dim=1).contiguous()
    sigma = torch.where(wall, torch.full((L,), float(case.sigma)), torch.full((L,), bs.SIGMA_PX))
    scales = (sigma * z / cam.fx).unsqueeze(1).repeat(1, 3).contiguous()
    rotations = torch.zeros(L, 4)
    rotations[:, 0] = 1.0
    opacities = torch.full((L, 1), 0.01)
    opacities[wall] = WALL_OPACITY
    opacities[kt == SKIP] = SKIP_OPACITY
    shs = (torch.rand(L, 1, 3, generator=g) * 3.0 - 1.5).contiguous()
    language = None
    if F > 0:
        l = torch.randn(L, F, generator=g)
        language = (l / l.norm(dim=1, keepdim=True)).contiguous()
    return Scene(cam, means3D, opacities, scales, rotations, shs, language, 0, torch.zeros(3), F), kind


def digest(images):
    """bwd_batch_scenes.digest over the images of a forward dict (SHA-256 of the fp32 bits, keys in sorted order; -0 counts as
    +0)."""
    return bs.digest({k: images[k] for k in IMAGE_KEYS if images.get(k) is not None})


def quadrant_of_rank(rank, tile):
    """the forward wave (slot_rank, csrc/olsr_device.h) that owns tile rank `rank` = row * tile + column"""
    return (rank // tile >= 8) * 2 + (rank % tile >= 8)


def _rank_tables(tile):
    import numpy as np
    r = np.arange(256)
    valid = r < tile * tile
    quad = np.where(valid, (r // tile >= 8) * 2 + (r % tile >= 8), -1)
    surv = valid & (r < 224) & np.isin(r % 7, (0, 1, 3, 4)) & (tile == 15)
    return quad, surv & (r < 112), surv & (r >= 112)


def expected_flags(contrib_mask, tile):
    """The flag byte of every list entry from the oracle's record (oracle_set_record(1): 256 bits per sorted list position,
    bit `rank` set when the pixel of that tile rank blended the entry).  Bit q (0..3): some blending rank lies in quadrant q.
    15 x 15 tiles only: bit 4 / bit 5: some blending rank survives the reference's reduction tree (rank < 224 and rank % 7 in
    {0, 1, 3, 4}) with rank below 112 / from 112 up - the two packed waves of the reference-mode backward."""
    import numpy as np
    words = contrib_mask.numpy().astype(np.uint32).reshape(-1, 8)
    bits = np.unpackbits(words.view(np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(bool)   # [R, 256], bit = rank
    quad, w0, w1 = _rank_tables(tile)
    fl = np.zeros(bits.shape[0], dtype=np.uint8)
    for q in range(4):
        fl |= (bits[:, quad == q].any(axis=1).astype(np.uint8) << q)
    fl |= bits[:, w0].any(axis=1).astype(np.uint8) << 4
    fl |= bits[:, w1].any(axis=1).astype(np.uint8) << 5
    return torch.from_numpy(fl)


def expected_tile_work(flags, ranges):
    """tile_work[2][tiles] from per-position flags and the tiles' list ranges [tiles, 2]: the number of set bits 0-3, then the
    number of set bits 4-5, over each tile's list."""
    nt = ranges.shape[0]
    tw = torch.zeros(2, nt, dtype=torch.int64)
    f = flags.long()
    slots = (f & 1) + ((f >> 1) & 1) + ((f >> 2) & 1) + ((f >> 3) & 1)
    packed = ((f >> 4) & 1) + ((f >> 5) & 1)
    for t in range(nt):
        a, b = int(ranges[t, 0]), int(ranges[t, 1])
        if b > a:
            tw[0, t] = int(slots[a:b].sum())
            tw[1, t] = int(packed[a:b].sum())
    return tw


def expected_blended(flags, point_list, P):
    """blended[g] = 1 exactly for the Gaussians with a non-zero flag somewhere"""
    bl = torch.zeros(P, dtype=torch.uint8)
    bl[point_list.long()[flags != 0]] = 1
    return bl
