"""Scenes for the forward composite's per-wave hit records (k_render_fwd.hip keeps a wave's records of a 128-entry batch in
one vector register - lane l: entries 2 l and 2 l + 1 - and writes them to LDS once per batch; the flush turns them into
flags[], blended[], n_touched and tile_work).  Built with the helpers of tests/fwd_batch_scenes.py: tile (0, 0) of a 2 x 2-tile
image carries the scene, Gaussian i is list position i of that tile.

The batch positions that matter are the lane boundaries of that register and the ends of a batch: POSITIONS = 62, 63, 64, 65,
126, 127 (lanes 31 | 32 and lane 63, both halves).

Families (cases(tile) lists them):
  plan   a faint stack (fwd_batch_scenes' `skips` family without skips) of N entries in which the entries at chosen list
         positions are replaced by
           ONE w   a faint entry (opacity 0.01) centred on pixel WAVE_PIXEL[w]: exactly that pixel blends it - one wave;
           ALL     an entry of opacity 0.3 centred on the corner the four quadrants share, (7.5, 7.5): all four waves blend it;
           NONE    an entry of opacity 0.005 centred between four pixels: its alpha >= 1/255 disc (radius 0.44 px) holds no
                   pixel centre - it is in the reference's list and no pixel blends it.
         one_r<k>  POSITIONS[i] -> ONE (i + k) % 4, k = 0..3: every position by every wave alone; N = 131 (odd tail of 3)
         all       POSITIONS -> ALL; N = 129 (odd tail of 1)
         none      POSITIONS -> NONE; N = 133 (odd tail of 5)
         stale_*   N = 257 (two whole batches and a tail of 1): what a wave records at position p of batch 0 it must not
                   report at position p of batch 1, and the other way round:
                     stale_one_none  batch 0: ONE, batch 1: NONE        stale_none_one  the reverse
                     stale_one_other batch 0: ONE w, batch 1: ONE w + 1  stale_all_one   batch 0: ALL, batch 1: ONE
                     stale_all_none  batch 0: ALL, batch 1: NONE
  stop   fwd_batch_scenes' `stop` family, 16 walls, a tail of 3 or 4 (whichever makes the list odd): s chosen so that quadrant 0 (offset 4) and
         quadrant 3 (offset 10 for 15 x 15 tiles, 11 for 16 x 16) saturate their last pixel at each of POSITIONS.
"""
from collections import namedtuple

import fwd_batch_scenes as fs

TILES = fs.TILES
F_VALUES = (0, 15, 32)
POSITIONS = (62, 63, 64, 65, 126, 127)
WAVE_PIXEL = ((3, 3), (11, 3), (3, 11), (11, 11))   # (x, y): a pixel well inside quadrant w of either tile size
SHARED_CORNER = (7.5, 7.5)                          # between pixels (7, 7), (8, 7), (7, 8), (8, 8): one of each quadrant
HOLE = (4.5, 4.5)                                   # between four pixels of quadrant 0
ONE_OPACITY, ALL_OPACITY, NONE_OPACITY = 0.01, 0.3, 0.005
STOP_WALLS, STOP_TAIL = 16, 3
STOP_OFFSETS = {15: (4, 10), 16: (4, 11)}           # (quadrant 0, quadrant 3): tests/test_fwd_batch_scenes_cpu.py
STOP_QUADRANTS = (0, 3)
BATCH = 128

# plan: {list position: ("one", w) | ("all",) | ("none",)};  stop: (quadrant, position) for the stop family, else None
HitCase = namedtuple("HitCase", "name base plan stop")


def _plan_case(name, N, plan):
    return HitCase(name, fs._case("skips", "hit_" + name, N=N), dict(plan), None)


def cases(tile):
    out = []
    for k in range(4):
        out.append(_plan_case(f"one_r{k}", 131, {p: ("one", (i + k) % 4) for i, p in enumerate(POSITIONS)}))
    out.append(_plan_case("all", 129, {p: ("all",) for p in POSITIONS}))
    out.append(_plan_case("none", 133, {p: ("none",) for p in POSITIONS}))
    b0 = {p: ("one", i % 4) for i, p in enumerate(POSITIONS)}
    two = lambda first, second: {**first, **{BATCH + p: v for p, v in second.items()}}   # noqa: E731
    out.append(_plan_case("stale_one_none", 257, two(b0, {p: ("none",) for p in POSITIONS})))
    out.append(_plan_case("stale_none_one", 257, two({p: ("none",) for p in POSITIONS}, b0)))
    out.append(_plan_case("stale_one_other", 257, two(b0, {p: ("one", (i + 1) % 4) for i, p in enumerate(POSITIONS)})))
    out.append(_plan_case("stale_all_one", 257, two({p: ("all",) for p in POSITIONS}, b0)))
    out.append(_plan_case("stale_all_none", 257, two({p: ("all",) for p in POSITIONS}, {p: ("none",) for p in POSITIONS})))
    for q, off in zip(STOP_QUADRANTS, STOP_OFFSETS[tile]):
        for p in POSITIONS:
            tail = STOP_TAIL + (p - off + STOP_WALLS + STOP_TAIL + 1) % 2   # (an odd list: the last pair is half sentinel)
            base = fs._case("stop", f"hit_stop_q{q}_p{p}", s=p - off, n_walls=STOP_WALLS, tail=tail)
            out.append(HitCase(f"stop_q{q}_p{p}", base, {}, (q, p)))
    return out


def case_id(tile, F, case):
    return f"t{tile}_F{F}_{case.name}"


def _place(sc, i, x_pix, y_pix, opacity):
    """Gaussian i centred on pixel coordinate (x_pix, y_pix) of the rasteriser (fwd_batch_scenes.HALF_PIXEL), its depth kept"""
    cam = sc.camera
    z = float(sc.means3D[i, 2])
    sc.means3D[i, 0] = (x_pix + fs.HALF_PIXEL - cam.cx) * z / cam.fx
    sc.means3D[i, 1] = (y_pix + fs.HALF_PIXEL - cam.cy) * z / cam.fy
    sc.opacities[i, 0] = opacity


def make(case, tile, F):
    """The scene (CPU tensors; Gaussian i is list position i of tile (0, 0))."""
    sc, _ = fs.make(case.base, tile, F)
    for p, what in case.plan.items():
        if what[0] == "one":
            _place(sc, p, WAVE_PIXEL[what[1]][0], WAVE_PIXEL[what[1]][1], ONE_OPACITY)
        elif what[0] == "all":
            _place(sc, p, SHARED_CORNER[0], SHARED_CORNER[1], ALL_OPACITY)
        else:
            _place(sc, p, HOLE[0], HOLE[1], NONE_OPACITY)
    return sc


def list_length(case):
    b = case.base
    return b.N if b.family == "skips" else b.s + b.n_walls + b.tail
