"""The scene of tests/test_gpu_bwd_sums.py: about 4000 isotropic Gaussians of chosen pixel radii on 320 x 240 pixels, laid out
so that the row sums of the per-Gaussian backward (csrc/k_preprocess_bwd.hip) take every path they have.

  occluders  four layers of opaque blobs (sigma 20 pixels, a 20-pixel grid) over the left 130 pixel columns: each is listed
             in about 80 tiles - the front list of big_list, runs of more than 64 rows - and behind the second layer the
             pixels are saturated: the deeper layers' inner blobs are listed and have no row.
  hidden     blobs of sigma 10 pixels, opacity 0.5, behind the occluders and wholly inside the saturated region: listed in
             about 20 tiles each, not one row.
  listed     sigma 10.5 .. 24 pixels at opacity 0.03 (nothing saturates: the alpha >= 1/255 contour lies at 2 sigma) on the
             right 170 columns: 13 .. 40 tiles, both work lists.
  small      sigma 0.6 .. 10.5 pixels, same place and opacity: 1 .. 12 tiles, summed inline.

More than 2 * 1024 Gaussians are listed in more than OLSR_MID_FOOTPRINT tiles, so that a wave of row_reduce_big_kernel's
persistent grid (1024 waves at this P) takes three items: its hand-written pipeline runs full.  The index order is a random
permutation: Gaussians without rows lie between ones with rows everywhere in the lists.

`facts(sc, tile)` computes what the GPU test asserts about the frame - on the CPU, from the oracle's recorded forward and the
float64 tile-list model of the ellipse binning (tests/tile_cull_ref.py); tests/test_bwd_sums_ref_cpu.py holds the scene to
them before any GPU sees it."""
import functools

import numpy as np
import torch

import tile_cull_ref as tref
from parity_common import fwd_args  # noqa: F401  (first: it puts the repository root on sys.path)
from online_lang_splatting_amd.scene import Scene, default_camera

W, H = 320, 240
TILE_COUNTS = (1, 12, 13, 32, 33)     # footprints that must exist with rows: both sides of both thresholds, and one tile
N_OCC_LAYERS, N_HIDDEN, N_LISTED, N_SMALL = 4, 150, 2400, 900


@functools.lru_cache(maxsize=None)
def make(F, seed=0):
    """The scene with F language channels (the geometry does not depend on F)."""
    rng = np.random.default_rng(4100 + seed)
    gx, gy = np.meshgrid(np.arange(5.0, 130.0, 20.0), np.arange(0.0, 241.0, 20.0))
    grid = np.stack([gx.reshape(-1), gy.reshape(-1)], 1)
    parts = []          # (centres [n, 2], sigma [n], opacity [n], depth [n])
    for layer in range(N_OCC_LAYERS):
        n = grid.shape[0]
        parts.append((grid, np.full(n, 20.0), np.full(n, 1.0), 1.0 + 0.05 * layer + 0.04 * rng.random(n)))
    n = N_HIDDEN
    parts.append((np.stack([rng.uniform(40, 65, n), rng.uniform(45, 195, n)], 1), np.full(n, 10.0), np.full(n, 0.5),
                  2.0 + 0.1 * rng.random(n)))
    for n, lo, hi in ((N_LISTED, 10.5, 24.0), (N_SMALL, 0.6, 10.5)):
        parts.append((np.stack([rng.uniform(150, 325, n), rng.uniform(-5, 245, n)], 1), rng.uniform(lo, hi, n),
                      np.full(n, 0.03), 3.0 + rng.random(n)))
    c, sig, op, z = (np.concatenate([p[k] for p in parts]) for k in range(4))
    perm = rng.permutation(c.shape[0])
    c, sig, op, z = c[perm], sig[perm], op[perm], z[perm]
    cam = default_camera(W, H)
    N = c.shape[0]
    # ndc2Pix puts the pinhole point u = fx x / z + cx at pixel coordinate u - 0.5
    x = (c[:, 0] + 0.5 - cam.cx) * z / cam.fx
    y = (c[:, 1] + 0.5 - cam.cy) * z / cam.fy
    means3D = torch.from_numpy(np.stack([x, y, z], 1)).float().contiguous()
    scales = torch.from_numpy(np.repeat((sig * z / cam.fx)[:, None], 3, 1)).float().contiguous()
    rot = torch.zeros(N, 4)
    rot[:, 0] = 1.0
    g = torch.Generator().manual_seed(4200 + seed)
    shs = (torch.rand(N, 1, 3, generator=g) * 3.0 - 1.5).contiguous()
    language = None
    if F > 0:
        l = torch.randn(N, F, generator=g)
        language = (l / l.norm(dim=1, keepdim=True)).contiguous()
    opac = torch.from_numpy(op).float().reshape(N, 1).contiguous()
    return Scene(cam, means3D, opac, scales, rot, shs, language, 0, torch.zeros(3), F)


@functools.lru_cache(maxsize=None)
def facts(tile, seed=0):
    """What the frame of make(., seed) at this tile edge must look like, from the oracle and the float64 model alone:
    dict(P, n_core, n_may [P]: tiles per Gaussian of the ellipse lists' two bounds, recorded [P]: tiles in which some pixel
    blended the Gaussian)."""
    import tile_cull_scenes as cs
    sc = make(3, seed)
    o = cs.oracle_run(sc, tile, record=True)
    P = sc.P
    mask = o["contrib_mask"].reshape(-1, 8)
    rec = cs.pairs_of_lists(o["ranges"], o["point_list"], P, keep=(mask != 0).any(axis=1))
    m = tref.model(o["means2D"], o["conic_opacity"], o["radii"], W, H, tile)
    count = lambda keys: np.bincount(tref.split_key(keys, P)[1], minlength=P)  # noqa: E731
    assert tref.is_subset(rec, m.core) and tref.is_subset(m.core, m.may)
    return dict(P=P, n_core=count(m.core), n_may=count(m.may), recorded=count(rec))
