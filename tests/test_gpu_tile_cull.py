"""The exact tile lists (OLSR_BINNING_ELLIPSE, the product's default) held from BOTH sides by the float64 model of
tests/tile_cull_ref.py on the aimed families of tests/tile_cull_scenes.py:

    core  <=  listed  <=  may            pair for pair

core: the instances the kernel's own definition (cull_* in csrc/olsr_device.h) must list - drop a clause of cull_row_span,
turn a pad inwards or floor a row short and a pair of core is missing; may: the instances its pads can explain - let `exact`
fall to false, double a pad or forget a clip to W - 1 / H - 1 and a listed pair lies outside.  Gaussians outside cull_setup's
gate keep their whole rect.  tests/test_tile_cull_model_cpu.py proves record <= core <= may <= rect on the oracle, so the
chain  record <= core <= listed <= may <= rect  closes here.

Also: tiles_touched[g] - what count_pending_rows (k_preprocess.hip) counted - is the number of list entries
emit_balanced_kernel (k_binning.hip) emitted for g, for every g; and the full parity check of tests/test_gpu_parity.py
(images, sub-list order, liveness flags against the oracle's record) on the same scenes.
"""
import numpy as np
import pytest
import torch

import tile_cull_ref as ref
import tile_cull_scenes as cs
from online_lang_splatting_amd import _abi
from parity_common import run_forward, tile_pairs
from test_gpu_parity import COMPOSITE_GRADS, _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(name, tile) for name in cs.FAMILIES for tile in cs.TILES]


def _show(keys, P, gx, n=5):
    tile, g = ref.split_key(keys[:n], P)
    return [(int(a), int(b % gx), int(b // gx)) for a, b in zip(g, tile)]     # (Gaussian, tile column, tile row)


@pytest.mark.parametrize("name,tile", CASES)
def test_lists_lie_between_core_and_may(hip, oracle, name, tile):
    fam, r = cs.make(name, tile), cs.reference(name, tile)
    m, sc, P = r["model"], fam.scene, fam.scene.P
    f, _ = run_forward(hip, sc, torch.device(DEV), tile, _abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE)
    torch.cuda.synchronize()
    R = int(f["R"])
    # the model's inputs are what the kernels saw: the product's preprocess equals the oracle's bit for bit
    vis = torch.from_numpy(r["pre"].radii > 0)
    assert torch.equal(f["radii"].cpu(), torch.from_numpy(r["pre"].radii))
    for k, w in (("means2D", 2), ("conic_opacity", 4)):
        got = hip.state_field("geometry", f["geom"], k, P=P, F=sc.F, dtype=torch.float32, count=w * P).cpu().view(P, w)
        want = torch.from_numpy(getattr(r["pre"], k))
        same = (got == want) | (got.isnan() & want.isnan())
        if name == "gate":      # (a NaN conic is stored as the record (-0, 0, 0, 1): k_preprocess.hip)
            same = same | want[:, :3].isnan().any(dim=1, keepdim=True)
        assert bool(same[vis].all()), k
    keys = tile_pairs(hip, f, sc, tile)[0].cpu().numpy() if R > 0 else np.zeros(0, dtype=np.int64)
    listed = np.unique(keys)
    assert listed.size == R, "a (Gaussian, tile) pair is listed twice"
    gx = m.gx
    missing, extra = np.setdiff1d(m.core, listed), np.setdiff1d(listed, m.may)
    print(f"{name} tile {tile}: listed={listed.size} core={m.core.size} may={m.may.size} rect={m.rect.size}  "
          f"|listed| / |core| = {listed.size / max(m.core.size, 1):.4f}  |listed| / |rect| = {listed.size / max(m.rect.size, 1):.4f}")
    assert missing.size == 0, f"{missing.size} pairs of core are not listed (Gaussian, column, row): {_show(missing, P, gx)}"
    assert extra.size == 0, f"{extra.size} listed pairs lie outside may (Gaussian, column, row): {_show(extra, P, gx)}"
    # outside the gate: the whole rect, nothing else
    g_listed, g_rect = ref.split_key(listed, P)[1], ref.split_key(m.rect, P)[1]
    assert np.array_equal(listed[m.full[g_listed]], m.rect[m.full[g_rect]])
    if name == "gate":
        assert int(m.full.sum()) >= 10
    # the count (k_preprocess.hip) equals the emission (k_binning.hip), Gaussian by Gaussian
    tt = hip.state_field("geometry", f["geom"], "tiles_touched", P=P, F=sc.F, dtype=torch.int32, count=P).cpu().numpy()
    emitted = np.bincount(g_listed, minlength=P)
    bad = np.nonzero(tt != emitted)[0]
    assert bad.size == 0, f"tiles_touched differs from the emitted entries for Gaussians {bad[:5]}: {tt[bad[:5]]} vs {emitted[bad[:5]]}"
    assert int(tt.sum()) == R


@pytest.mark.parametrize("name,tile", CASES)
def test_parity_on_the_aimed_scenes(hip, oracle, name, tile):
    """Images, radii, n_touched, the sub-list order and the liveness flags against the oracle's record.  Behind the composite
    only the chain on identical inputs is compared, as for the needles of tests/test_gpu_parity.py: these scenes are needles,
    far-away splats and degenerate conics."""
    fam = cs.make(name, tile)
    _check(hip, oracle, fam.scene, seed=tile, tile=tile, check_flags=True, grad_keys=COMPOSITE_GRADS,
           chain_worst_bound=2e-2, chain_min_fraction=0.995)
