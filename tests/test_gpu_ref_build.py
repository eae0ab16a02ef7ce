"""The HIP kernels against the reference's own kernel source, without the oracle in between.

tests/test_ref_build_cpu.py holds the oracle to the reference's forward.cu / backward.cu / rasterizer_impl.cu compiled
as host C++ (oracle/ref_build.py; the libraries under oracle/_ref/ are all this file reads of them).  Here the product
is held to the same libraries directly, on the dense, ragged and precomputed scenes of tests/ref_scenes.py and on one
scene without language, at both tile sizes:

  * the product's forward with the reference's binning (BINNING_RECT): num_rendered, radii, n_touched, the per-Gaussian
    state of every visible Gaussian, point_list, ranges, n_contrib, final_T and the opacity image are EQUAL; the colour,
    language and depth images, where the product contracts `C += f alpha T` into an fma as nvcc would and the
    contraction-off reference build does not, stay within 2 (n_contrib + 1) 2^-24 max|f| per pixel and channel (both add
    the same terms, sum of alpha T <= 1, one rounding apart per term);
  * olsr_debug_backward_ordered on that state and the same cotangents: the six composite-level tensors EQUAL the
    reference build's (blocks in ascending tile order there, which is the ordered kernel's order);
  * the product's per-Gaussian outputs EQUAL the reference's computeCov2DCUDA + preprocessCUDA run (backward_chain) on the
    product's own composite-level gradients.
"""
import functools

import pytest
import torch

import ref_scenes as S
from online_lang_splatting_amd import _abi
from parity_common import (COMPOSITE_KEYS, assert_ordered_equals_oracle, first_difference, ordered_backward,
                           run_backend)

from oracle import oracle_ref

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not oracle_ref.available(),
                                 reason="oracle/_ref holds no reference build and the reference tree is absent")]

DEV = "cuda:0"
CASES = [pytest.param((name, tile), id=f"{name}-t{tile}") for name, tiles in S.GPU_SCENES for tile in tiles]


@functools.lru_cache(maxsize=None)
def _product(hip, name, tile):
    sp = S.spec(name)
    fg, gg = run_backend(hip, sp.scene, torch.device(DEV), S.SEED, tile, _abi.BWD_REFERENCE, binning=_abi.BINNING_RECT,
                         **sp.kw)
    torch.cuda.synchronize()
    return fg, gg


def _eq(a, b, what):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    assert a.numel() == b.numel(), f"{what}: {a.numel()} vs {b.numel()} elements"
    if not a.is_floating_point():
        bad = a.long() != b.long()
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {a.numel()} integers differ, first at {int(bad.nonzero()[0])}"
        return
    d = first_difference(a, b)
    assert d is None, f"{what}: {d[3]} of {a.numel()} elements differ, first at {d[0]}: {d[1]!r} vs {d[2]!r}"


@pytest.fixture(scope="module", params=CASES)
def case(request):
    name, tile = request.param
    assert oracle_ref.available(tile, S.spec(name).scene.F), f"no reference build for tile {tile}"
    m = S.conditions(name, tile)
    print(f"\n{name} tile {tile}: {m}")
    return name, tile


def test_forward_equals_reference_build(hip, case):
    name, tile = case
    sp = S.spec(name)
    sc = sp.scene
    P, F, W, H = sc.P, sc.F, sc.camera.width, sc.camera.height
    fg, _ = _product(hip, name, tile)
    fr, _ = S.ref_run(name, tile)
    st = fr["state"]
    where = f"{name} tile {tile}"
    assert fg["R"] == fr["R"] > 0, f"{where}: num_rendered {fg['R']} vs {fr['R']}"
    R = fr["R"]
    for k in ("radii", "n_touched", "opacity"):
        _eq(fg[k], fr[k], f"{where}: {k}")
    # the per-Gaussian state, where the reference writes it: the rows of the visible Gaussians (it leaves the others
    # unwritten), rgb and clamped when colours come from SH, cov3D when it comes from scales and rotations
    hip.TILE = tile
    vis = fr["radii"] > 0
    assert 0 < int(vis.sum())
    geo = lambda k, dt, n: hip.state_field("geometry", fg["geom"], k, P=P, F=F, dtype=dt, count=n).cpu()  # noqa: E731
    per_gaussian = [("depths", torch.float32, 1), ("means2D", torch.float32, 2), ("conic_opacity", torch.float32, 4),
                    ("tiles_touched", torch.int32, 1)]
    if "cov3D_precomp" not in sp.kw:
        per_gaussian.append(("cov3D", torch.float32, 6))
    if "colors_precomp" not in sp.kw:
        per_gaussian += [("rgb", torch.float32, 3), ("clamped", torch.uint8, 3)]
    for k, dt, w in per_gaussian:
        _eq(geo(k, dt, P * w).view(P, w)[vis], st[k].view(P, w)[vis], f"{where}: {k} of the visible Gaussians")
    nt = ((W + tile - 1) // tile) * ((H + tile - 1) // tile)
    img = lambda k, dt, n: hip.state_field("image", fg["img"], k, W=W, H=H, dtype=dt, count=n).cpu()  # noqa: E731
    _eq(hip.state_field("binning", fg["binning"], "point_list", R=R, F=F, dtype=torch.int32, count=R), st["point_list"],
        f"{where}: point_list")
    _eq(img("ranges", torch.int32, 2 * nt), st["ranges"], f"{where}: ranges")
    _eq(img("n_contrib", torch.int32, W * H), st["n_contrib"], f"{where}: n_contrib")
    _eq(img("final_T", torch.float32, W * H), st["final_T"], f"{where}: final_T")
    for k in ("color", "language", "depth"):
        if fr[k] is None or fr[k].numel() == 0:
            continue
        bound = S.image_bound(name, fr, k)
        err = (fg[k].cpu().double() - fr[k].double()).abs()
        print(f"{where}: {k}: max |product - reference build| {err.max().item():.3e}, "
              f"smallest margin to the bound {(bound - err).min().item():.3e}")
        assert bool((err <= bound).all()), (f"{where}: {k}: {int((err > bound).sum())} values outside "
                                            f"2 (n_contrib + 1) 2^-24 max|f|, worst excess {(err - bound).max().item():.3e}")


def test_ordered_backward_equals_reference_build(hip, case):
    name, tile = case
    sp = S.spec(name)
    fg, _ = _product(hip, name, tile)
    _, gr = S.ref_run(name, tile)
    gord = ordered_backward(hip, sp.scene, fg, S.SEED, tile, _abi.BWD_REFERENCE, **sp.kw)
    assert any(gr[k].numel() and bool((gr[k] != 0).any()) for k in COMPOSITE_KEYS)
    assert_ordered_equals_oracle(gr, gord, where=f"{name} tile {tile}: ordered vs the reference build: ")


def test_chain_equals_reference_kernels(hip, case):
    name, tile = case
    sp = S.spec(name)
    _, gg = _product(hip, name, tile)
    fr, _ = S.ref_run(name, tile)
    oracle_ref.TILE = tile
    comp = {k: gg[k] for k in ("dL_dmeans2D", "dL_dconic", "dL_dcolors", "dL_ddepths")}
    want = oracle_ref.backward_chain(max(sp.scene.F, 0), comp, *fr["bwd_args"])
    for k in oracle_ref.CHAIN_KEYS:
        if want[k].numel():
            _eq(gg[k], want[k], f"{name} tile {tile}: chain: {k}")
    assert any(bool((want[k] != 0).any()) for k in oracle_ref.CHAIN_KEYS)
