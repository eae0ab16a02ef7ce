"""The disentangled rasteriser (row f4) against DGR-D's own kernel source, without the restatement in between.

tests/test_dgrd_ref_build_cpu.py holds tests/dgrd_oracle.py to DGR-D's forward.cu / backward.cu / rasterizer_impl.cu
compiled as host C++ (oracle/ref_build.py; the libraries under oracle/_ref/ are all this file reads of them).  Here the
product's two passes (online_lang_splatting_amd/disentangled.py; tests/dgrd_product.py runs them with their state
buffers at hand) are held to the same libraries directly, on the scenes of tests/dgrd_scenes.py:

  * forward with the reference's binning (BINNING_RECT): R1 == R and R2 == R_lang; radii and radii_lang (through
    _merge_radii), n_touched(_lang) and the opacity images; per set point_list, ranges, n_contrib, final_T and the
    per-Gaussian state of the Gaussians that pass sees are EQUAL.  The colour, language and depth images, where the
    product contracts `C += f alpha T` into an fma and the contraction-off build does not, stay within
    2 (n_contrib + 1) 2^-24 max|f| per pixel and channel with each set's own n_contrib.  The public
    LanguageGaussianRasterizer returns the same bits as the two passes;
  * forward with the product's own binning (BINNING_ELLIPSE): images and counters are the same bits as its RECT run;
  * olsr_debug_backward_ordered on pass 1's state with (dL_dcolor, dL_ddepth) and on pass 2's with (zero colour,
    dL_dlanguage, no depth): the eight composite-level tensors EQUAL DGR-D's.  In pass 2 the colour, depth and
    background terms of dL_dalpha are products of a zero cotangent with finite values (1 - alpha >= 0.01, the dummy
    colours are zero): they add +-0;
  * the product's per-Gaussian gradients EQUAL DGR-D's computeCov2DCUDA + computeCov2DCUDA_no_tau +
    language_preprocessCUDA run (refd_backward_chain) on the product's own composite-level gradients of both passes, and
    the pose gradient is the fixed-order sum of that dL_dtau.  DGR-D gates its chain on the merged radii, the product each
    pass on its own: a set with an empty square has zero composite-level gradients, and the outputs agree all the same;
  * the fast composite backward of both passes is within K 2^-24 of each element's condition of the ordered one (row a9).
"""
import functools

import pytest
import torch

import dgrd_product as DP
import dgrd_scenes as S
from online_lang_splatting_amd import _abi
from parity_common import assert_tau_sum_fixed_order, first_difference
from test_dgrd_ref_build_cpu import image_bound

from oracle import oracle_ref_dgrd as Rd

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not Rd.available(), reason="oracle/_ref holds no DGR-D build and the reference tree is absent")]

DEV = "cuda:0"
COUNTERS = ("radii", "n_touched", "opacity")


@functools.lru_cache(maxsize=None)
def _product(hip, name, binning=_abi.BINNING_RECT):
    return DP.run_passes(hip, S.spec(name), S.cotangents(name), torch.device(DEV), binning=binning)


def _eq(a, b, what):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    assert a.numel() == b.numel(), f"{what}: {a.numel()} vs {b.numel()} elements"
    if not a.is_floating_point():
        bad = a.long() != b.long()
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {a.numel()} integers differ, first at {int(bad.nonzero()[0])}"
        return
    d = first_difference(a, b)
    assert d is None, f"{what}: {d[3]} of {a.numel()} elements differ, first at {d[0]}: {d[1]!r} vs {d[2]!r}"


@pytest.fixture(scope="module", params=S.GPU_SCENES)
def case(request):
    name = request.param
    assert Rd.available(S.spec(name)["language"].shape[1]), f"{name}: no DGR-D build for its channel count"
    m = S.conditions(name)
    print(f"\n{name}: {m}")
    return name


def test_forward_equals_dgrd_build(hip, case):
    from online_lang_splatting_amd.disentangled import _merge_radii
    name = case
    s = S.spec(name)
    cam = s["camera"]
    P, W, H = s["means3D"].shape[0], cam.width, cam.height
    fr, _ = S.ref_run(name)
    f = fr["fields"]
    (f1, _), (f2, _) = _product(hip, name)
    assert (f1["R"], f2["R"]) == (fr["R"], fr["R_lang"]), f"{name}: num_rendered"
    radii, radii_lang = _merge_radii(f1["radii"], f2["radii"])
    _eq(radii, fr["radii"], f"{name}: radii")
    _eq(radii_lang, fr["radii_lang"], f"{name}: radii_lang")
    hip.TILE = S.TILE
    nt = ((W + S.TILE - 1) // S.TILE) * ((H + S.TILE - 1) // S.TILE)
    for fp, sfx, F in ((f1, "", 0), (f2, "_lang", s["language"].shape[1])):
        where = f"{name}: set {1 if not sfx else 2}"
        _eq(fp["n_touched"], fr["n_touched" + sfx], f"{where}: n_touched")
        _eq(fp["opacity"], fr["opacity" + sfx], f"{where}: opacity")
        R = fp["R"]
        if R == 0:
            assert name == "all_culled" and not bool((fp["radii"] != 0).any())
            continue
        # the per-Gaussian state, where the pass writes it: the Gaussians whose square of this set covers a tile
        vis = fp["radii"].cpu() > 0
        _eq(vis, f["tiles_touched" + sfx] > 0, f"{where}: which squares cover a tile")
        geo = lambda k, dt, n: hip.state_field("geometry", fp["geom"], k, P=P, F=F, dtype=dt, count=n).cpu()  # noqa: E731
        per_gaussian = [("depths", "depths", torch.float32, 1), ("means2D", "means2D", torch.float32, 2),
                        ("conic_opacity", "conic_opacity" + sfx, torch.float32, 4),
                        ("tiles_touched", "tiles_touched" + sfx, torch.int32, 1)]
        if s.get("cov3D_precomp" + sfx) is None:
            per_gaussian.append(("cov3D", "cov3D" + sfx, torch.float32, 6))
        if not sfx and s.get("colors_precomp") is None:
            per_gaussian += [("rgb", "rgb", torch.float32, 3), ("clamped", "clamped", torch.uint8, 3)]
        for k, kr, dt, w in per_gaussian:
            _eq(geo(k, dt, P * w).view(P, w)[vis], f[kr].view(P, w)[vis], f"{where}: {k} of the visible Gaussians")
        img = lambda k, dt, n: hip.state_field("image", fp["img"], k, W=W, H=H, dtype=dt, count=n).cpu()  # noqa: E731
        _eq(hip.state_field("binning", fp["binning"], "point_list", R=R, F=F, dtype=torch.int32, count=R),
            f["point_list" + sfx], f"{where}: point_list")
        _eq(img("ranges", torch.int32, 2 * nt), f["ranges" + sfx], f"{where}: ranges")
        _eq(img("n_contrib", torch.int32, W * H), f["n_contrib" + sfx], f"{where}: n_contrib")
        _eq(img("final_T", torch.float32, W * H), f["final_T" + sfx], f"{where}: final_T")
    images = dict(color=f1["color"], depth=f1["depth"], language=f2["language"])
    for k, sfx in (("color", ""), ("language", "_lang"), ("depth", "")):
        bound = image_bound(name, fr, k, sfx)
        err = (images[k].cpu().double() - fr[k].double()).abs()
        print(f"{name}: {k}: max |product - DGR-D build| {err.max().item():.3e}, "
              f"smallest margin to the bound {(bound - err).min().item():.3e}")
        assert bool((err <= bound).all()), (f"{name}: {k}: {int((err > bound).sum())} values outside "
                                            f"2 (n_contrib + 1) 2^-24 max|f|, worst excess {(err - bound).max().item():.3e}")


def _public(hip, name, binning):
    """The public module on the scene: its nine outputs."""
    from diff_gaussian_rasterization_disentangle import GaussianRasterizationSettings, LanguageGaussianRasterizer
    s = S.spec(name)
    dev = torch.device(DEV)
    cam = s["camera"]
    hip.BINNING = binning
    rs = GaussianRasterizationSettings(
        image_height=cam.height, image_width=cam.width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=s["bg"].to(dev),
        scale_modifier=s.get("scale_modifier", 1.0), viewmatrix=cam.world_view_transform.to(dev),
        projmatrix=cam.full_proj_transform.to(dev), projmatrix_raw=cam.projection_matrix.to(dev),
        sh_degree=s["sh_degree"], campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
    d = lambda k: None if s.get(k) is None else s[k].to(dev)  # noqa: E731
    pre, pre2, col = s.get("cov3D_precomp") is not None, s.get("cov3D_precomp_lang") is not None, s.get("colors_precomp") is not None
    m = d("means3D")
    with torch.no_grad():
        out = LanguageGaussianRasterizer(raster_settings=rs)(
            means3D=m, means2D=torch.zeros_like(m), opacities=d("opacities"), opacities_lang=d("opacities_lang"),
            shs=None if col else d("shs"), colors_precomp=d("colors_precomp"), language_precomp=d("language"),
            scales=None if pre else d("scales"), scales_lang=None if pre2 else d("scales_lang"),
            rotations=None if pre else d("rotations"), rotations_lang=None if pre2 else d("rotations_lang"),
            cov3D_precomp=d("cov3D_precomp"), cov3D_precomp_lang=d("cov3D_precomp_lang"))
    names = ("color", "language", "radii", "radii_lang", "depth", "opacity", "opacity_lang", "n_touched", "n_touched_lang")
    return dict(zip(names, out))


def test_public_module_and_ellipse_binning_give_the_same_bits(hip, case):
    from online_lang_splatting_amd.disentangled import _merge_radii
    name = case
    (f1, _), (f2, _) = _product(hip, name)
    radii, radii_lang = _merge_radii(f1["radii"], f2["radii"])
    want = dict(color=f1["color"], language=f2["language"], radii=radii, radii_lang=radii_lang, depth=f1["depth"],
                opacity=f1["opacity"], opacity_lang=f2["opacity"], n_touched=f1["n_touched"], n_touched_lang=f2["n_touched"])
    for binning, label in ((_abi.BINNING_RECT, "RECT"), (_abi.BINNING_ELLIPSE, "ELLIPSE")):
        got = _public(hip, name, binning)
        for k in want:
            _eq(got[k], want[k], f"{name}: public module, BINNING_{label}: {k}")


def test_ordered_backward_equals_dgrd_build(hip, case):
    name = case
    _, gr = S.ref_run(name)
    passes = _product(hip, name)
    ordered = DP.assert_fast_is_rounding_only(hip, S.spec(name), passes, S.cotangents(name), name)
    got = DP.dgrd_composite(ordered)
    if name != "all_culled":
        assert any(bool((gr[k] != 0).any()) for k in Rd.COMPOSITE_KEYS)
    for k in Rd.COMPOSITE_KEYS:
        _eq(got[k], gr[k], f"{name}: ordered vs the DGR-D build: {k}")


def test_chain_equals_dgrd_kernels(hip, case):
    name = case
    fr, _ = S.ref_run(name)
    passes = _product(hip, name)
    want = Rd.backward_chain(S.spec(name), fr, DP.dgrd_chain_inputs(passes))
    got = DP.dgrd_chain_outputs(passes)
    for k in Rd.CHAIN_KEYS:
        if want[k].numel():
            _eq(got[k], want[k], f"{name}: chain: {k}")
    if name != "all_culled":
        assert all(bool((want[k] != 0).any()) for k in ("dL_dcov3D_lang",) + (("dL_dcov3D",) if name != "language_only" else ()))
    # theta / rho: the fixed-order sum of pass 1's dL_dtau; set 2 adds nothing to it
    assert_tau_sum_fixed_order(passes[0][1], where=f"{name}: ")
