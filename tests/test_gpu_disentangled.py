"""Row f4: the disentangled-language rasterizer (online_lang_splatting_amd/disentangled.py, shim package
diff_gaussian_rasterization_disentangle) against tests/dgrd_oracle.py, the restatement that
tests/test_dgrd_ref_build_cpu.py holds to DGR-D's own kernel source.

The forward is compared bit for bit.  The backward is held to the criteria of rows a9 and a10, for both passes:
the public module's twelve gradients are the bits of the two passes run at the `_C` level (tests/dgrd_product.py); the
ordered composite kernel on each pass's state EQUALS the restatement's composite-level gradients; the fast composite kernel
lies within K 2^-24 of each element's condition of the ordered one; and the per-Gaussian gradients EQUAL the restatement's
chain run on the product's own composite-level gradients."""
import pytest
import torch

from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import make_scene
from dgrd_scenes import scene2
from parity_common import first_difference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scene2(P, W, H, F=3, seed=0, border=False):
    """A make_scene scene plus a second opacity / scale / rotation set (tests/dgrd_scenes.py: scene2)."""
    return scene2(P, W, H, F, seed, border)


def _settings(s, dev):
    from diff_gaussian_rasterization_disentangle import GaussianRasterizationSettings
    cam = s["camera"]
    return GaussianRasterizationSettings(
        image_height=cam.height, image_width=cam.width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=s["bg"].to(dev),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        projmatrix_raw=cam.projection_matrix.to(dev), sh_degree=s["sh_degree"], campos=cam.camera_center.to(dev),
        prefiltered=False, debug=False)


def _run_product(s, dev, seed, cot):
    from diff_gaussian_rasterization_disentangle import LanguageGaussianRasterizer
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)  # noqa: E731
    names = ("means3D", "opacities", "opacities_lang", "scales", "scales_lang", "rotations", "rotations_lang", "shs",
             "language")
    L = {n: leaf(s[n]) for n in names}
    means2D = torch.zeros_like(L["means3D"], requires_grad=True)
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    rast = LanguageGaussianRasterizer(raster_settings=_settings(s, dev))
    out = rast(means3D=L["means3D"], means2D=means2D, opacities=L["opacities"], opacities_lang=L["opacities_lang"],
               shs=L["shs"], colors_precomp=None, language_precomp=L["language"], scales=L["scales"],
               scales_lang=L["scales_lang"], rotations=L["rotations"], rotations_lang=L["rotations_lang"],
               cov3D_precomp=None, cov3D_precomp_lang=None, theta=theta, rho=rho)
    color, language, radii, radii_lang, depth, opacity, opacity_lang, n_touched, n_touched_lang = out
    dc, dl, dd = (t.to(dev) for t in cot)
    # the opacity images take part in the loss but, like in the reference, carry no gradient
    loss = (color * dc).sum() + (language * dl).sum() + (depth * dd).sum() + 0.3 * opacity.sum() + 0.2 * opacity_lang.sum()
    loss.backward()
    grads = {n: L[n].grad for n in names}
    grads.update(means2D=means2D.grad, theta=theta.grad, rho=rho.grad)
    fwd = dict(color=color, language=language, radii=radii, radii_lang=radii_lang, depth=depth, opacity=opacity,
               opacity_lang=opacity_lang, n_touched=n_touched, n_touched_lang=n_touched_lang)
    return {k: v.detach().cpu() for k, v in fwd.items()}, {k: v.detach().cpu() for k, v in grads.items()}


def _cot(s, F, seed):
    g = torch.Generator().manual_seed(99 + seed)
    H, W = s["camera"].height, s["camera"].width
    n = float(H * W)
    return (torch.randn(3, H, W, generator=g) / n, torch.randn(F, H, W, generator=g) / n,
            torch.randn(1, H, W, generator=g) / n)


@pytest.mark.parametrize("binning", [_abi.BINNING_RECT, _abi.BINNING_ELLIPSE])
@pytest.mark.parametrize("P,W,H,F,seed,border", [(4000, 200, 150, 3, 11, False), (3000, 173, 131, 3, 12, True),
                                                  (2500, 160, 120, 15, 13, True)])
def test_disentangled_rasterizer_matches_the_oracle(hip, oracle, P, W, H, F, seed, border, binning):
    import dgrd_oracle as D
    dev = torch.device(DEV)
    s = _scene2(P, W, H, F, seed, border)
    cot = _cot(s, F, seed)
    fo, saved = D.forward(s)
    want = D.backward_all(s, saved, *cot)
    hip.BINNING = binning
    fg, gg = _run_product(s, dev, seed, cot)
    # forward: every image and counter bit for bit
    for k in ("color", "language", "depth", "opacity", "opacity_lang", "radii", "radii_lang", "n_touched",
              "n_touched_lang"):
        assert torch.equal(fg[k], fo[k]), k
    if border:
        r1, r2 = fo["raw_radii"]
        assert int(((r1 < 0) & (r2 > 0)).sum()) > 0 and int(((r2 < 0) & (r1 > 0)).sum()) > 0, "the border case must occur"
        # ... and there the reported radius is the magnitude of the signed one
        m = (r1 < 0) & (r2 > 0)
        assert torch.equal(fg["radii"][m], -r1[m]) and bool((fg["radii"][m] > 0).all())
    # backward: DGR-D's gradients, the public module's against the two passes at the `_C` level ...
    import dgrd_product as DP
    passes = DP.run_passes(hip, s, cot, dev, binning=binning)
    g1, g2 = passes[0][1], passes[1][1]
    tau = g1["dL_dtau_sum"].reshape(6)
    same = dict(means3D=g1["dL_dmeans3D"], means2D=g1["dL_dmeans2D"], shs=g1["dL_dsh"], language=g2["dL_dlanguage"],
                opacities=g1["dL_dopacity"], opacities_lang=g2["dL_dopacity"], scales=g1["dL_dscales"],
                scales_lang=g2["dL_dscales"], rotations=g1["dL_drotations"], rotations_lang=g2["dL_drotations"],
                rho=tau[:3], theta=tau[3:])
    for k, v in same.items():
        assert gg[k] is not None, k
        d = first_difference(gg[k], v)
        assert d is None, f"{k}: the public module and the two passes differ in {d[3]} elements, first at {d[0]}: {d[1]!r} vs {d[2]!r}"
        assert bool((v != 0).any()), k
    # ... the passes' composite level: the ordered kernel EQUALS the restatement, the fast one differs by rounding only
    got = DP.dgrd_composite(DP.assert_fast_is_rounding_only(hip, s, passes, cot, f"P={P} seed={seed}"))
    for k, v in got.items():
        d = first_difference(v, want[k])
        assert d is None, f"ordered vs the restatement: {k}: {d[3]} elements differ, first at {d[0]}: {d[1]!r} vs {d[2]!r}"
    # ... and the per-Gaussian chain EQUALS the restatement's on the product's own composite-level gradients
    chain = D.backward_chain(s, saved, {k: v.cpu() for k, v in DP.dgrd_chain_inputs(passes).items()})
    for k, v in DP.dgrd_chain_outputs(passes).items():
        d = first_difference(v, chain[k])
        assert d is None, f"chain: {k}: {d[3]} elements differ, first at {d[0]}: {d[1]!r} vs {d[2]!r}"
    D.release(saved)


def test_language_loss_gives_no_mean_or_pose_gradient(hip):
    dev = torch.device(DEV)
    s = _scene2(2000, 160, 120, 3, 21)
    H, W = 120, 160
    zero3, zero1 = torch.zeros(3, H, W), torch.zeros(1, H, W)
    dl = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)) / (H * W)
    _f, g = _run_product(s, dev, 21, (zero3, dl, zero1))
    for k in ("means3D", "means2D", "theta", "rho", "scales", "rotations", "opacities", "shs"):
        assert float(g[k].abs().max()) == 0.0, k
    for k in ("language", "opacities_lang", "scales_lang", "rotations_lang"):
        assert float(g[k].abs().max()) > 0.0, k


def test_rgb_rasterizer_of_the_disentangled_package_uses_16_pixel_tiles(hip, oracle):
    from diff_gaussian_rasterization_disentangle import GaussianRasterizer
    from parity_common import run_backend
    dev = torch.device(DEV)
    sc = make_scene(3000, 160, 120, 0, seed=31, max_sh_degree=1)
    s = dict(camera=sc.camera, bg=sc.bg, sh_degree=sc.sh_degree)
    fo, _go = run_backend(oracle, sc, None, 3, 16, _abi.BWD_REFERENCE)
    rast = GaussianRasterizer(raster_settings=_settings(s, dev))
    m = sc.means3D.to(dev)
    color, radii, depth, opacity, n_touched = rast(
        means3D=m, means2D=torch.zeros_like(m), opacities=sc.opacities.to(dev), shs=sc.shs.to(dev),
        scales=sc.scales.to(dev), rotations=sc.rotations.to(dev))
    assert torch.equal(color.cpu(), fo["color"]) and torch.equal(n_touched.cpu(), fo["n_touched"])
    assert torch.equal(depth.cpu(), fo["depth"]) and torch.equal(radii.cpu(), fo["radii"])
    oracle.release(fo["geom"])
