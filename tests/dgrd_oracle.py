"""CPU oracle of the disentangled rasterizer DGR-D (submodules/diff-gaussian-rasterization-disentangle-optim) — TEST
INFRASTRUCTURE, written independently of online_lang_splatting_amd/disentangled.py.

It restates DGR-D by what its kernels do, on top of the oracle of the plain rasterizer (oracle/oracle_C.py, which
restates DGR = submodules/diff-gaussian-rasterization): two passes of that oracle with DGR-D's 16x16 tiles
(DGR-D/cuda_rasterizer/config.h:17-18) plus a radius rule.  tests/test_dgrd_ref_build_cpu.py holds every statement below
to DGR-D's own kernel source, compiled as host C++ (oracle/ref_build.py, oracle/oracle_ref_dgrd.py), on the scenes of
tests/dgrd_scenes.py: outputs, saved state and gradients are compared as equalities.

A scene is a dict of CPU tensors: camera, bg, means3D, sh_degree, language, shs or colors_precomp, and per set
opacities, scales + rotations or cov3D_precomp (second set: the same names with the suffix _lang); scale_modifier is
optional.
"""
import torch

from oracle import oracle_C
from online_lang_splatting_amd import _abi

TILE = 16
E = torch.empty(0)


def _with(O, tile, mode, flags):
    O.TILE, O.BWD_MODE, O.FLAGS = tile, mode, flags


def _opt(a, k):
    return a[k] if a.get(k) is not None else E


def _set(a, sfx):
    """(scales, rotations, scale_modifier, cov3D_precomp) of one set as the oracle's positional arguments."""
    cov = _opt(a, "cov3D_precomp" + sfx)
    pre = cov.numel() > 0
    return (E if pre else a["scales" + sfx], E if pre else a["rotations" + sfx], a.get("scale_modifier", 1.0), cov)


def _zero_det(O, geom, radii):
    """Per Gaussian: did this pass go on with a zero determinant?  Its conic is then what 1 / 0 gives: conic.x = c * inf
    with c >= 0.3.  (Read where the pass wrote a conic: the squares that cover a tile.  A zero determinant needs a
    footprint thousands of pixels long, whose square covers every tile.)"""
    cx = O.get_field(geom, "conic_opacity").view(-1, 4)[:, 0]
    return (radii > 0) & ~torch.isfinite(cx)


def forward(sc2, mode=_abi.BWD_REFERENCE, O=oracle_C):
    """sc2: dict with the DGR-D inputs (CPU tensors).  Returns (outputs dict, saved state).  O: the instance of
    oracle/oracle_C.py to run on (tests bind private ones to a variant library).

    The zero determinant (DGR-D forward.cu:356-366): the plain rasteriser drops a Gaussian whose float32 2D covariance has
    det == 0; DGR-D drops it only when BOTH sets' determinants are zero, and otherwise lets the zero set go on with an
    infinite conic.  So both passes run with OLSR_FLAG_ORACLE_KEEP_ZERO_DET, and a Gaussian that came out with a zero
    determinant in both is taken out (moved onto the camera centre, where the frustum test culls it as DGR-D's early return
    does: nothing written, radii 0) and the passes are run again."""
    out, saved = _forward(sc2, sc2["means3D"], mode, O)
    both = _zero_det(O, saved["geom1"], saved["r1"]) & _zero_det(O, saved["geom2"], saved["r2"])
    if bool(both.any()):
        release(saved)
        means = sc2["means3D"].clone()
        means[both] = sc2["camera"].camera_center.to(means.dtype)
        out, saved = _forward(sc2, means, mode, O)
    return out, saved


def _forward(sc2, means3D, mode, O):
    a = dict(sc2, means3D=means3D)
    cam = a["camera"]
    common = (cam.world_view_transform, cam.full_proj_transform, cam.projection_matrix, cam.tanfovx, cam.tanfovy,
              cam.height, cam.width)
    col = _opt(a, "colors_precomp")
    shs = E if col.numel() else a["shs"]
    _with(O, TILE, mode, _abi.FLAG_SIGNED_EMPTY_RADII | _abi.FLAG_ORACLE_KEEP_ZERO_DET)
    try:
        # colour + depth loop of language_renderCUDA (DGR-D forward.cu:506-560): lists, conics and opacities of set 1
        R1, color, r1, geom1, bin1, img1, depth, opacity, n_touched = O.rasterize_gaussians(
            a["bg"], a["means3D"], col, a["opacities"], *_set(a, ""), *common, shs, a["sh_degree"], cam.camera_center,
            False, False)
        # language loop (DGR-D forward.cu:562-633): lists, conics and opacities of set 2; colours play no role in it
        zeros = torch.zeros(a["means3D"].shape[0], 3)
        R2, _c, language, r2, geom2, bin2, img2, _d, opacity_lang, n_touched_lang = O.rasterize_language_gaussians(
            a["bg"], a["means3D"], zeros, a["language"], a["opacities_lang"], *_set(a, "_lang"), *common, E, 0,
            cam.camera_center, False, False)
    finally:
        _with(O, 15, _abi.BWD_REFERENCE, 0)
    # languagePreprocessCUDA returns early only when BOTH squares cover no tile (DGR-D forward.cu:391-397) and then
    # writes radii[idx] = my_radius, radii_lang[idx] = my_radius_lang unconditionally (:421-431)
    vis = (r1 > 0) | (r2 > 0)
    radii = torch.where(vis, r1.abs(), torch.zeros_like(r1))
    radii_lang = torch.where(vis, r2.abs(), torch.zeros_like(r2))
    out = dict(color=color, language=language, radii=radii, radii_lang=radii_lang, depth=depth, opacity=opacity,
               opacity_lang=opacity_lang, n_touched=n_touched, n_touched_lang=n_touched_lang, R1=R1, R2=R2,
               raw_radii=(r1, r2))
    saved = dict(common=common[:5], geom1=geom1, bin1=bin1, img1=img1, geom2=geom2, bin2=bin2, img2=img2, R1=R1, R2=R2,
                 r1=r1.clamp(min=0), r2=r2.clamp(min=0), zeros=zeros, col=col, shs=shs, O=O, means3D=means3D)
    return out, saved


def state(saved):
    """The saved state under DGR-D's names (oracle_ref_dgrd.STATE_FIELDS): set 1's from pass 1, set 2's (_lang) from pass 2;
    means2D and depths are computed alike by both passes and taken from pass 1 where it is visible, else from pass 2."""
    O = saved["O"]
    g1 = lambda k: O.get_field(saved["geom1"], k)  # noqa: E731
    g2 = lambda k: O.get_field(saved["geom2"], k)  # noqa: E731
    st = {k: g1(k) for k in ("cov3D", "conic_opacity", "rgb", "clamped", "tiles_touched", "point_list", "ranges",
                             "n_contrib", "final_T")}
    st.update({k + "_lang": g2(k) for k in ("cov3D", "conic_opacity", "tiles_touched", "point_list", "ranges",
                                            "n_contrib", "final_T")})
    v1 = saved["r1"] > 0
    st["means2D"] = torch.where(v1[:, None], g1("means2D").view(-1, 2), g2("means2D").view(-1, 2)).reshape(-1)
    st["depths"] = torch.where(v1, g1("depths"), g2("depths"))
    return st


def _args1(a, s, dc, dd):
    cam = a["camera"]
    return (0, a["bg"], s["means3D"], s["r1"], s["col"], None, *_set(a, ""), *s["common"], dc, None, dd, s["shs"],
            a["sh_degree"], cam.camera_center, s["geom1"], s["R1"], s["bin1"], s["img1"], False)


def _args2(a, s, dc, dl, dd):
    cam = a["camera"]
    return (a["language"].shape[1], a["bg"], s["means3D"], s["r2"], s["zeros"], a["language"], *_set(a, "_lang"),
            *s["common"], torch.zeros_like(dc), dl, torch.zeros_like(dd), E, 0, cam.camera_center, s["geom2"], s["R2"],
            s["bin2"], s["img2"], False)


_FROM_1 = ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dtau")
_FROM_2 = dict(dL_dcov3D_lang="dL_dcov3D", dL_dscales_lang="dL_dscales", dL_drotations_lang="dL_drotations")


def backward_all(sc2, saved, dc, dl, dd, mode=_abi.BWD_REFERENCE):
    """Every gradient of DGR-D's backward under the names of oracle_ref_dgrd (COMPOSITE_KEYS + CHAIN_KEYS); dd may be
    None (the binding passes zeros then)."""
    a, s = sc2, saved
    O = s["O"]
    if dd is None:
        dd = torch.zeros(1, a["camera"].height, a["camera"].width)
    _with(O, TILE, mode, 0)
    try:
        # colour loop of language_render_cuda (DGR-D backward.cu:1218-1335) + computeCov2DCUDA + the first-set half of
        # language_preprocessCUDA (:1545-1564, :676-808): the RGB rasterizer's backward
        g1 = O.backward_all(*_args1(a, s, dc, dd))
        # language loop (:1337-1428): dL_dalpha_lang has only the feature term (no colour, depth or background term),
        # the recursion is not skip-guarded (:1385-1393), thread 0's feature gradient is the one added (:1423-1425), no
        # mean gradient is formed; computeCov2DCUDA_no_tau (:354-436) then yields dL_dcov3D_lang only, from which
        # language_preprocessCUDA derives scale_lang / rotation_lang.  With zero colour / depth cotangents the language
        # rasterizer's backward computes exactly these terms (its colour terms multiply the zero cotangents).
        g2 = O.backward_all(*_args2(a, s, dc, dl, dd))
    finally:
        _with(O, 15, _abi.BWD_REFERENCE, 0)
    g = {k: g1[k] for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_ddepths") + _FROM_1}
    g.update(dL_dconic_lang=g2["dL_dconic"], dL_dopacity_lang=g2["dL_dopacity"], dL_dlanguage=g2["dL_dlanguage"])
    g.update({k: g2[v] for k, v in _FROM_2.items()})
    return g


def backward_chain(sc2, saved, comp):
    """The per-Gaussian half alone (DGR-D's computeCov2DCUDA, computeCov2DCUDA_no_tau, language_preprocessCUDA) on
    caller-provided composite-level gradients: dict with dL_dmeans2D [P,3], dL_dconic and dL_dconic_lang [P,2,2],
    dL_dcolors [P,3], dL_ddepths [P,1].  The second set sees its conic gradient and nothing else."""
    a, s = sc2, saved
    O = s["O"]
    P, H, W = a["means3D"].shape[0], a["camera"].height, a["camera"].width
    dc, dl, dd = torch.zeros(3, H, W), torch.zeros(a["language"].shape[1], H, W), torch.zeros(1, H, W)
    c1 = {k: comp[k] for k in ("dL_dmeans2D", "dL_dconic", "dL_dcolors", "dL_ddepths")}
    c2 = dict(dL_dmeans2D=torch.zeros(P, 3), dL_dconic=comp["dL_dconic_lang"], dL_dcolors=torch.zeros(P, 3),
              dL_ddepths=torch.zeros(P, 1))
    _with(O, TILE, _abi.BWD_REFERENCE, 0)
    try:
        a1, a2 = _args1(a, s, dc, dd), _args2(a, s, dc, dl, dd)
        g1 = O.backward_chain(a1[0], c1, *a1[1:])
        g2 = O.backward_chain(a2[0], c2, *a2[1:])
    finally:
        _with(O, 15, _abi.BWD_REFERENCE, 0)
    g = {k: g1[k] for k in _FROM_1}
    g.update({k: g2[v] for k, v in _FROM_2.items()})
    return g


def backward(sc2, saved, dc, dl, dd, mode=_abi.BWD_REFERENCE):
    """DGR-D's gradients (names of DGR-D __init__.py:389-404)."""
    g = backward_all(sc2, saved, dc, dl, dd, mode)
    tau = g["dL_dtau"].view(-1, 6).sum(0)  # DGR-D __init__.py:405-407
    return dict(means2D=g["dL_dmeans2D"], colors=g["dL_dcolors"], language=g["dL_dlanguage"], opacities=g["dL_dopacity"],
                opacities_lang=g["dL_dopacity_lang"], means3D=g["dL_dmeans3D"], cov3D=g["dL_dcov3D"],
                cov3D_lang=g["dL_dcov3D_lang"], sh=g["dL_dsh"], scales=g["dL_dscales"], scales_lang=g["dL_dscales_lang"],
                rotations=g["dL_drotations"], rotations_lang=g["dL_drotations_lang"], rho=tau[:3], theta=tau[3:])


def release(saved):
    saved["O"].release(saved["geom1"])
    saved["O"].release(saved["geom2"])
