"""The disentangled rasteriser's two passes at the `_C` level, as online_lang_splatting_amd/disentangled.py runs them, with
what a test needs besides the public outputs: each pass's state buffers and its composite-level gradients.  Shared by
tests/test_gpu_dgrd_ref_build.py and tests/test_gpu_disentangled.py.  A scene is the dict of tests/dgrd_scenes.py."""
import torch

from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import Scene
from parity_common import COMPOSITE_KEYS, assert_rounding_only, ordered_backward

TILE = 16
K_BOUND = 36.0  # the fast composite backward within K 2^-24 of each element's condition


def _dev(t, dev):
    return None if t is None else t.to(dev)


def pass_scenes(s):
    """(Scene, kw) of pass 1 and of pass 2, as parity_common.fwd_args / ordered_backward take them."""
    P, F = s["means3D"].shape[0], s["language"].shape[1]
    sm = s.get("scale_modifier", 1.0)
    none3 = torch.zeros(P, 3)
    sc1 = Scene(s["camera"], s["means3D"], s["opacities"], s.get("scales"), s.get("rotations"), s.get("shs"), None,
                s["sh_degree"], s["bg"], 0)
    kw1 = dict(colors_precomp=s.get("colors_precomp"), cov3D_precomp=s.get("cov3D_precomp"), scale_modifier=sm)
    sc2 = Scene(s["camera"], s["means3D"], s["opacities_lang"], s.get("scales_lang"), s.get("rotations_lang"), None,
                s["language"], 0, s["bg"], F)
    kw2 = dict(colors_precomp=none3, cov3D_precomp=s.get("cov3D_precomp_lang"), scale_modifier=sm)
    return (sc1, kw1), (sc2, kw2)


def run_passes(hip, s, cot, dev, binning=_abi.BINNING_RECT, mode=_abi.BWD_REFERENCE):
    """Both passes, forward and backward.  Returns per pass a forward dict (R, images, signed radii, n_touched, geom /
    binning / img buffers) and every gradient of _C.backward_all (dL_dconic, dL_ddepths and dL_dtau_sum included)."""
    from parity_common import fwd_args
    dc, dl, dd = (_dev(t, dev) for t in cot)
    cfg = (TILE, mode, binning)
    out = []
    for i, (sc, kw) in enumerate(pass_scenes(s)):
        F = sc.F
        a = fwd_args(sc, dev, **{k: _dev(v, dev) if torch.is_tensor(v) else v for k, v in kw.items()})
        if F == 0:
            a.insert(3, None)  # the language slot
        R, color, lang, radii, geom, binb, img, depth, opac, nt = hip._forward(
            F, *a, cfg=cfg, flags=_abi.FLAG_SIGNED_EMPTY_RADII)
        fwd = dict(R=R, color=color, language=lang, radii=radii, depth=depth, opacity=opac, n_touched=nt, geom=geom,
                   binning=binb, img=img)
        # backward arguments in the order of _C._backward
        bg, means3D, colors, language, _op, scales, rots, sm, cov, view, proj, proj_raw, tanx, tany, H, W, sh, deg, campos = a[:19]
        g_color = dc if i == 0 else torch.zeros_like(dc)
        g = hip.backward_all(F, bg, means3D, radii.clamp(min=0), colors, language, scales, rots, sm, cov, view, proj,
                             proj_raw, tanx, tany, g_color, dl if i == 1 else None, dd if i == 0 else None, sh, deg,
                             campos, geom, R, binb, img, False, cfg=cfg)
        out.append((fwd, g))
    torch.cuda.synchronize()
    return out


def pass_cotangents(cot, i):
    dc, dl, dd = cot
    return (dc, None, dd) if i == 0 else (torch.zeros_like(dc), dl, None)


def ordered_pass(hip, s, passes, cot, i, condition=False, mode=_abi.BWD_REFERENCE):
    """olsr_debug_backward_ordered on pass i's state with that pass's cotangents."""
    sc, kw = pass_scenes(s)[i]
    return ordered_backward(hip, sc, passes[i][0], 0, TILE, mode, cotangents=pass_cotangents(cot, i), condition=condition,
                            **kw)


def assert_fast_is_rounding_only(hip, s, passes, cot, where):
    """Row a9's criterion on both passes: every composite-level gradient of the fast kernel within K_BOUND 2^-24 of the
    element's condition, measured against the ordered kernel on the same state.  Returns the ordered runs."""
    ordered = []
    for i in (0, 1):
        if passes[i][0]["R"] == 0:
            # an empty list: the ordered instrument has nothing to run on, and every gradient is exactly zero
            g = {k: passes[i][1][k] for k in COMPOSITE_KEYS}
            assert all(not bool((v != 0).any()) for v in g.values()), f"{where}: pass {i + 1}: a gradient without an instance"
            ordered.append(g)
            continue
        gord = ordered_pass(hip, s, passes, cot, i)
        gcond = ordered_pass(hip, s, passes, cot, i, condition=True)
        assert_rounding_only(passes[i][1], gord, gcond, k_bound=K_BOUND, name=f"{where}: pass {i + 1}: ")
        ordered.append(gord)
    return ordered


def dgrd_composite(ordered):
    """The two ordered runs under DGR-D's names (oracle_ref_dgrd.COMPOSITE_KEYS)."""
    g1, g2 = ordered
    return dict(dL_dmeans2D=g1["dL_dmeans2D"], dL_dconic=g1["dL_dconic"], dL_dopacity=g1["dL_dopacity"],
                dL_dcolors=g1["dL_dcolors"], dL_ddepths=g1["dL_ddepths"], dL_dconic_lang=g2["dL_dconic"],
                dL_dopacity_lang=g2["dL_dopacity"], dL_dlanguage=g2["dL_dlanguage"])


def dgrd_chain_inputs(passes):
    g1, g2 = passes[0][1], passes[1][1]
    return dict(dL_dmeans2D=g1["dL_dmeans2D"], dL_dconic=g1["dL_dconic"], dL_dconic_lang=g2["dL_dconic"],
                dL_dcolors=g1["dL_dcolors"], dL_ddepths=g1["dL_ddepths"])


def dgrd_chain_outputs(passes):
    """The product's per-Gaussian gradients under DGR-D's names (oracle_ref_dgrd.CHAIN_KEYS): set 1's from pass 1, of pass
    2 only the covariance, scale and rotation gradients (its mean and pose gradients do not exist in DGR-D)."""
    g1, g2 = passes[0][1], passes[1][1]
    return dict(dL_dmeans3D=g1["dL_dmeans3D"], dL_dcov3D=g1["dL_dcov3D"], dL_dsh=g1["dL_dsh"], dL_dscales=g1["dL_dscales"],
                dL_drotations=g1["dL_drotations"], dL_dtau=g1["dL_dtau"], dL_dcov3D_lang=g2["dL_dcov3D"],
                dL_dscales_lang=g2["dL_dscales"], dL_drotations_lang=g2["dL_drotations"])


__all__ = ["COMPOSITE_KEYS"]
