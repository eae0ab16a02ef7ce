"""The disentangled reference rasteriser's own kernels (DGR-D), run on the host.  TEST INFRASTRUCTURE ONLY.

Loads oracle/_ref/libref_dgrd_t16_f{F}.so (oracle/ref_build.py: DGR-D's cuda_rasterizer sources compiled as host C++ over
the execution model of oracle/ref_shim/, driven through DGR-D's LanguageRasterizer entry points by
oracle/ref_entry_dgrd.cpp).  Only tests/ may import it.

A scene is the dict tests/dgrd_scenes.py builds: camera, bg, means3D, sh_degree, language, shs or colors_precomp, and per
set opacities, scales + rotations or cov3D_precomp (second set: the same names with the suffix _lang); scale_modifier is
optional.  The language channel count of the scene selects the build (3 or 15).
"""
import ctypes as C
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
from online_lang_splatting_amd import _abi  # noqa: E402  (struct declarations only)
from oracle import ref_build  # noqa: E402

TILE = 16
FAM = ref_build.DGRD

COMPOSITE_KEYS = ("dL_dmeans2D", "dL_dconic", "dL_dconic_lang", "dL_dopacity", "dL_dopacity_lang", "dL_dcolors",
                  "dL_dlanguage", "dL_ddepths")
CHAIN_KEYS = ("dL_dmeans3D", "dL_dcov3D", "dL_dcov3D_lang", "dL_dsh", "dL_dscales", "dL_dscales_lang", "dL_drotations",
              "dL_drotations_lang", "dL_dtau")
STATE_FIELDS = ("means2D", "depths", "cov3D", "cov3D_lang", "conic_opacity", "conic_opacity_lang", "rgb", "clamped",
                "tiles_touched", "tiles_touched_lang", "point_list", "point_list_lang", "ranges", "ranges_lang",
                "n_contrib", "n_contrib_lang", "final_T", "final_T_lang")
_INT_FIELDS = {"clamped": torch.uint8, "keys": torch.int64, "keys_lang": torch.int64}
_INT32 = ("tiles_touched", "point_offsets", "point_list", "ranges", "n_contrib")

_libs = {}


def available(F=None):
    """Is there a DGR-D build for F language channels - or, without an argument, any - or the tree to make one from?"""
    have = FAM.builds if ref_build.have_reference(FAM) else ref_build.existing_builds(FAM)
    return bool(have) if F is None else (TILE, F) in have


def lib(F):
    if F not in _libs:
        so = ref_build.lib_path(TILE, F, fam=FAM)
        if ref_build.have_reference(FAM) and (TILE, F) in FAM.builds:
            so = ref_build.build_one(TILE, F, fam=FAM)
        if not os.path.exists(so):
            raise RuntimeError(f"no DGR-D build for {F} language channels ({so}); python oracle/ref_build.py makes it "
                               "where the reference tree is present")
        L = C.CDLL(so)
        vp, sp = C.c_void_p, C.POINTER(_abi.OlsrScene)
        L.refd_create.restype = vp
        L.refd_destroy.argtypes = [vp]
        L.refd_forward.argtypes = [vp, sp, sp] + [vp] * 11
        L.refd_backward.argtypes = [vp, sp, sp] + [vp] * 22
        L.refd_backward_chain.argtypes = [vp, sp, sp] + [vp] * 16
        for f in (L.refd_forward, L.refd_backward, L.refd_backward_chain):
            f.restype = C.c_int
        L.refd_get_field.argtypes = [vp, C.c_char_p, vp]
        L.refd_get_field.restype = C.c_int64
        assert L.refd_tile() == TILE and L.refd_language_channels() == F, (so, L.refd_tile(), L.refd_language_channels())
        _libs[F] = L
    return _libs[F]


class _State:
    def __init__(self, L):
        self.L = L
        self.h = L.refd_create()

    def __del__(self):
        try:
            self.L.refd_destroy(self.h)
        except Exception:
            pass


def _f(t):
    return t.detach().cpu().contiguous().float() if t is not None and t.numel() > 0 else None


def _scenes(a, opacities=True):
    """(olsr_scene of set 1 with everything shared, olsr_scene of set 2, the tensors both point into)."""
    cam = a["camera"]
    P = a["means3D"].shape[0]
    F = a["language"].shape[1]
    shared = [_f(x) for x in (a["bg"], a["means3D"], a["language"], cam.world_view_transform, cam.full_proj_transform,
                              cam.projection_matrix, cam.camera_center)]
    bg, m, lang, v, p, pr, cp = shared
    keep = list(shared)
    out = []
    for sfx in ("", "_lang"):
        sh = _f(a.get("shs")) if not sfx and a.get("colors_precomp") is None else None
        col = _f(a.get("colors_precomp")) if not sfx else None
        if sfx:
            col = torch.zeros(P, 3)  # (never read: the second struct carries the second set's four arrays only)
        op = _f(a["opacities" + sfx]) if opacities else torch.zeros(max(P, 1))
        cov = _f(a.get("cov3D_precomp" + sfx))
        sc = _f(a.get("scales" + sfx)) if cov is None else None
        rot = _f(a.get("rotations" + sfx)) if cov is None else None
        keep += [sh, col, op, cov, sc, rot]
        out.append(_abi.make_scene(
            P=P, D=a["sh_degree"], M=sh.shape[1] if sh is not None else 0, F=F, width=cam.width, height=cam.height,
            tile=TILE, prefiltered=False, debug=False, bwd_mode=_abi.BWD_REFERENCE, tan_fovx=cam.tanfovx,
            tan_fovy=cam.tanfovy, scale_modifier=a.get("scale_modifier", 1.0), flags=0, background=bg, means3D=m, shs=sh,
            colors_precomp=col, language_precomp=lang, opacities=op, scales=sc, rotations=rot, cov3D_precomp=cov,
            viewmatrix=v, projmatrix=p, projmatrix_raw=pr, cam_pos=cp))
    return out[0], out[1], keep


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"DGR-D build: {what} failed with code {rc}")


def forward(a):
    """Every output of DGR-D's forward as a dict, R and R_lang, and "state": the handle of the saved buffers."""
    cam = a["camera"]
    P, F, H, W = a["means3D"].shape[0], a["language"].shape[1], cam.height, cam.width
    s1, s2, keep = _scenes(a)
    o = dict(color=torch.zeros(3, H, W), language=torch.zeros(F, H, W), depth=torch.zeros(1, H, W),
             opacity=torch.zeros(1, H, W), opacity_lang=torch.zeros(1, H, W))
    o.update({k: torch.zeros(P, dtype=torch.int32) for k in ("radii", "radii_lang", "n_touched", "n_touched_lang")})
    R, R_lang = C.c_int32(0), C.c_int32(0)
    st = _State(lib(F))
    _check(st.L.refd_forward(st.h, C.byref(s1), C.byref(s2), *(o[k].data_ptr() for k in (
        "color", "language", "depth", "opacity", "opacity_lang", "radii", "radii_lang", "n_touched", "n_touched_lang")),
        C.addressof(R), C.addressof(R_lang)), "forward")
    o.update(R=R.value, R_lang=R_lang.value, state=st)
    return o


def get_field(fwd, name):
    st = fwd["state"]
    n = st.L.refd_get_field(st.h, name.encode(), None)
    if n < 0:
        raise KeyError(name)
    dt = _INT_FIELDS.get(name, torch.int32 if name.replace("_lang", "") in _INT32 else torch.float32)
    t = torch.zeros(n, dtype=dt)
    st.L.refd_get_field(st.h, name.encode(), t.data_ptr())
    return t


def _grads(a, keys):
    P, F = a["means3D"].shape[0], a["language"].shape[1]
    M = a["shs"].shape[1] if a.get("colors_precomp") is None else 0
    w = dict(dL_dmeans2D=(P, 3), dL_dconic=(P, 2, 2), dL_dconic_lang=(P, 2, 2), dL_dopacity=(P, 1),
             dL_dopacity_lang=(P, 1), dL_dcolors=(P, 3), dL_dlanguage=(P, F), dL_ddepths=(P, 1), dL_dmeans3D=(P, 3),
             dL_dcov3D=(P, 6), dL_dcov3D_lang=(P, 6), dL_dsh=(P, M, 3), dL_dscales=(P, 3), dL_dscales_lang=(P, 3),
             dL_drotations=(P, 4), dL_drotations_lang=(P, 4), dL_dtau=(P, 6))
    return {k: torch.zeros(*w[k]) for k in keys}


def _radii(fwd):
    return fwd["radii"].contiguous().to(torch.int32), fwd["radii_lang"].contiguous().to(torch.int32)


def backward_all(a, fwd, dL_dcolor, dL_dlanguage, dL_ddepth):
    """Every gradient of DGR-D's backward (COMPOSITE_KEYS + CHAIN_KEYS); dL_ddepth may be None."""
    st = fwd["state"]
    s1, s2, keep = _scenes(a, opacities=False)  # (opacities are no input of DGR-D's backward)
    g = _grads(a, COMPOSITE_KEYS + CHAIN_KEYS)
    r, rl = _radii(fwd)
    dc, dl, dd = _f(dL_dcolor), _f(dL_dlanguage), _f(dL_ddepth)
    _check(st.L.refd_backward(st.h, C.byref(s1), C.byref(s2), r.data_ptr(), rl.data_ptr(), dc.data_ptr(), dl.data_ptr(),
                              dd.data_ptr() if dd is not None else None,
                              *(g[k].data_ptr() for k in COMPOSITE_KEYS + CHAIN_KEYS)), "backward")
    return g


def backward_chain(a, fwd, composite):
    """DGR-D's computeCov2DCUDA, computeCov2DCUDA_no_tau and language_preprocessCUDA alone, on caller-provided
    composite-level gradients: dict with dL_dmeans2D [P,3], dL_dconic and dL_dconic_lang [P,2,2], dL_dcolors [P,3],
    dL_ddepths [P,1]."""
    st = fwd["state"]
    P = a["means3D"].shape[0]
    s1, s2, keep = _scenes(a, opacities=False)
    g = _grads(a, CHAIN_KEYS)
    r, rl = _radii(fwd)
    names = ("dL_dmeans2D", "dL_dconic", "dL_dconic_lang", "dL_dcolors", "dL_ddepths")
    cin = {k: composite[k].detach().cpu().contiguous().float() for k in names}
    for k, w in zip(names, (3, 4, 4, 3, 1)):
        assert cin[k].numel() == w * P, k
    _check(st.L.refd_backward_chain(st.h, C.byref(s1), C.byref(s2), r.data_ptr(), rl.data_ptr(),
                                    *(cin[k].data_ptr() for k in names), *(g[k].data_ptr() for k in CHAIN_KEYS)),
           "backward_chain")
    return g


def release(fwd):
    fwd.pop("state", None)
