"""The reference rasteriser's own kernels, run on the host, with the surface of oracle/oracle_C.py.  TEST INFRASTRUCTURE ONLY.

Loads oracle/_ref/libref_t{TILE}_f{F}.so (oracle/ref_build.py: the reference's cuda_rasterizer sources compiled as host
C++ over the execution model of oracle/ref_shim/, driven through the reference's Rasterizer / LanguageRasterizer entry
points by oracle/ref_entry.cpp).  Same functions and positional signatures as oracle_C, so tests/parity_common.run_backend
takes this module as a backend unchanged.  Only tests/ may import it.

TILE selects the build (15 or 16); the language channel count of the call selects it too (15, 3 or 16; calls without
language run through the RGB entry points of the 15-channel build of that tile).  BWD_MODE and BINNING are accepted and
ignored: the reference has one backward and one binning.
"""
import ctypes as C
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
from online_lang_splatting_amd import _abi  # noqa: E402  (struct declarations only)
from oracle import ref_build  # noqa: E402

TILE = 15
BWD_MODE = _abi.BWD_REFERENCE
BINNING = 0
LIBM_EXP = False  # the -DREF_LIBM_EXP build (built on demand; mirrors oracle_C's "libm_exp" variant)

_libs = {}
_states = {}
_next_id = [1]

CHAIN_KEYS = ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dtau")


def available(tile=None, F=None):
    """Is there a build for (tile, F channels) - or, without arguments, any build at all - or the tree to make one from?"""
    if ref_build.have_reference():
        return tile is None or (tile, 15 if not F else F) in ref_build.BUILDS
    have = ref_build.existing_builds()
    return bool(have) if tile is None else (tile, 15 if not F else F) in have


def lib(F):
    """The build for the current TILE and F language channels (F == 0: the 15-channel build's RGB entry points)."""
    key = (TILE, 15 if F <= 0 else F, LIBM_EXP)
    if key not in _libs:
        tile, f, libm = key
        so = ref_build.lib_path(tile, f, libm)
        if ref_build.have_reference() and (tile, f) in ref_build.BUILDS:
            so = ref_build.build_one(tile, f, libm)
        if not os.path.exists(so):
            raise RuntimeError(f"no reference build for tile {tile}, {f} language channels ({so}); "
                               "python oracle/ref_build.py makes it where the reference tree is present")
        L = C.CDLL(so)
        vp = C.c_void_p
        L.ref_create.restype = vp
        L.ref_destroy.argtypes = [vp]
        L.ref_variant.restype = C.c_char_p
        L.ref_forward.argtypes = [vp, C.POINTER(_abi.OlsrScene)] + [vp] * 7
        L.ref_forward.restype = C.c_int
        L.ref_backward.argtypes = [vp, C.POINTER(_abi.OlsrScene)] + [vp] * 16
        L.ref_backward.restype = C.c_int
        L.ref_backward_chain.argtypes = [vp, C.POINTER(_abi.OlsrScene)] + [vp] * 11
        L.ref_backward_chain.restype = C.c_int
        L.ref_mark_visible.argtypes = [C.c_int32, vp, vp, vp, vp]
        L.ref_mark_visible.restype = C.c_int
        L.ref_get_field.argtypes = [vp, C.c_char_p, vp]
        L.ref_get_field.restype = C.c_int64
        assert L.ref_tile() == tile and L.ref_language_channels() == f, (so, L.ref_tile(), L.ref_language_channels())
        _libs[key] = L
    return _libs[key]


class _State:
    def __init__(self, L):
        self.L = L
        self.h = L.ref_create()

    def __del__(self):
        try:
            self.L.ref_destroy(self.h)
        except Exception:
            pass


def _f(t):
    return t.detach().cpu().contiguous().float() if t is not None and t.numel() > 0 else None


def _scene(bg, means3D, colors, language, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
           projmatrix, projmatrix_raw, tan_fovx, tan_fovy, H, W, sh, degree, campos, prefiltered, debug, F):
    keep = [_f(x) for x in (bg, means3D, sh, colors, language, opacity, scales, rotations, cov3D_precomp,
                            viewmatrix, projmatrix, projmatrix_raw, campos)]
    bg_, m_, sh_, col_, lang_, op_, sc_, rot_, cov_, v_, p_, pr_, cp_ = keep
    M = sh_.shape[1] if sh_ is not None else 0
    s = _abi.make_scene(P=means3D.shape[0], D=degree, M=M, F=F, width=W, height=H, tile=TILE,
                        prefiltered=prefiltered, debug=debug, bwd_mode=_abi.BWD_REFERENCE, tan_fovx=tan_fovx,
                        tan_fovy=tan_fovy, scale_modifier=scale_modifier, flags=0, background=bg_, means3D=m_, shs=sh_,
                        colors_precomp=col_, language_precomp=lang_, opacities=op_, scales=sc_, rotations=rot_,
                        cov3D_precomp=cov_, viewmatrix=v_, projmatrix=p_, projmatrix_raw=pr_, cam_pos=cp_)
    return s, keep


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"reference build: {what} failed with code {rc}")


def _forward(F, bg, means3D, colors, language, opacity, scales, rotations, scale_modifier, cov3D_precomp,
             viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, H, W, sh, degree, campos, prefiltered, debug):
    P = means3D.shape[0]
    s, keep = _scene(bg, means3D, colors, language, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                     viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, H, W, sh, degree, campos,
                     prefiltered, debug, F)
    out_color = torch.zeros(3, H, W)
    out_lang = torch.zeros(max(F, 0), H, W)
    out_depth = torch.zeros(1, H, W)
    out_opacity = torch.zeros(1, H, W)
    radii = torch.zeros(P, dtype=torch.int32)
    n_touched = torch.zeros(P, dtype=torch.int32)
    R = C.c_int32(0)
    L = lib(F)
    st = _State(L)
    sid = _next_id[0]
    _next_id[0] += 1
    _states[sid] = st
    _check(L.ref_forward(st.h, C.byref(s), out_color.data_ptr(), out_lang.data_ptr(), out_depth.data_ptr(),
                         out_opacity.data_ptr(), radii.data_ptr(), n_touched.data_ptr(), C.addressof(R)), "forward")
    geom = torch.tensor([sid], dtype=torch.int64).view(torch.uint8)
    empty = torch.empty(0, dtype=torch.uint8)
    return R.value, out_color, out_lang, radii, geom, empty, empty.clone(), out_depth, out_opacity, n_touched


def state_of(geomBuffer):
    return _states[int(geomBuffer.view(torch.int64)[0])]


def release(geomBuffer):
    _states.pop(int(geomBuffer.view(torch.int64)[0]), None)


_FIELD_DT = {"clamped": torch.uint8, "tiles_touched": torch.int32, "point_offsets": torch.int32,
             "point_list": torch.int32, "keys": torch.int64, "ranges": torch.int32, "n_contrib": torch.int32}


def get_field(geomBuffer, name):
    st = state_of(geomBuffer)
    n = st.L.ref_get_field(st.h, name.encode(), None)
    if n < 0:
        raise KeyError(name)
    t = torch.zeros(n, dtype=_FIELD_DT.get(name, torch.float32))
    st.L.ref_get_field(st.h, name.encode(), t.data_ptr())
    return t


def rasterize_gaussians(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        projmatrix, projmatrix_raw, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                        campos, prefiltered, debug):
    r = _forward(0, bg, means3D, colors, None, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                 viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                 campos, prefiltered, debug)
    R, color, _lang, radii, geom, binning, img, depth, opacity_out, n_touched = r
    return R, color, radii, geom, binning, img, depth, opacity_out, n_touched


def rasterize_language_gaussians(bg, means3D, colors, language, opacity, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy,
                                 image_height, image_width, sh, degree, campos, prefiltered, debug):
    return _forward(language.shape[1], bg, means3D, colors, language, opacity, scales, rotations, scale_modifier,
                    cov3D_precomp, viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, image_height,
                    image_width, sh, degree, campos, prefiltered, debug)


def _backward(F, bg, means3D, radii, colors, language, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
              projmatrix, projmatrix_raw, tan_fovx, tan_fovy, dL_dout_color, dL_dout_language, dL_dout_depth, sh,
              degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, composite=None):
    P = means3D.shape[0]
    H, W = dL_dout_color.shape[1], dL_dout_color.shape[2]
    st = state_of(geomBuffer)
    dummy_op = torch.zeros(max(P, 1))  # (opacities are no input of the reference's backward)
    s, keep = _scene(bg, means3D, colors, language, dummy_op, scales, rotations, scale_modifier, cov3D_precomp,
                     viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, H, W, sh, degree, campos, False,
                     debug, F)
    M = s.M
    g = dict(
        dL_dmeans2D=torch.zeros(P, 3), dL_dconic=torch.zeros(P, 2, 2), dL_dopacity=torch.zeros(P, 1),
        dL_dcolors=torch.zeros(P, 3), dL_dlanguage=torch.zeros(P, max(F, 0)), dL_ddepths=torch.zeros(P, 1),
        dL_dmeans3D=torch.zeros(P, 3), dL_dcov3D=torch.zeros(P, 6), dL_dsh=torch.zeros(P, M, 3),
        dL_dscales=torch.zeros(P, 3), dL_drotations=torch.zeros(P, 4), dL_dtau=torch.zeros(P, 6))
    rad = radii.detach().cpu().contiguous().to(torch.int32)
    if composite is not None:
        cin = {k: composite[k].detach().cpu().contiguous().float() for k in
               ("dL_dmeans2D", "dL_dconic", "dL_dcolors", "dL_ddepths")}
        assert cin["dL_dmeans2D"].numel() == 3 * P and cin["dL_dconic"].numel() == 4 * P
        assert cin["dL_dcolors"].numel() == 3 * P and cin["dL_ddepths"].numel() == P
        _check(st.L.ref_backward_chain(
            st.h, C.byref(s), rad.data_ptr(), cin["dL_dmeans2D"].data_ptr(), cin["dL_dconic"].data_ptr(),
            cin["dL_dcolors"].data_ptr(), cin["dL_ddepths"].data_ptr(), g["dL_dmeans3D"].data_ptr(),
            g["dL_dcov3D"].data_ptr(), g["dL_dsh"].data_ptr(), g["dL_dscales"].data_ptr(),
            g["dL_drotations"].data_ptr(), g["dL_dtau"].data_ptr()), "backward_chain")
        return {k: g[k] for k in CHAIN_KEYS}
    dc = _f(dL_dout_color)
    dl = _f(dL_dout_language) if F > 0 else torch.zeros(1)
    dd = _f(dL_dout_depth)
    _check(st.L.ref_backward(
        st.h, C.byref(s), rad.data_ptr(), dc.data_ptr(), dl.data_ptr(), dd.data_ptr(),
        g["dL_dmeans2D"].data_ptr(), g["dL_dconic"].data_ptr(), g["dL_dopacity"].data_ptr(),
        g["dL_dcolors"].data_ptr(), g["dL_dlanguage"].data_ptr(), g["dL_ddepths"].data_ptr(),
        g["dL_dmeans3D"].data_ptr(), g["dL_dcov3D"].data_ptr(), g["dL_dsh"].data_ptr(),
        g["dL_dscales"].data_ptr(), g["dL_drotations"].data_ptr(), g["dL_dtau"].data_ptr()), "backward")
    return g


def backward_chain(F, composite, *args, **kw):
    """The reference's computeCov2DCUDA and backward preprocessCUDA alone, on caller-provided composite-level gradients
    (dict with dL_dmeans2D [P,3], dL_dconic [P,2,2], dL_dcolors [P,3], dL_ddepths [P,1]); args as backward_all."""
    return _backward(F, *args, composite=composite, **kw)


def backward_all(F, *args, **kw):
    """Every gradient of the reference's backward, dL_dconic and dL_ddepths included; args as oracle_C.backward_all."""
    return _backward(F, *args, **kw)


def mark_visible(means3D, viewmatrix, projmatrix):
    P = means3D.shape[0]
    present = torch.zeros(P, dtype=torch.bool)
    m, v, p = _f(means3D), _f(viewmatrix), _f(projmatrix)
    if P:
        _check(lib(0).ref_mark_visible(P, m.data_ptr(), v.data_ptr(), p.data_ptr(), present.data_ptr()), "mark_visible")
    return present
