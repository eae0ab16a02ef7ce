"""TSDF fusion, the part that needs no GPU: the ctypes mirrors match include/olsr.h, the C-ABI entries refuse bad arguments
before any HIP call, and the Python class refuses a CPU device (there is no fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000   # a made-up address: every call below returns before anything could follow it


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import build
    build.build()
    from online_lang_splatting_amd import _lib
    return _lib.lib()


def test_struct_layout_and_constants_match_the_header():
    from online_lang_splatting_amd import _abi
    assert C.sizeof(_abi.OlsrTsdfView) == 128 and _abi.OlsrTsdfView.depth.offset == 104 and _abi.OlsrTsdfView.H.offset == 88
    assert C.sizeof(_abi.OlsrTsdfVolume) == 64 and _abi.OlsrTsdfVolume.tsdf.offset == 40
    src = open(os.path.join(ROOT, "include", "olsr.h")).read()
    defs = dict(re.findall(r"#define (OLSR_TSDF_[A-Z_]+) (\d+)", src))
    assert int(defs["OLSR_TSDF_MAX_VIEWS"]) == _abi.TSDF_MAX_VIEWS == 16
    assert (int(defs["OLSR_TSDF_FEAT_FLOAT"]), int(defs["OLSR_TSDF_FEAT_PACKED_RGB"])) == (_abi.TSDF_FEAT_FLOAT, _abi.TSDF_FEAT_PACKED_RGB)
    assert (int(defs["OLSR_TSDF_IMAGE_CHANNELS"]), int(defs["OLSR_TSDF_IMAGE_ROWS"])) == (_abi.TSDF_IMAGE_CHANNELS, _abi.TSDF_IMAGE_ROWS)
    # sixteen views and the volume fit the 4 KiB of kernel arguments
    assert 16 * C.sizeof(_abi.OlsrTsdfView) + C.sizeof(_abi.OlsrTsdfVolume) + 8 <= 4096


def _volume(**kw):
    from online_lang_splatting_amd import _abi
    a = dict(X=4, Y=5, Z=6, F=15, feat_mode=_abi.TSDF_FEAT_FLOAT, voxel_size=0.02, trunc_margin=0.1, tsdf=X, weight=X, feat=X)
    a.update(kw)
    return _abi.OlsrTsdfVolume(**a)


def _view(**kw):
    from online_lang_splatting_amd import _abi
    a = dict(fx=30.0, fy=30.0, cx=15.5, cy=11.5, obs_weight=1.0, H=24, W=32, depth=X, feat=X)
    a.update(kw)
    return _abi.OlsrTsdfView(**a)


def test_entries_validate_their_arguments(L):
    from online_lang_splatting_amd import _abi
    ARG = _abi.OLSR_ERR_ARG
    ok = _volume()
    one = (_abi.OlsrTsdfView * 1)

    def integrate(vol, views):
        return L.olsr_tsdf_integrate(C.byref(vol), len(views), one(*views) if len(views) == 1 else (_abi.OlsrTsdfView * len(views))(*views), None)
    rows = [
        ("no volume", lambda: L.olsr_tsdf_init(None, None), "tsdf_init: volume is required"),
        ("empty", lambda: L.olsr_tsdf_init(C.byref(_volume(Y=0)), None), "tsdf_init: volume: X, Y, Z must be >= 1"),
        ("too large", lambda: L.olsr_tsdf_init(C.byref(_volume(X=2048, Y=1024, Z=1024)), None),
         "tsdf_init: volume: X Y Z must be below 2^31"),
        ("F", lambda: L.olsr_tsdf_init(C.byref(_volume(F=7)), None), "tsdf_init: volume: F must be one of 0, 3, 15, 16, 32"),
        ("packed F", lambda: L.olsr_tsdf_init(C.byref(_volume(feat_mode=1, F=3)), None),
         "tsdf_init: volume: F must be 1 with OLSR_TSDF_FEAT_PACKED_RGB"),
        ("mode", lambda: L.olsr_tsdf_init(C.byref(_volume(feat_mode=2)), None), "tsdf_init: volume: unknown feat_mode"),
        ("voxel size", lambda: L.olsr_tsdf_init(C.byref(_volume(voxel_size=0.0)), None),
         "tsdf_init: volume: voxel_size and trunc_margin must be > 0"),
        ("no feat", lambda: L.olsr_tsdf_init(C.byref(_volume(feat=None)), None),
         "tsdf_init: volume: tsdf, weight and (F > 0) feat are required"),
        ("no views", lambda: L.olsr_tsdf_integrate(C.byref(ok), 0, one(), None), "tsdf_integrate: between 1 and 16 views"),
        ("17 views", lambda: integrate(ok, [_view()] * 17), "tsdf_integrate: between 1 and 16 views"),
        ("NULL views", lambda: L.olsr_tsdf_integrate(C.byref(ok), 1, None, None), "tsdf_integrate: between 1 and 16 views"),
        ("view size", lambda: integrate(ok, [_view(W=0)]), "tsdf_integrate: a view's H, W must be >= 1 and 32 H W below 2^31"),
        ("view depth", lambda: integrate(ok, [_view(depth=None)]), "tsdf_integrate: a view's depth and (F > 0) feat are required"),
        ("view feat", lambda: integrate(ok, [_view(), _view(feat=None)]), "tsdf_integrate: a view's depth and (F > 0) feat are required"),
        ("view layout", lambda: integrate(ok, [_view(feat_layout=2)]), "tsdf_integrate: unknown feat_layout"),
        ("surface size", lambda: L.olsr_tsdf_surface_plan(C.byref(_volume(X=1024, Y=1024, Z=1024)), 0.0, X, X, None),
         "tsdf_surface_plan: volume: 3 X Y Z must be below 2^31"),
        ("plan scratch", lambda: L.olsr_tsdf_surface_plan(C.byref(ok), 0.0, None, X, None),
         "tsdf_surface_plan: scratch and status are required"),
        ("emit capacity", lambda: L.olsr_tsdf_surface_emit(C.byref(ok), 0.0, X, -1, X, X, X, None),
         "tsdf_surface_emit: scratch and capacity >= 0 are required"),
        ("emit points", lambda: L.olsr_tsdf_surface_emit(C.byref(ok), 0.0, X, 10, None, X, X, None),
         "tsdf_surface_emit: points and (F > 0) feats are required"),
        ("emit feats", lambda: L.olsr_tsdf_surface_emit(C.byref(ok), 0.0, X, 10, X, None, X, None),
         "tsdf_surface_emit: points and (F > 0) feats are required"),
    ]
    wrong = []
    for label, call, message in rows:
        rc = call()
        got = L.olsr_last_error().decode()
        if rc != ARG or got != message:
            wrong.append((label, rc, got))
    assert not wrong, wrong
    # nothing to emit is not an error, whatever the pointers
    assert L.olsr_tsdf_surface_emit(C.byref(ok), 0.0, X, 0, None, None, None, None) == _abi.OLSR_OK


def test_surface_scratch_size(L):
    # two int32 per block of 256 voxels in two carved sub-arrays: each may be padded to 256 bytes, and the base takes up to 256
    # more (tests/test_extents_cpu.py checks the layout itself)
    slack = 256 * (2 + 1)
    for dim, payload in (((1, 1, 1), 2 * 4), ((400, 250, 150), 2 * 4 * -(-400 * 250 * 150 // 256)), ((0, 5, 5), 0)):
        assert payload <= L.olsr_tsdf_surface_scratch_bytes(*dim) <= payload + slack, dim


def test_python_side_without_a_gpu():
    import online_lang_splatting_amd as pkg
    from online_lang_splatting_amd.tsdf import TSDFVolume, get_view_frustum
    assert pkg.TSDFVolume is TSDFVolume and "TSDFVolume" in pkg.__all__
    with pytest.raises(RuntimeError, match="GPU device is required"):
        TSDFVolume(np.array([[0, 1], [0, 1], [0, 1.0]]), 0.1, device="cpu")
    # the frustum: the camera centre and the four image corners at the largest depth, through the pose
    K = np.array([[50.0, 0, 20], [0, 40.0, 10], [0, 0, 1]])
    pose = np.eye(4)
    pose[:3, 3] = [1.0, 2.0, 3.0]
    depth = np.zeros((20, 40), np.float32)
    depth[3, 4] = 2.0
    fr = get_view_frustum(depth, K, pose)
    want = np.array([[0, 0, 0], [-0.8, -0.5, 2], [-0.8, 0.5, 2], [0.8, -0.5, 2], [0.8, 0.5, 2]]).T + pose[:3, 3:4]
    assert fr.shape == (3, 5) and np.allclose(fr, want, atol=1e-12)
    assert TSDFVolume.get_view_frustum is get_view_frustum
