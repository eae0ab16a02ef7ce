"""The keyframe seeding's C-ABI and host layer without a GPU: the symbols load, the struct mirrors include/olsr.h, every
argument error returns OLSR_ERR_ARG before anything touches the device (the pointers below are never dereferenced), and
seed_rows refuses a CPU tensor."""
import ctypes as C

import pytest
import torch

from online_lang_splatting_amd import _abi


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


W, H = 64, 48
N = W * H


def _params(**kw):
    p = dict(W=W, H=H, plane_stride=N, M=1, downsample=8, seed=3, fx=32.0, fy=32.0, cx=31.5, cy=23.5,
             rgb_boundary_threshold=0.01, depth_trunc=100.0, point_size=0.05, adaptive_pointsize=1, capacity=N // 8)
    p.update(kw)
    return _abi.OlsrKeyframeSeedParams(**p)


PTR = 0x1000


def _rows(**kw):
    r = dict(means3D=PTR, shs=PTR, opacities=PTR, scales=PTR, rotations=PTR)
    r.update(kw)
    return _abi.OlsrMapBuffers(**r)


def test_symbols_and_struct_layout(L):
    from online_lang_splatting_amd import _lib
    for s in ("olsr_keyframe_seed_scratch_bytes", "olsr_keyframe_seed_plan", "olsr_keyframe_seed_finish"):
        assert hasattr(L, s) and s in _lib.EXPORTS
    S = _abi.OlsrKeyframeSeedParams
    # int32 W, H | int64 plane_stride | int32 M, downsample | uint32 seed | pad | double fx, fy, cx, cy | float threshold,
    # depth_trunc | double point_size | int32 adaptive_pointsize, capacity
    assert C.sizeof(S) == 88
    offsets = dict(W=0, H=4, plane_stride=8, M=16, downsample=20, seed=24, fx=32, fy=40, cx=48, cy=56,
                   rgb_boundary_threshold=64, depth_trunc=68, point_size=72, adaptive_pointsize=80, capacity=84)
    for name, off in offsets.items():
        assert getattr(S, name).offset == off, name
    assert L.olsr_keyframe_seed_scratch_bytes(W, H) >= 4 * N
    assert L.olsr_keyframe_seed_scratch_bytes(1200, 680) > L.olsr_keyframe_seed_scratch_bytes(W, H)
    import online_lang_splatting_amd as pkg
    assert pkg.seed_rows is not None and "seed_rows" in pkg.__all__
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    assert callable(GaussianMap.extend_from_rgbd)


BAD_PARAMS = [("W = 0", dict(W=0)), ("W < 0", dict(W=-4)), ("H = 0", dict(H=0)), ("H < 0", dict(H=-1)),
              ("downsample = 0", dict(downsample=0)), ("downsample < 0", dict(downsample=-8)),
              ("plane_stride < W H", dict(plane_stride=N - 1)), ("plane_stride < 0", dict(plane_stride=-N)),
              ("capacity < W H / downsample", dict(capacity=N // 8 - 1)), ("capacity < 0", dict(capacity=-1)),
              ("M = 0", dict(M=0)), ("M < 0", dict(M=-1)),
              ("fx = 0", dict(fx=0.0)), ("fx < 0", dict(fx=-32.0)), ("fx NaN", dict(fx=float("nan"))),
              ("fx inf", dict(fx=float("inf"))), ("fy = 0", dict(fy=0.0)), ("fy < 0", dict(fy=-1.0)),
              ("fy NaN", dict(fy=float("nan"))), ("fy inf", dict(fy=float("inf"))),
              ("depth_trunc = 0", dict(depth_trunc=0.0)), ("depth_trunc < 0", dict(depth_trunc=-100.0)),
              ("depth_trunc NaN", dict(depth_trunc=float("nan")))]


def _call(fn, args):
    a = [None if x is None else (C.byref(x) if isinstance(x, C.Structure) else x) for x in args]
    return fn(*a)


def test_plan_argument_errors(L):
    # params, image, depth, exposure, w2c, rows, pix_index, scratch, status, aux, stream
    ok = [_params(), PTR, PTR, None, PTR, _rows(), PTR, PTR, PTR, PTR, None]
    rows = [("params", {0: None}), ("image", {1: None}), ("depth", {2: None}), ("w2c", {4: None}), ("rows", {5: None}),
            ("pix_index", {6: None}), ("scratch", {7: None}), ("status", {8: None}), ("aux", {9: None})]
    rows += [(f"rows.{k}", {5: _rows(**{k: None})}) for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    rows += [(what, {0: _params(**kw)}) for what, kw in BAD_PARAMS]
    # an exposure pointer changes nothing about the checks
    rows += [("image, with an exposure", {1: None, 3: PTR})]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert _call(L.olsr_keyframe_seed_plan, args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"keyframe_seed_plan: "), what
    assert _call(L.olsr_keyframe_seed_plan, [_params(depth_trunc=0.0)] + ok[1:]) == _abi.OLSR_ERR_ARG
    assert b"depth_trunc must be > 0" in L.olsr_last_error()


def test_finish_argument_errors(L):
    # params, n, rows, aux, scratch, knn_scratch, stream
    ok = [_params(), 100, _rows(), PTR, PTR, PTR, None]
    rows = [("params", {0: None}), ("n < 0", {1: -1}), ("n > capacity", {1: N // 8 + 1}), ("rows", {2: None}),
            ("aux", {3: None}), ("scratch", {4: None}), ("knn_scratch", {5: None}), ("rows.means3D", {2: _rows(means3D=None)}),
            ("rows.scales", {2: _rows(scales=None)}), ("n > W H", {0: _params(W=4, H=4, plane_stride=16, capacity=200)})]
    rows += [(what, {0: _params(**kw)}) for what, kw in BAD_PARAMS]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert _call(L.olsr_keyframe_seed_finish, args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"keyframe_seed_finish: "), what
    # fewer than four rows: no three neighbours, OLSR_OK with nothing written (no launch: the pointers are never used)
    for n in (0, 1, 3):
        assert _call(L.olsr_keyframe_seed_finish, [_params(), n, _rows(), PTR, PTR, None, None]) == _abi.OLSR_OK


def test_seed_rows_needs_a_gpu():
    from online_lang_splatting_amd import seed_rows
    with pytest.raises(RuntimeError, match="GPU"):
        seed_rows(torch.zeros(3, H, W), torch.ones(H, W), torch.eye(4), (32.0, 32.0, 31.5, 23.5), downsample=8, seed=0)
