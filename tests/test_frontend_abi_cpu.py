"""The frame step's C-ABI and host layer without a GPU: the symbols load, the structs mirror include/olsr.h, every argument
error returns OLSR_ERR_ARG before anything touches the device (the pointers below are never dereferenced), and the host layer
refuses CPU tensors."""
import ctypes as C

import pytest
import torch

from online_lang_splatting_amd import _abi


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


PTR = 0x1000
W, H = 96, 64
N = W * H
ENTRIES = ("olsr_frontend_scratch_bytes", "olsr_grad_mask", "olsr_median_depth", "olsr_covisibility", "olsr_keyframe_decide")


def test_symbols_structs_and_exports(L):
    from online_lang_splatting_amd import _lib
    for s in ENTRIES:
        assert hasattr(L, s) and s in _lib.EXPORTS
    V, D = _abi.OlsrCovisViews, _abi.OlsrKeyframeDecideParams
    assert C.sizeof(V) == 8 + 8 * 16 and V.K.offset == 0 and V.vis.offset == 8
    assert C.sizeof(D) == 32
    for i, name in enumerate(("window_len", "window_size", "check_time", "single_thread", "kf_translation", "kf_min_translation",
                              "kf_overlap", "kf_cutoff")):
        assert getattr(D, name).offset == 4 * i, name
    assert (_abi.GRAD_MASK_BLOCKS, _abi.GRAD_MASK_GLOBAL, _abi.COVIS_MAX_VIEWS, _abi.COVIS_COUNTS) == (0, 1, 16, 33)
    assert _abi.KEYFRAME_RECORD_BYTES == 4 * (8 + _abi.KEYFRAME_RECORD_FLOATS) == 192
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "olsr.h")).read()
    for line in ("#define OLSR_GRAD_MASK_BLOCKS 0", "#define OLSR_GRAD_MASK_GLOBAL 1", "#define OLSR_COVIS_MAX_VIEWS 16",
                 "#define OLSR_COVIS_COUNTS 33", "#define OLSR_KEYFRAME_RECORD_FLOATS 40", "#define OLSR_KEYFRAME_RECORD_BYTES 192"):
        assert line in header, line
    assert L.olsr_frontend_scratch_bytes(N) >= 4 * N + 4 * 4 * 256
    assert L.olsr_frontend_scratch_bytes(1200 * 680) > L.olsr_frontend_scratch_bytes(N)
    import online_lang_splatting_amd as pkg
    for name in ("tracking_mask", "median_depth", "KeyframeSelector"):
        assert getattr(pkg, name) is not None and name in pkg.__all__


def _errors(L, fn, ok, rows, prefix):
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
        assert fn(*args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(prefix), (what, L.olsr_last_error())


def test_grad_mask_argument_errors(L):
    # W, H, plane_stride, mode, edge_threshold, image, mask, scratch, stream
    for mode in (_abi.GRAD_MASK_BLOCKS, _abi.GRAD_MASK_GLOBAL):
        ok = [W, H, N, mode, 4.0, PTR, PTR, PTR, None]
        rows = [("W = 0", {0: 0}), ("W < 0", {0: -W}), ("H = 0", {1: 0}), ("H < 0", {1: -1}), ("stride < W H", {2: N - 1}),
                ("stride < 0", {2: -N}), ("image", {5: None}), ("mask", {6: None}), ("mode", {3: 2}), ("mode < 0", {3: -1}),
                ("W H above int32", {0: 1 << 16, 1: 1 << 16, 2: 1 << 40})]
        _errors(L, L.olsr_grad_mask, ok, rows, b"grad_mask: ")
    blocks = [W, H, N, _abi.GRAD_MASK_BLOCKS, 4.0, PTR, PTR, None, None]
    rows = [("H < 32", {1: 31, 2: 1 << 20}), ("W < 32", {0: 31, 2: 1 << 20}),
            ("a block above 8192 pixels", {0: 3872, 1: 2208, 2: 1 << 30}),          # 121 x 69 = 8349
            ("a block's LDS rows above 64 KiB", {0: 32 * 8192, 1: 32, 2: 1 << 30})]   # 1 x 8192 pixels, 4 x 8194 floats
    _errors(L, L.olsr_grad_mask, blocks, rows, b"grad_mask: ")
    glob = [W, H, N, _abi.GRAD_MASK_GLOBAL, 4.0, PTR, PTR, PTR, None]
    _errors(L, L.olsr_grad_mask, glob, [("scratch", {7: None}), ("H < 2", {1: 1}), ("W < 2", {0: 1})], b"grad_mask: ")


def test_median_depth_argument_errors(L):
    # N, depth, opacity, mask, scratch, median, count, stream
    ok = [N, PTR, PTR, None, PTR, PTR, PTR, None]
    rows = [("N = 0", {0: 0}), ("N < 0", {0: -5}), ("N above int32", {0: 1 << 31}), ("depth", {1: None}), ("opacity", {2: None}),
            ("scratch", {4: None}), ("median", {5: None}), ("count", {6: None}), ("depth, with a mask", {1: None, 3: PTR})]
    _errors(L, L.olsr_median_depth, ok, rows, b"median_depth: ")


def _views(K, null=None):
    v = _abi.OlsrCovisViews(K=K)
    for k in range(max(0, min(K, 16))):
        v.vis[k] = None if k == null else PTR
    return v


def test_covisibility_argument_errors(L):
    # P, n_touched, views, cur_out, counts, stream
    ok = [1000, PTR, _views(3), None, PTR, None]
    rows = [("P = 0", {0: 0}), ("P < 0", {0: -1}), ("P above int32", {0: 1 << 31}), ("n_touched", {1: None}), ("views", {2: None}),
            ("counts", {4: None}), ("K < 0", {2: _views(-1)}), ("K = 17", {2: _views(17)}), ("vis[1] NULL", {2: _views(3, null=1)}),
            ("vis[15] NULL", {2: _views(16, null=15)}), ("counts, with cur_out", {3: PTR, 4: None})]
    _errors(L, L.olsr_covisibility, ok, rows, b"covisibility: ")


def _decide(**kw):
    p = dict(window_len=3, window_size=8, check_time=1, single_thread=0, kf_translation=0.08, kf_min_translation=0.05,
             kf_overlap=0.9, kf_cutoff=0.4)
    p.update(kw)
    return _abi.OlsrKeyframeDecideParams(**p)


def test_keyframe_decide_argument_errors(L):
    # params, counts, median, cur_pose, kf_poses, record, stream
    ok = [_decide(), PTR, PTR, PTR, PTR, PTR, None]
    rows = [("params", {0: None}), ("counts", {1: None}), ("median", {2: None}), ("cur_pose", {3: None}), ("kf_poses", {4: None}),
            ("record", {5: None}), ("window_len < 0", {0: _decide(window_len=-1)}), ("window_len = 17", {0: _decide(window_len=17)}),
            ("window_size = 0", {0: _decide(window_size=0)}), ("window_size < 0", {0: _decide(window_size=-3)}),
            ("record, empty window", {0: _decide(window_len=0), 4: None, 5: None})]
    _errors(L, L.olsr_keyframe_decide, ok, rows, b"keyframe_decide: ")


def test_host_layer_needs_a_gpu():
    from online_lang_splatting_amd import KeyframeSelector, median_depth, tracking_mask
    with pytest.raises(RuntimeError, match="GPU"):
        tracking_mask(torch.zeros(3, H, W), 4.0)
    with pytest.raises(RuntimeError, match="GPU"):
        median_depth(torch.ones(H, W), torch.ones(H, W))
    sel = KeyframeSelector(8, 4, 0.08, 0.05, 0.9)
    with pytest.raises(RuntimeError, match="GPU"):
        sel.add_keyframe(0, torch.eye(4), torch.ones(10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU"):
        sel.observe(1, torch.ones(10, dtype=torch.int32), torch.eye(4), torch.ones(H, W), torch.ones(H, W))
    with pytest.raises(ValueError):
        KeyframeSelector(17, 4, 0.08, 0.05, 0.9)
