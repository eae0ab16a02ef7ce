"""The frame ingest's C-ABI and host layer without a GPU: the symbol loads, the struct mirrors include/olsr_frame_ingest.h,
every argument error returns OLSR_ERR_ARG before anything touches the device (the pointers below are never dereferenced), and
the host layer refuses CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from online_lang_splatting_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "olsr_frame_ingest.h")


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


PTR = 0x1000
W, H = 96, 64
N = W * H


def test_symbol_struct_and_exports(L):
    from online_lang_splatting_amd import _lib
    header = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(olsr_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.EXPORTS_FRAME_INGEST) == ["olsr_frame_ingest"]
    assert hasattr(L, "olsr_frame_ingest")
    S = _abi.OlsrFrameIngestParams
    # int32 W, H, depth_type, _pad0; int64 plane_stride; double depth_scale: no implicit padding
    fields = re.search(r"typedef struct olsr_frame_ingest_params \{(.*?)\} olsr_frame_ingest_params;", code, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in S._fields_] == ["W", "H", "depth_type", "_pad0", "plane_stride", "depth_scale"]
    assert C.sizeof(S) == 32
    assert [getattr(S, n).offset for n in names] == [0, 4, 8, 12, 16, 24]
    assert [getattr(S, n).size for n in names] == [4, 4, 4, 4, 8, 8]
    for line in ("#define OLSR_INGEST_DEPTH_U16 0", "#define OLSR_INGEST_DEPTH_F32 1"):
        assert line in header, line
    assert (_abi.INGEST_DEPTH_U16, _abi.INGEST_DEPTH_F32) == (0, 1)
    assert "cv2.remap" in header and "OUT OF SCOPE" in header    # the undistortion branch is stated as out of scope
    import online_lang_splatting_amd as pkg
    assert pkg.ingest_frame is not None and "ingest_frame" in pkg.__all__


def _p(**kw):
    p = dict(W=W, H=H, depth_type=_abi.INGEST_DEPTH_U16, plane_stride=N, depth_scale=6553.5)
    p.update(kw)
    return _abi.OlsrFrameIngestParams(**p)


def test_argument_errors(L):
    # params, rgb, depth, image, depth_out, stream
    ok = [_p(), PTR + 1, PTR, PTR, PTR, None]
    rows = [("params", {0: None}), ("W = 0", {0: _p(W=0)}), ("W < 0", {0: _p(W=-W)}), ("H = 0", {0: _p(H=0)}),
            ("H < 0", {0: _p(H=-1)}), ("W H above int32", {0: _p(W=1 << 16, H=1 << 16, plane_stride=1 << 40)}),
            ("stride < W H", {0: _p(plane_stride=N - 1)}), ("stride < 0", {0: _p(plane_stride=-N)}),
            ("depth_type", {0: _p(depth_type=2)}), ("depth_type < 0", {0: _p(depth_type=-1)}),
            ("scale = 0", {0: _p(depth_scale=0.0)}), ("scale < 0", {0: _p(depth_scale=-1.0)}),
            ("scale nan", {0: _p(depth_scale=float("nan"))}), ("scale inf", {0: _p(depth_scale=float("inf"))}),
            ("rgb", {1: None}), ("depth", {2: None}), ("image", {3: None}), ("depth_out", {4: None}),
            ("uint16 depth at an odd address", {2: PTR + 1}),
            ("float depth at address 2 mod 4", {0: _p(depth_type=_abi.INGEST_DEPTH_F32), 2: PTR + 2}),
            ("image at address 2 mod 4", {3: PTR + 2}), ("depth_out at address 1 mod 4", {4: PTR + 1})]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
        assert L.olsr_frame_ingest(*args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"frame_ingest: "), (what, L.olsr_last_error())


def test_host_layer_needs_a_gpu():
    from online_lang_splatting_amd import ingest_frame
    with pytest.raises(RuntimeError, match="GPU"):
        ingest_frame(torch.zeros(H, W, 3, dtype=torch.uint8), torch.zeros(H, W, dtype=torch.uint16), 6553.5)
