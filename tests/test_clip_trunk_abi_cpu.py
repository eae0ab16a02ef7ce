"""The CLIP image tower's C-ABI and host layer without a GPU: the symbols load, the structs mirror include/olsr_clip_trunk.h,
every argument error returns OLSR_ERR_ARG before anything touches the device (the pointers below are never dereferenced), the
workspace of the real configuration proves that stage 0's hidden map is never stored whole, the packed layout is the header's,
and the host layer refuses a CPU device and a state dict with a missing or an unused `visual.*` entry."""
import ctypes as C
import os
import re

import pytest
import torch

from online_lang_splatting_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "olsr_clip_trunk.h")
PTR = 0x1000
REAL = dict(depths=_abi.CLIP_TRUNK_DEPTHS, dims=_abi.CLIP_TRUNK_DIMS, embed_dim=_abi.CLIP_TRUNK_EMBED, R=768)


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


def _t(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=64, H=20, W=27, R=32, mean=_abi.CLIP_PIXEL_MEAN,
       std=_abi.CLIP_PIXEL_STD, ln_eps=1e-6, launches=(0, 0), workspace_bytes=1 << 40):
    p = _abi.OlsrClipTrunkParams(embed_dim=embed_dim, H=H, W=W, R=R, ln_eps=ln_eps, workspace_bytes=workspace_bytes)
    p.depths[:], p.dims[:], p.mean[:], p.std[:], p.launches[:] = depths, dims, mean, std, launches
    return p


def _b(C_=64, h=5, w=7, ln_eps=1e-6, workspace_bytes=1 << 40):
    return _abi.OlsrConvnextBlockParams(C=C_, h=h, w=w, ln_eps=ln_eps, workspace_bytes=workspace_bytes)


def _fields(code, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [n.strip().split("[")[0] for n in decl.strip().split(None, 1)[1].split(",")]
    return out


def test_symbols_structs_and_exports(L):
    from online_lang_splatting_amd import _lib, build
    header = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(olsr_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.EXPORTS_CLIP_TRUNK)
    assert not set(_lib.EXPORTS_CLIP_TRUNK) & set(_lib.EXPORTS + _lib.EXPORTS_SINGLE_STAGE + _lib.EXPORTS_FRAME_INGEST
                                                  + _lib.EXPORTS_MAP_IO)
    for name in _lib.EXPORTS_CLIP_TRUNK:
        assert hasattr(L, name), name
    S = _abi.OlsrClipTrunkParams
    assert _fields(code, "olsr_clip_trunk_params") == [f[0] for f in S._fields_]
    assert C.sizeof(S) == 112
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 16, 32, 36, 40, 44, 48, 60, 72, 76, 80, 88, 104]
    B = _abi.OlsrConvnextBlockParams
    assert _fields(code, "olsr_convnext_block_params") == [f[0] for f in B._fields_]
    assert C.sizeof(B) == 32 and [getattr(B, f[0]).offset for f in B._fields_] == [0, 4, 8, 12, 16, 24]
    for line, value in (("#define OLSR_CLIP_TRUNK_FUSED_MAX_C 256", _abi.CLIP_TRUNK_FUSED_MAX_C),
                        ("#define OLSR_CLIP_TRUNK_MAX_LAUNCHES 128", _abi.CLIP_TRUNK_MAX_LAUNCHES),
                        ("#define OLSR_CLIP_TRUNK_MAX_DIM 4096", _abi.CLIP_TRUNK_MAX_DIM)):
        assert line in header and int(line.split()[-1]) == value, line
    assert "erff" in header and "OUT OF SCOPE" in header and "PACKED PARAMETERS" in header
    assert any(u[0] == "k_clip_trunk.hip" for u in build.UNITS) and any(h.endswith("olsr_clip_trunk.h") for h in build.HEADERS)
    import online_lang_splatting_amd as pkg
    assert pkg.ClipTrunk is not None and "ClipTrunk" in pkg.__all__


BAD_CONFIGS = [("a dim that is no multiple of 64", dict(dims=(64, 128, 200, 512))), ("a dim of 0", dict(dims=(0, 128, 256, 512))),
               ("a negative dim", dict(dims=(64, -128, 256, 512))), ("a dim above the limit", dict(dims=(64, 128, 256, 8192))),
               ("R no multiple of 32", dict(R=48)), ("R = 0", dict(R=0)), ("R < 0", dict(R=-32)), ("R above the limit", dict(R=8192)),
               ("a depth of 0", dict(depths=(1, 0, 2, 1))), ("a negative depth", dict(depths=(1, 1, -2, 1))),
               ("more launches than the mask holds", dict(depths=(1, 1, 60, 1))),
               ("embed_dim no multiple of 16", dict(embed_dim=40)), ("embed_dim = 0", dict(embed_dim=0)),
               ("H = 0", dict(H=0)), ("W < 0", dict(W=-27)), ("3 H W above int32", dict(H=1 << 15, W=1 << 15)),
               ("std = 0", dict(std=(68.5, 0.0, 70.3))), ("std nan", dict(std=(68.5, float("nan"), 70.3))),
               ("mean inf", dict(mean=(float("inf"), 116.7, 104.1)))]


def test_trunk_argument_errors(L):
    # params, image, packed_params, res2, res3, clip_vis_dense, workspace, stream
    ok = [_t(), PTR + 4, PTR, PTR + 4, PTR + 8, PTR + 12, PTR, None]
    rows = [("params", {0: None})] + [(what, {0: _t(**kw)}) for what, kw in BAD_CONFIGS]
    rows += [("ln_eps = 0", {0: _t(ln_eps=0.0)}), ("ln_eps < 0", {0: _t(ln_eps=-1e-6)}), ("ln_eps nan", {0: _t(ln_eps=float("nan"))}),
             ("a launch bit beyond the last launch", {0: _t(launches=(1 << 17, 0))}),
             ("a launch bit in the second word", {0: _t(launches=(0, 1))}),
             ("a small workspace", {0: _t(workspace_bytes=64)}), ("no workspace bytes", {0: _t(workspace_bytes=0)}),
             ("image", {1: None}), ("packed_params", {2: None}), ("res2", {3: None}), ("res3", {4: None}),
             ("clip_vis_dense", {5: None}), ("workspace", {6: None}),
             ("packed_params at 4 mod 16", {2: PTR + 4}), ("workspace at 8 mod 16", {6: PTR + 8}),
             ("image at 2 mod 4", {1: PTR + 2}), ("res2 at 1 mod 4", {3: PTR + 1}), ("clip_vis_dense at 3 mod 4", {5: PTR + 3})]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
        assert L.olsr_clip_trunk_forward(*args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"clip_trunk_forward: "), (what, L.olsr_last_error())
    # the small configuration has 2 + 3 + (2 + 2 + 2 * 2 + 3) + 1 = 17 launches: bit 16 is its last
    assert L.olsr_clip_trunk_launches(C.byref(_t())) == 17


def test_block_argument_errors(L):
    # params, x, block_params, y, workspace, stream
    ok = [_b(), PTR + 4, PTR, PTR + 8, PTR, None]
    rows = [("params", {0: None}), ("C no multiple of 64", {0: _b(C_=96)}), ("C = 0", {0: _b(C_=0)}), ("C < 0", {0: _b(C_=-64)}),
            ("C above the limit", {0: _b(C_=8192)}), ("h = 0", {0: _b(h=0)}), ("w < 0", {0: _b(w=-7)}),
            ("4 C h w above int32", {0: _b(C_=1536, h=1 << 10, w=1 << 10)}), ("ln_eps = 0", {0: _b(ln_eps=0.0)}),
            ("a small workspace", {0: _b(workspace_bytes=2 * 64 * 35 * 4 - 1)}),
            ("x", {1: None}), ("block_params", {2: None}), ("y", {3: None}), ("workspace", {4: None}),
            ("block_params at 4 mod 16", {2: PTR + 4}), ("workspace at 4 mod 16", {4: PTR + 4}), ("y at 2 mod 4", {3: PTR + 2})]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
        assert L.olsr_convnext_block(*args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"convnext_block: "), (what, L.olsr_last_error())
    assert L.olsr_convnext_block_workspace_bytes(64, 5, 7) == 2 * 64 * 35 * 4          # fused: the map twice
    assert L.olsr_convnext_block_workspace_bytes(512, 5, 7) == 6 * 512 * 35 * 4        # three launches: and the hidden map
    for bad in ((96, 5, 7), (0, 5, 7), (64, 0, 7), (64, 5, -1), (8192, 5, 7), (1536, 1 << 10, 1 << 10)):
        assert L.olsr_convnext_block_workspace_bytes(*bad) == 0, bad


def test_workspace_bytes(L):
    for what, kw in BAD_CONFIGS:
        p = _t(**kw)
        assert L.olsr_clip_trunk_workspace_bytes(C.byref(p)) == 0, what
        assert L.olsr_clip_trunk_packed_floats(C.byref(p)) == 0 and L.olsr_clip_trunk_launches(C.byref(p)) == 0, what
    assert L.olsr_clip_trunk_workspace_bytes(None) == 0
    real = _t(H=680, W=1200, **REAL)
    n = L.olsr_clip_trunk_workspace_bytes(C.byref(real))
    stage0_map = 192 * 192 * 192 * 4
    # two stage-0 maps plus one whole stage-0 hidden map would be 6 of these: below it, the hidden map is never stored whole
    assert 0 < n < 6 * stage0_map
    assert n == 4 * stage0_map        # two maps and stage 1's hidden map, the largest of a three-launch stage
    # the image's size adds nothing: it is sampled in place
    assert L.olsr_clip_trunk_workspace_bytes(C.byref(_t(H=1, W=1, **REAL))) == n
    # stem 2, downsamples 3, stage 0's blocks 2 launches each, the others 3, head 1
    assert L.olsr_clip_trunk_launches(C.byref(real)) == 2 + 3 + 3 * 2 + (3 + 27 + 3) * 3 + 1 <= _abi.CLIP_TRUNK_MAX_LAUNCHES


def test_packed_layout_is_the_state_table(L):
    for kw in (dict(), dict(H=680, W=1200, **REAL)):
        p = _t(**kw)
        table = _abi.clip_trunk_state(tuple(p.depths), tuple(p.dims), p.embed_dim)
        total = 0
        for _, shape in table:
            n = 1
            for s in shape:
                n *= s
            assert total % 4 == 0        # every array starts 16-byte aligned
            total += n
        assert L.olsr_clip_trunk_packed_floats(C.byref(p)) == total
    c = 192
    assert sum(torch.Size(s).numel() for _, s in _abi.clip_block_state("b", c)) == 8 * c * c + 58 * c
    assert len(set(k for k, _ in table)) == len(table) and table[-1][0] == "visual.head.proj.weight"


def test_host_layer_needs_a_gpu_and_packs_round_trip():
    from online_lang_splatting_amd import ClipTrunk, clip_trunk
    with pytest.raises(RuntimeError, match="GPU"):
        ClipTrunk("cpu", depths=(1, 1, 1, 1), dims=(64, 64, 64, 64), embed_dim=16, resolution=32)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ClipTrunk("cuda:0", depths=(1, 1, 1, 1), dims=(64, 72, 64, 64), embed_dim=16, resolution=32)
    g = torch.Generator().manual_seed(0)
    for name, shape in (("b.conv_dw.weight", (64, 1, 7, 7)), ("s.downsample.1.weight", (128, 64, 2, 2)), ("b.mlp.fc1.weight", (8, 4))):
        w = torch.randn(shape, generator=g)
        packed = clip_trunk._pack(name, w).reshape(-1).clone()
        assert torch.equal(clip_trunk._unpack(name, packed, shape), w), name
    w = torch.randn(64, 1, 7, 7, generator=g)
    assert torch.equal(clip_trunk._pack("conv_dw.weight", w).reshape(49, 64)[3 * 7 + 5], w[:, 0, 3, 5])      # [ky kx][c]
    w = torch.randn(128, 64, 2, 2, generator=g)
    assert torch.equal(clip_trunk._pack("downsample.1.weight", w).reshape(128, 4, 64)[:, 2 * 1 + 0], w[:, :, 1, 0])
