"""A frame's ingest on the GPU (olsr_frame_ingest, frontend.ingest_frame) against the numpy restatement
tests/frame_ingest_ref.py, bit for bit, on the golden cases (which pin the restatement to the reference's statements) and on
the shapes at which the kernel takes another path.  Every call runs twice and must give the same bytes.

Shapes (W x H).  A lane takes four consecutive pixels of the flat frame, a workgroup 1024: 1 x 1 and 3 x 1 (one ragged lane,
bytes read one by one), 67 x 5 = 335 and 255 x 2 = 510 (a ragged last lane behind full ones), 128 x 3 (no ragged lane),
67 x 33 = 2211 (three workgroups), 2051 x 1025 (more lanes than the launch has: the grid-stride loop).
Addresses.  The byte stream starts 0, 1, 2 and 3 bytes past a 4-byte boundary (the aligned-word path lines the bytes up by
that shift; the lanes whose words would leave the stream read bytes); the depth 0 and one element past a 16-byte boundary
(vector or element loads); the outputs 0 and 4 bytes past one (16-byte or 4-byte stores), the image with a plane stride of
W H and of W H + 3 floats.  Inputs and outputs lie between guard bytes (tests/extent_harness.py): the guards, and the gap
between two planes, keep their fill, and every output word is written."""
import numpy as np
import pytest
import torch

import extent_harness as X
import frame_ingest_ref as R
from test_frame_ingest_ref_golden import GOLD, NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (3, 1), (67, 5), (128, 3), (255, 2), (67, 33)]
DEPTHS = {"u16": np.uint16, "f32": np.float32}


def put(array, misalign):
    """`array` on the device between guards, its first byte `misalign` bytes past a 256-byte boundary."""
    raw = np.ascontiguousarray(array).view(np.uint8).ravel()
    view = X.guarded(raw.size, misalign, DEV)
    view.copy_(torch.from_numpy(raw.copy()))
    dtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float32): torch.float32}[array.dtype]
    return view.view(dtype).view(array.shape)


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()


def run(rgb, depth, scale, rgb_shift=0, depth_shift=0, out_shift=None, gap=0):
    """-> (image, depth) as numpy; guards checked; two runs equal.  out_shift None: ingest_frame allocates."""
    from online_lang_splatting_amd import ingest_frame
    H, W = depth.shape
    N = W * H
    X.reset()
    d_rgb = put(rgb, rgb_shift)
    d_depth = put(depth, depth_shift * depth.dtype.itemsize)
    assert d_rgb.data_ptr() % 4 == rgb_shift % 4
    outs = []
    for _ in range(2):
        if out_shift is None:
            img, dep = ingest_frame(d_rgb, d_depth, scale)
            assert img.shape == (3, H, W) and dep.shape == (H, W) and img.dtype == dep.dtype == torch.float32
            X.check([d_rgb.view(-1), d_depth.view(-1).view(torch.uint8)])
        else:
            planes = X.guarded_tensor((3, N + gap), torch.float32, out_shift, DEV)
            out_d = X.guarded_tensor((H, W), torch.float32, out_shift, DEV)
            out_i = planes[:, :N].view(3, H, W)
            img, dep = ingest_frame(d_rgb, d_depth, scale, out_image=out_i, out_depth=out_d)
            assert img.data_ptr() == out_i.data_ptr() and dep.data_ptr() == out_d.data_ptr()
            X.check([d_rgb.view(-1), d_depth.view(-1).view(torch.uint8), planes, out_d], written=[out_i, out_d])
            if gap:
                assert bool((planes[:, N:].contiguous().view(torch.int32) == X.F32_PREFILL).all()), "the gap between two planes was written"
        outs.append((bits(img), bits(dep)))
        result = (img.cpu().numpy(), dep.cpu().numpy())
    assert outs[0] == outs[1], "two runs differ"
    assert bits(d_rgb) == np.ascontiguousarray(rgb).tobytes() and bits(d_depth) == np.ascontiguousarray(depth).tobytes()
    return result


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_golden_cases(name):
    rgb, depth, scale = GOLD[f"{name}_rgb"], GOLD[f"{name}_depth_in"], float(GOLD[f"{name}_scale"])
    want = R.ingest(rgb, depth, scale)
    assert same(want[0], GOLD[f"{name}_image"]) and same(want[1], GOLD[f"{name}_depth"])
    for rgb_shift in range(4):
        got = run(rgb, depth, scale, rgb_shift=rgb_shift, out_shift=0)
        assert same(got[0], want[0]) and same(got[1], want[1]), rgb_shift


@pytest.mark.parametrize("kind", sorted(DEPTHS))
@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes_and_addresses(W, H, kind):
    rgb, depth = R.synthetic_frame(W, H, DEPTHS[kind], seed=7 * W + H)
    if kind == "f32" and W * H >= 8:   # non-finite depths stay what they are
        depth.ravel()[[2, 5, 7]] = [np.nan, np.inf, -np.inf]
    scale = 6553.5 if (W + H) % 2 else 5000.0
    want = R.ingest(rgb, depth, scale)
    rows = [dict(out_shift=None)]
    rows += [dict(rgb_shift=s, depth_shift=s % 2, out_shift=4 * (s % 2), gap=3 * (s // 2)) for s in range(4)]
    for kw in rows:
        got = run(rgb, depth, scale, **kw)
        assert np.array_equal(np.isnan(got[1]), np.isnan(want[1]))
        assert same(got[0], want[0]), kw
        assert same(np.nan_to_num(got[1], nan=0.0), np.nan_to_num(want[1], nan=0.0)), kw


def test_more_lanes_than_the_launch_has():
    """2051 x 1025 pixels = 525 570 lanes of four against 2048 workgroups of 256: the loop takes a second turn."""
    from online_lang_splatting_amd import ingest_frame
    W, H = 2051, 1025
    rgb, depth = R.synthetic_frame(W, H, np.uint16, seed=3)
    want = R.ingest(rgb, depth, 1000.0)
    whole = torch.zeros(W * H * 3 + 8, dtype=torch.uint8, device=DEV)
    d_rgb = whole[3:3 + W * H * 3].view(H, W, 3)
    d_rgb.copy_(torch.from_numpy(rgb))
    d_depth = torch.from_numpy(depth).to(DEV)
    a = ingest_frame(d_rgb, d_depth, 1000.0)
    b = ingest_frame(d_rgb, d_depth, 1000.0)
    assert bits(a[0]) == bits(b[0]) == want[0].tobytes()
    assert bits(a[1]) == bits(b[1]) == want[1].tobytes()


def test_argument_errors():
    from online_lang_splatting_amd import ingest_frame
    H, W = 4, 6
    rgb = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    d16 = torch.zeros(H, W, dtype=torch.uint16, device=DEV)
    f32 = torch.zeros(H, W, dtype=torch.float32, device=DEV)
    ingest_frame(rgb, d16, 6553.5)
    ingest_frame(rgb, f32, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        ingest_frame(rgb.cpu(), d16, 6553.5)
    with pytest.raises(RuntimeError, match="GPU"):
        ingest_frame(rgb, d16.cpu(), 6553.5)
    with pytest.raises(RuntimeError, match="GPU"):
        ingest_frame(rgb, d16, 6553.5, out_depth=f32.cpu())
    bad = [dict(rgb_u8=rgb.float()), dict(rgb_u8=torch.zeros(3, H, W, dtype=torch.uint8, device=DEV)),
           dict(rgb_u8=torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)),
           dict(rgb_u8=torch.zeros(H, 2 * W, 3, dtype=torch.uint8, device=DEV)[:, ::2]),       # not contiguous
           dict(depth=d16.to(torch.int32)), dict(depth=f32.double()), dict(depth=torch.zeros(W, H, dtype=torch.uint16, device=DEV)),
           dict(depth=torch.zeros(H, 2 * W, dtype=torch.float32, device=DEV)[:, ::2]),
           dict(depth_scale=0.0), dict(depth_scale=-5000.0), dict(depth_scale=float("inf")), dict(depth_scale=float("nan")),
           dict(out_image=torch.zeros(3, H, W, dtype=torch.float64, device=DEV)),
           dict(out_image=torch.zeros(H, W, 3, dtype=torch.float32, device=DEV)),
           dict(out_image=torch.zeros(3, H, 2 * W, dtype=torch.float32, device=DEV)[:, :, ::2]),
           dict(out_depth=torch.zeros(H, W + 1, dtype=torch.float32, device=DEV)),
           dict(out_depth=torch.zeros(H, 2 * W, dtype=torch.float32, device=DEV)[:, ::2])]
    for kw in bad:
        args = dict(rgb_u8=rgb, depth=d16, depth_scale=6553.5)
        args.update(kw)
        with pytest.raises(ValueError, match="ingest_frame"):
            ingest_frame(**args)
