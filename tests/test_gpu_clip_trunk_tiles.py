"""include/olsr_clip_trunk.h (HIP) beyond one pixel tile and one neuron tile.

Every launch of the tower tiles its work over 64 pixels x 64 neurons, and tests/test_gpu_clip_trunk.py compares with a truth
only where both tile indices are 0: its trunk runs at R = 32 (maps of 64, 16, 4 and 1 pixels, E = 64), its blocks on 5x7, 1x1
and 6x6.  tests/test_clip_trunk_ref_golden.py states that gap as a test: a kernel that ignored blockIdx.x, one that ignored
blockIdx.y or never wrote a partial neuron tile, and a three-launch block that lost its channel-major output would all have
given those cases' bits.  The cases here (tests/clip_trunk_ref.py: TRUNK_CASES, BLOCK_CASES; each note says what it resolves):

    wide       depths 1,1,2,1  dims 192,384,768,1536  E 48  R 64  image 50x75   real widths; stem on 4 pixel tiles; res3 from
                                                                               a three-launch block with both outputs; the
                                                                               downsample to 1536; head over 1536, partial
                                                                               neuron tile; up- and downsampling in one call
    tiles96    depths 1,1,2,1  dims 64,128,256,512    E 80  R 96  image 96x131  9 tiles, 2 1/4 tiles, head on 3x3 with two
                                                                               neuron tiles (the second partial); H = R
    tiles64    the same                                E 16  R 64  image 77x64   W = R; three waves of the head without neurons
    same_size  the small trunk                         E 64  R 32  image 32x32   H = W = R (the kernel samples with lambda = 0)
    one_row    the small trunk                         E 64  R 32  image 1x3     y0 = y1 = 0 everywhere
    deep       depths 1,1,30,1 dims 64,64,64,64       E 16  R 32  image 32x32   72 launches: the mask's second word
    blocks     C = 64, 128, 256 (the fused kernel's NT = 1, 2, 4), 320 (three launches, 5 partial sums, OUT = 1280) on 9x12
               (two tiles, w a multiple of 4) and 11x13 (three tiles, w = 1 mod 4, pixels with a full 7x7 window)

Yardstick: `_ratio_rule` of tests/test_gpu_lang_codec.py, unchanged, against the float64 truth of tests/clip_trunk_ref.py:
    max and rms of |hip - truth| <= max(4 x the same of ref32, 4 * 2^-24 max|truth|)
That 4x fits was measured on the CPU first, by the protocol of tests/test_gpu_hr_net.py's docstring (the float32 evaluation in
the kernels' order against ref32; tests/test_clip_trunk_ref_golden.py asserts every figure below 2 and max|truth| in
[1e-2, 1e3]; here max|truth| is 1.9 - 5.8).  (max ratio, rms ratio):
    wide      clip_vis_dense 0.43 0.43   res3 0.35 0.43   res2 0.91 0.93
    tiles96   clip_vis_dense 1.03 1.01   res3 0.99 1.01   res2 1.00 1.01
    tiles64   clip_vis_dense 0.61 0.69   res3 0.42 0.65   res2 0.73 0.93
    same_size clip_vis_dense 1.00 1.04   res3 0.51 0.65   res2 1.41 0.92
    one_row   clip_vis_dense 0.93 0.82   res3 0.57 0.70   res2 0.73 0.90
    deep      clip_vis_dense 1.08 0.95   res3 0.47 0.65   res2 1.12 0.94
    block 64  9x12 0.71 0.84  11x13 0.65 0.86     block 128  9x12 0.73 0.80  11x13 0.84 0.81
    block 256 9x12 1.00 0.75  11x13 0.99 0.79     block 320  9x12 0.76 0.69  11x13 0.73 0.69
(tiles96's ref32 is 20 x further from the truth than the other cases', 2e-5 to 3e-5: float32 source coordinates up to 130 in
the resize, which the kernels share; its ratios near 1.00 say so.)
On the GPU (MI355X) the kernels measured, hip against ref32 (max ratio, rms ratio):
    wide      clip_vis_dense 0.41 0.42   res3 0.22 0.43   res2 0.91 0.94
    tiles96   clip_vis_dense 0.99 1.01   res3 0.99 1.01   res2 1.00 1.01
    tiles64   clip_vis_dense 0.59 0.82   res3 0.77 0.81   res2 0.73 0.94
    same_size clip_vis_dense 0.54 0.76   res3 0.84 0.83   res2 1.51 0.92
    one_row   clip_vis_dense 0.45 0.53   res3 0.67 0.82   res2 0.73 0.90
    deep      clip_vis_dense 0.62 0.75   res3 0.58 0.82   res2 1.12 0.95
    block 64  9x12 1.00 0.93  11x13 0.67 0.92     block 128  9x12 0.90 0.85  11x13 0.97 0.85
    block 256 9x12 1.13 0.86  11x13 1.00 0.86     block 320  9x12 0.85 0.83  11x13 0.73 0.84
Worst: 1.51 in max (same_size res2: one element at 1.4e-6 against ref32's 9.3e-7; the CPU restatement of the kernels' order
gives 1.41 there, so it is the order, not the device), 1.01 in rms; the earlier cases' 0.47 - 1.12 for comparison.  The figures
move by a few per cent with the CPU that evaluates ref32.  This file, tests/test_gpu_clip_trunk.py and
tests/test_gpu_clip_trunk_extents.py in one run: 45 tests in 2.8 s, no test of this file above 0.5 s (wide, with its
references).  Nothing was found: every case passed as the kernels stood.
Everything else is exact: a second call's bits, a pixel against the other pixels of a constant map and against another launch
geometry, the launches one by one and word by word against the whole call.  References are computed once
(clip_trunk_ref._CASE_REFS, shared with the CPU tests) and trunks built once (TRUNKS).  Weights are drawn from seeds.
"""
import pytest
import torch

import clip_trunk_ref as R
from test_gpu_clip_trunk import DEV, _bits, _block_trunk, _trunk
from test_gpu_lang_codec import _ratio_rule

pytestmark = pytest.mark.gpu


def _case_trunk(case):
    from online_lang_splatting_amd import ClipTrunk
    kw = R.trunk_config(case)
    key = ("case", case["state_seed"]) + tuple(kw.values())
    return _trunk(key, lambda: ClipTrunk(DEV, R.trunk_case_state(case), **kw))


def _tile_block_trunk(c):
    return _trunk(("tiles", c), lambda: _block_trunk(c, R.block_state(c, c)))


@pytest.mark.parametrize("name", list(R.TRUNK_CASES))
def test_trunk_cases(hip, name):
    case = R.TRUNK_CASES[name]
    img, t64, t32, _ = R.trunk_case_refs(name)
    trunk, x = _case_trunk(case), img.to(DEV)
    out = {k: v.cpu().clone() for k, v in trunk.forward(x).items()}
    r, d = case["resolution"], case["dims"]
    assert {k: tuple(v.shape) for k, v in out.items()} == {"clip_vis_dense": (case["embed_dim"], r // 32, r // 32),
                                                           "res3": (d[1], r // 8, r // 8), "res2": (d[0], r // 4, r // 4)}
    for k in out:
        assert out[k].shape == t64[k].shape
        _ratio_rule(f"{name} {k}", out[k], t64[k], t32[k])
    for k, v in trunk.forward(x).items():
        assert _bits(v.cpu(), out[k]), f"two runs differ in {k}"


@pytest.mark.parametrize("name", list(R.BLOCK_CASES))
def test_block_cases(hip, name):
    state, x, t64, t32 = R.block_case_refs(name)
    trunk = _tile_block_trunk(R.BLOCK_CASES[name]["c"])
    out = trunk.block(x.to(DEV), 0, 0).cpu().clone()
    assert tuple(out.shape) == tuple(x.shape)
    _ratio_rule(f"block {name}", out, t64, t32)
    assert _bits(trunk.block(x.to(DEV), 0, 0).cpu(), out), "two runs differ"


@pytest.mark.parametrize("c", [64, 256, 320])
def test_a_pixel_does_not_depend_on_its_tile(hip, c):
    """A 20 x 20 map that is constant over space: every pixel whose 7x7 window lies inside the map (3 <= y, x < 17: 196 pixels
    in 7 of the 64-pixel tiles, at every lane position of the dense launches and every position in the depthwise kernel's
    groups of four) sees the same numbers in the same order, so it must have pixel (3, 3)'s bits in every channel; and so must
    the centre of the 7 x 7 map of the same values, where the window is the same and the launch geometry another (one tile,
    14 depthwise groups instead of 100).  64: the fused kernel; 256: its widest; 320: the three-launch block."""
    v = R.make_map(c, 1, 1, 200 + c)[:, 0, 0]      # on the 1/32 grid, as make_map rounds
    state = R.block_state(c, c)
    big, small = v[:, None, None].expand(c, 20, 20).contiguous(), v[:, None, None].expand(c, 7, 7).contiguous()
    # the float64 statement says so too: the interior is constant, equal to the small map's centre, and the border is not
    t_big, t_small = R.block(state, big, torch.float64), R.block(state, small, torch.float64)
    inner = t_big[:, 3:17, 3:17]
    assert float((inner - inner[:, :1, :1]).abs().max()) <= 1e-12
    assert float((inner[:, 0, 0] - t_small[:, 3, 3]).abs().max()) <= 1e-12
    assert float((t_big[:, 2, 3] - t_big[:, 3, 3]).abs().max()) > 1e-3 and float((t_big[:, 3, 2] - t_big[:, 3, 3]).abs().max()) > 1e-3
    trunk = _tile_block_trunk(c)
    out = trunk.block(big.to(DEV), 0, 0).cpu().clone()
    assert bool(torch.isfinite(out).all())
    want = out[:, 3:4, 3:4].expand(c, 14, 14)
    differ = out[:, 3:17, 3:17].contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    assert not bool(differ.any()), f"{int(differ.any(0).sum())} of 196 interior pixels differ from pixel (3, 3); first (c, y, x) " \
                                   f"{[int(i) for i in differ.nonzero()[0]]} (+3)"
    centre = trunk.block(small.to(DEV), 0, 0).cpu()[:, 3, 3]
    assert _bits(centre.contiguous(), out[:, 3, 3].contiguous()), "pixel (3, 3) of 20x20 differs from the centre of 7x7"
    assert float((out[:, 2, 3] - out[:, 3, 3]).abs().max()) > 1e-3


def test_mask_across_the_second_word(hip):
    """The deep trunk has 72 launches: bits 64 ... 71 lie in launches[1] (`int(launches) >> 64` in clip_trunk.py,
    `p.launches[k >> 6] >> (k & 63)` in the host code)."""
    from online_lang_splatting_amd._lib import OlsrError
    img = R.trunk_case_refs("deep")[0]
    trunk, x = _case_trunk(R.TRUNK_CASES["deep"]), img.to(DEV)
    assert trunk.n_launches == 72
    whole = {k: v.cpu().clone() for k, v in trunk.forward(x).items()}
    low, every = (1 << 64) - 1, (1 << 72) - 1

    def poison():
        for v in trunk.forward(x).values():
            v.fill_(float("nan"))
        trunk.workspace().zero_()

    def same(out, what):
        for k, v in out.items():
            assert _bits(v.cpu(), whole[k]), f"{what} differ from the whole call in {k}"

    poison()
    for k in range(72):
        out = trunk.forward(x, launches=1 << k)
    same(out, "the launches one by one")
    poison()
    trunk.forward(x, launches=low)
    same(trunk.forward(x, launches=every ^ low), "word 0 and then word 1")
    same(trunk.forward(x, launches=every), "all 72 bits")
    # a bit of word 1 is not read as a bit of word 0: launch 71 is the head, launch 7 (= 71 & 63) a block of stage 2
    poison()
    out = trunk.forward(x, launches=1 << 71)
    assert bool(torch.isnan(out["res2"]).all()) and bool(torch.isnan(out["res3"]).all())
    assert not bool(torch.isnan(out["clip_vis_dense"]).any()), "the head alone did not write clip_vis_dense"
    with pytest.raises(OlsrError, match="launch that does not exist"):
        trunk.forward(x, launches=1 << 72)
    same(trunk.forward(x), "a call after the masked ones")
