"""include/olsr_clip_trunk.h (HIP) and clip_trunk.ClipTrunk on the GPU: the CLIP ConvNeXt image tower.

Yardstick: the project's own, imported unchanged from tests/test_gpu_lang_codec.py.  With `truth` the float64 and `ref32` the
float32 evaluation of the reference's statement (tests/golden/clip_trunk.npz, recorded from the reference's ConvNextBlock;
tests/clip_trunk_ref.py, which tests/test_clip_trunk_ref_golden.py pins to that file bit for bit, for the other sizes):
    max and rms of |hip - truth| <= max(4 x the same of ref32, 4 * 2^-24 max|truth|)
Why 4x fits was measured on the CPU before the cases were trusted, by the protocol of tests/test_gpu_hr_net.py's docstring:
clip_trunk_ref.*_kernel_order, the float32 evaluation that adds up in the kernels' order, against ref32 (max ratio, rms ratio):
    c64_5x7 0.94 0.82   c64_1x1 0.77 1.15   c192_5x7 0.73 0.72   c192_1x1 1.00 1.06
    small trunk, 20x27 image: clip_vis_dense 0.57 0.70   res3 0.45 0.64   res2 0.89 0.91
All below 2, after the kernels' order (not the rule) was changed once: a dense layer as one chain of single roundings measured
2.29 at c192_1x1, so every 64 k are now summed from zero and added to the running sum, and LayerNorm's sums are in double.
tests/test_clip_trunk_ref_golden.py repeats the measurement and asserts it.  On the GPU the kernels measured 0.47 - 1.12 x
ref32 over the cases below (max 1.04 at C = 384 on 5x7, rms 1.12 at c64_1x1; the small trunk 0.47 - 0.97, 27 blocks in a row
0.91 / 0.95).  Every figure is printed.

Everything else is exact: repeated runs, the launches one by one against the whole call, an image plane at a 4-byte-but-not-
16-byte address, the keyframe chain against its steps by hand; a NaN reaches exactly the outputs the float64 statement says
it reaches.  References are computed once (REFS) and shared.  Weights are drawn from seeds, never committed.

test_stage_depth: the trunk does not expose a stage on its own, so the 27 blocks are compared through block() only.
test_keyframe_chain: the HR net's input widths are fixed (768, 384, 192), which rules the small trunk out; a small-spatial
trunk with E = 768, d1 = 384, d0 = 192 at R = 32 stands in (maps 1x1, 4x4, 8x8).
"""
import pytest
import torch

import clip_trunk_ref as R
from test_gpu_lang_codec import _ratio_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REFS = {}
TRUNKS = {}
SMALL_KW = dict(depths=R.SMALL["depths"], dims=R.SMALL["dims"], embed_dim=R.SMALL["embed_dim"])
B0 = "visual.trunk.stages.0.blocks.0."


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _trunk(key, make):
    if key not in TRUNKS:
        TRUNKS[key] = make()
    return TRUNKS[key]


def _small():
    from online_lang_splatting_amd import ClipTrunk
    return _trunk("small", lambda: ClipTrunk(DEV, R.trunk_state(1, **SMALL_KW), resolution=32, **SMALL_KW))


def _block_trunk(c, block_state):
    """A tower whose stage 0 is one block of c channels with `block_state`'s parameters (the rest small and unused)."""
    from online_lang_splatting_amd import ClipTrunk
    kw = dict(depths=(1, 1, 1, 1), dims=(c, 64, 64, 64), embed_dim=16)
    st = R.trunk_state(5, **kw)
    for k, v in block_state.items():
        assert st[B0 + k].shape == v.shape
        st[B0 + k] = v
    return ClipTrunk(DEV, st, resolution=32, **kw)


def _block_refs(c, h, w):
    """(state, x, truth, ref32) of the drawn block of width c on an h x w map, computed once."""
    key = ("block", c, h, w)
    if key not in REFS:
        st, x = R.block_state(c, c), R.make_map(c, h, w, c + h)
        REFS[key] = (st, x, R.block(st, x, torch.float64), R.block(st, x, torch.float32))
    return REFS[key]


def _small_refs(hw):
    key = ("small", hw)
    if key not in REFS:
        st, img = R.trunk_state(1, **SMALL_KW), R.make_image(*hw, 1)
        REFS[key] = (img, R.forward(st, img, torch.float64, **R.SMALL), R.forward(st, img, torch.float32, **R.SMALL))
    return REFS[key]


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_block_golden(hip, key):
    state, x, t64, t32 = R.golden_case(key)
    c = R.GOLDEN_CASES[key][0]
    trunk = _trunk(("golden", c), lambda: _block_trunk(c, state))
    out = trunk.block(x.to(DEV), 0, 0).cpu()
    assert tuple(out.shape) == tuple(x.shape)
    _ratio_rule(f"golden {key}", out, t64, t32)


@pytest.mark.parametrize("hw", [(5, 7), (1, 1)])
@pytest.mark.parametrize("c", [192, 384, 768, 1536])
def test_block_widths(hip, c, hw):
    state, x, t64, t32 = _block_refs(c, *hw)
    trunk = _trunk(("width", c), lambda: _block_trunk(c, state))
    out = trunk.block(x.to(DEV), 0, 0).cpu().clone()
    _ratio_rule(f"block C = {c} on {hw[0]}x{hw[1]}", out, t64, t32)
    assert _bits(trunk.block(x.to(DEV), 0, 0).cpu(), out), "two runs differ"


@pytest.mark.parametrize("c", [64, 512])
def test_block_nan(hip, c):
    """9 x 12 (two pixel tiles), a NaN at channel 17 of pixel (1, 10): the depthwise window carries it to rows 0..4, columns
    7..11 of that channel, LayerNorm to every channel of those 25 pixels, and nowhere else.  c = 64: the fused block; 512:
    the three-launch block."""
    state, x, _, _ = _block_refs(c, 9, 12)
    bad = x.clone()
    bad[17, 1, 10] = float("nan")
    want = torch.isnan(R.block(state, bad, torch.float64))
    assert int(want.sum()) == 25 * c and not bool(want[:, 5:].any()) and not bool(want[:, :, :7].any())
    trunk = _trunk(("width", c), lambda: _block_trunk(c, state))
    clean = trunk.block(x.to(DEV), 0, 0).cpu().clone()
    got = trunk.block(bad.to(DEV), 0, 0).cpu()
    assert torch.equal(torch.isnan(got), want)
    assert torch.equal(got[~want].view(torch.int32), clean[~want].view(torch.int32)), "a clean output changed"
    assert bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("hw", [(20, 27), (45, 61)])
def test_small_trunk(hip, hw):
    """depths (1, 1, 2, 1), dims (64, 128, 256, 512), E = 64, R = 32: maps of 8x8, 4x4, 2x2, 1x1.  20x27 is upsampled, 45x61
    downsampled; neither size is a multiple of anything."""
    img, t64, t32 = _small_refs(hw)
    trunk = _small()
    out = {k: v.cpu().clone() for k, v in trunk.forward(img.to(DEV)).items()}
    assert {k: tuple(v.shape) for k, v in out.items()} == {"clip_vis_dense": (64, 1, 1), "res3": (128, 4, 4), "res2": (64, 8, 8)}
    for k in out:
        _ratio_rule(f"small trunk {hw[0]}x{hw[1]} {k}", out[k], t64[k], t32[k])
    # an image whose planes start at a 4-byte-but-not-16-byte address
    buf = torch.zeros(3 * hw[0] * hw[1] + 1, device=DEV)
    shifted = buf[1:].view(3, *hw)
    shifted.copy_(img)
    assert shifted.data_ptr() % 16 == 4
    again = trunk.forward(shifted)
    for k in out:
        assert _bits(again[k].cpu(), out[k]), k


def test_stage_depth(hip):
    """27 blocks at C = 64 on a 6x6 map, the long chain of the real stage 2 at a size where float64 is instant."""
    from online_lang_splatting_amd import ClipTrunk
    kw = dict(depths=(27, 1, 1, 1), dims=(64, 64, 64, 64), embed_dim=16)
    st = R.trunk_state(2, **kw)
    trunk = ClipTrunk(DEV, st, resolution=32, **kw)
    x = R.make_map(64, 6, 6, 27)
    y, t64, t32 = x.to(DEV), x.double(), x
    for j in range(27):
        p = f"visual.trunk.stages.0.blocks.{j}."
        y = trunk.block(y, 0, j)
        t64, t32 = R.block(st, t64, torch.float64, prefix=p), R.block(st, t32, torch.float32, prefix=p)
    _ratio_rule("27 blocks at C = 64", y.cpu(), t64, t32)


def test_reproducible_and_mask(hip):
    img, _, _ = _small_refs((20, 27))
    trunk, x = _small(), img.to(DEV)
    whole = {k: v.cpu().clone() for k, v in trunk.forward(x).items()}
    for k, v in trunk.forward(x).items():
        assert _bits(v.cpu(), whole[k]), f"two runs differ in {k}"
    assert trunk.n_launches == 17
    for v in trunk.forward(x).values():
        v.fill_(float("nan"))
    trunk.workspace().zero_()
    for k in range(trunk.n_launches):
        out = trunk.forward(x, launches=1 << k)
    for k, v in out.items():
        assert _bits(v.cpu(), whole[k]), f"the launches one by one differ from the whole call in {k}"
    from online_lang_splatting_amd._lib import OlsrError
    with pytest.raises(OlsrError, match="launch that does not exist"):
        trunk.forward(x, launches=1 << trunk.n_launches)


def test_real_size_smoke(hip):
    """convnext_large at 768 x 768 with weights drawn on the device (785 MB) and a 680 x 1200 image: shapes, finiteness, equal
    bits twice, and an untouched guard behind the workspace.  No float64 truth at this size."""
    from online_lang_splatting_amd import ClipTrunk, _abi
    trunk = ClipTrunk(DEV)
    kw = dict(depths=_abi.CLIP_TRUNK_DEPTHS, dims=_abi.CLIP_TRUNK_DIMS, embed_dim=_abi.CLIP_TRUNK_EMBED)
    trunk.load_state_dict(R.trunk_state(3, device=DEV, **kw))
    assert trunk.flat.numel() * 4 > 780e6 and trunk.n_launches == 111
    n = trunk.workspace().numel()
    assert n == 4 * 192 * 192 * 192 * 4
    guarded = torch.full((n + 65536,), 0xA5, dtype=torch.uint8, device=DEV)
    assert guarded.data_ptr() % 16 == 0
    trunk._work = guarded[:n]
    img = R.make_image(680, 1200, 3, device=DEV)
    out = {k: v.clone() for k, v in trunk.forward(img).items()}
    assert {k: tuple(v.shape) for k, v in out.items()} == {"clip_vis_dense": (768, 24, 24), "res3": (384, 96, 96),
                                                           "res2": (192, 192, 192)}
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
        print(f"real size {k}: max|value| {float(v.abs().max()):.3e}")
    for k, v in trunk.forward(img).items():
        assert torch.equal(v.view(torch.int32), out[k].view(torch.int32)), f"two runs differ in {k}"
    assert bool((guarded[n:] == 0xA5).all()), "the guard behind the workspace was written"
    assert not bool((guarded[:n] == 0xA5).all())


def test_keyframe_chain(hip):
    import hr_net_ref as RH
    import lang_codec_ref as RC
    import lang_encoder_ref as RE
    from online_lang_splatting_amd import ClipTrunk
    from online_lang_splatting_amd.hr_net import HighResLanguageNet
    from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec
    from online_lang_splatting_amd.lang_encoder import LanguageEncoder
    from online_lang_splatting_amd.lang_single_stage import SingleStageTargets
    from online_lang_splatting_amd.slam_iterations import OnlineLanguageTargets
    from test_gpu_lang_single_stage import _encoder
    kw = dict(depths=(1, 1, 1, 1), dims=(192, 384, 64, 64), embed_dim=768)
    trunk = ClipTrunk(DEV, R.trunk_state(4, **kw), resolution=32, **kw)
    hr = HighResLanguageNet(DEV, RH.net_state(300))
    img = R.make_image(20, 27, 4, device=DEV)

    def by_hand():
        o = trunk.forward(img)
        return o["clip_vis_dense"][None], o["res3"][None], o["res2"][None]

    # single-stage targets: add_keyframe_backbone takes no encoder
    enc = _encoder()
    a, b = SingleStageTargets(enc, hw=(8, 8)), SingleStageTargets(enc, hw=(8, 8))
    call = trunk.feature_fn(hr)(7, img)
    assert call[0] == "add_keyframe_backbone" and len(call) == 5 and call[4] is hr
    ta = getattr(a, call[0])(7, *call[1:])            # what slam.py does with the tuple
    tb = b.add_keyframe_backbone(7, *by_hand(), hr)
    assert tuple(ta.shape) == (15, 8, 8) and torch.equal(ta, tb) and bool(torch.isfinite(ta).all())

    # online targets: it takes the general encoder
    def codec():
        c = OnlineLanguageCodec(DEV, seed=0)
        c.load_state_dict(RC.unflatten(RC.initial_params(1)))
        return c

    genc = LanguageEncoder(DEV, RE.encoder_state(11))
    a, b = OnlineLanguageTargets(codec(), lr=1e-3, hw=(8, 8)), OnlineLanguageTargets(codec(), lr=1e-3, hw=(8, 8))
    call = trunk.feature_fn(hr, genc)(7, img)
    assert len(call) == 6 and call[4] is hr and call[5] is genc
    ta = getattr(a, call[0])(7, *call[1:])
    tb = b.add_keyframe_backbone(7, *by_hand(), hr, genc)
    assert tuple(ta.shape) == (15, 8, 8) and torch.equal(ta, tb) and bool(torch.isfinite(ta).all())
    assert torch.equal(a.features[7], b.features[7]) and torch.equal(a.codec.flat, b.codec.flat)


def test_loader_is_loud_and_round_trips(hip):
    from online_lang_splatting_amd import ClipTrunk
    st = R.trunk_state(1, **SMALL_KW)
    trunk = _small()
    back = trunk.state_dict()
    assert list(back) == list(st)
    for k in st:
        assert _bits(back[k].cpu(), st[k]), k
    # an open_clip checkpoint also holds the text tower: ignored; wrapped in {"state_dict": ...}: unwrapped
    full = dict(st, **{"text.token_embedding.weight": torch.zeros(4, 4), "logit_scale": torch.zeros(())})
    fresh = ClipTrunk(DEV, {"state_dict": full}, resolution=32, **SMALL_KW)
    assert torch.equal(fresh.flat, trunk.flat)
    missing = {k: v for k, v in st.items() if k != "visual.trunk.stages.2.blocks.1.gamma"}
    with pytest.raises(RuntimeError, match="missing keys .*stages.2.blocks.1.gamma"):
        fresh.load_state_dict(missing)
    with pytest.raises(RuntimeError, match="unexpected keys .*visual.trunk.norm_pre.weight"):
        fresh.load_state_dict(dict(st, **{"visual.trunk.norm_pre.weight": torch.zeros(512)}))
    with pytest.raises(RuntimeError, match="has shape"):
        fresh.load_state_dict(dict(st, **{"visual.head.proj.weight": torch.zeros(64, 256)}))
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        trunk.forward(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="no block"):
        trunk.block(torch.zeros(256, 2, 2, device=DEV), 2, 2)
