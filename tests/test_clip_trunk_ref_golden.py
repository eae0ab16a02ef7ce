"""tests/clip_trunk_ref.py against vectors recorded from the reference's own ConvNextBlock and LayerNorm
(tests/golden/clip_trunk.npz, made by tests/golden/make_golden_clip_trunk.py), without a GPU.

  - block() equals the recorded float64 outputs to 1e-12 and the recorded float32 outputs BIT FOR BIT: the restatement issues
    the same torch ops (conv2d, layer_norm, linear, gelu, linear, mul, add) on the same machine code, so nothing is left to an
    ulp.  The channels_first LayerNorm likewise, and the channels_last one through F.layer_norm.
  - the drawn parameters are the recorded ones (the drawing is pinned, so the seeds of the GPU tests mean something).
  - every case the GPU tests compare by the ratio rule has a finite float64 truth with 1e-2 <= max|truth| <= 1e3: otherwise
    the rule would compare noise.
  - the protocol of tests/test_gpu_hr_net.py's docstring: the float32 evaluation in the kernels' order against the reference's
    float32 evaluation, both against truth.  Measured here (max ratio, rms ratio):
        c64_5x7 0.94 0.82   c64_1x1 0.77 1.15   c192_5x7 0.73 0.72   c192_1x1 1.00 1.06
        small trunk, 20x27 image: clip_vis_dense 0.57 0.70   res3 0.45 0.64   res2 0.89 0.91
    All below 2, so the 4x of the GPU tests' rule stands as it is.  They were not at first: with every dense output as ONE
    chain of single roundings, c192_1x1 measured 2.29 (max) and 1.90 (rms), fc2's 768 terms being the long chain.  As the
    protocol asks, the kernels' order was changed, not the rule: a dense layer now sums each 64 k from zero and adds the
    partial sums to the running sum (include/olsr_clip_trunk.h, ARITHMETIC), and LayerNorm's sums are in double.  The
    figures are printed and asserted below 2.
"""
import pytest
import torch

import clip_trunk_ref as R
from online_lang_splatting_amd import _abi


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_block_equals_the_recorded_outputs(key):
    state, x, t64, t32 = R.golden_case(key)
    c, h, w, _ = R.GOLDEN_CASES[key]
    assert tuple(x.shape) == (c, h, w) and t64.dtype == torch.float64 and t32.dtype == torch.float32
    got64 = R.block(state, x, torch.float64)
    assert float((got64 - t64).abs().max()) <= 1e-12
    assert _bits(R.block(state, x, torch.float32), t32)
    # the branch is visible: gamma was drawn, not left at the reference's 1e-6
    assert float((t64 - x.double()).abs().max()) > 0.1


def test_drawn_parameters_are_the_recorded_ones():
    z = R.golden()
    for c in (64, 192):
        state = R.block_state(c, c, grid=int(z["grid"]))
        rec = R.golden_case(f"c{c}_1x1", z)[0]
        assert list(state) == list(rec) == list(R.BLOCK_KEYS)
        for k in state:
            assert _bits(state[k], rec[k]), (c, k)
        assert 0.05 <= float(state["gamma"].min()) and float(state["gamma"].max()) <= 0.2
    for key, (c, h, w, seed) in R.GOLDEN_CASES.items():
        assert _bits(R.make_map(c, h, w, seed), torch.from_numpy(z[f"{key}_x"]))


def test_layer_norm_both_formats():
    z = R.golden()
    x, w, b = (torch.from_numpy(z[k]) for k in ("ln_x", "ln_w", "ln_b"))
    assert float(z["ln_eps"]) == R.EPS == _abi.CLIP_LN_EPS
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        first = R.layer_norm_cf(x, w, b, dtype)
        last = R._ln2d(x.to(dtype)[None], w.to(dtype), b.to(dtype), R.EPS)[0]
        for got, name in ((first, "first"), (last, "last")):
            want = torch.from_numpy(z[f"ln_{name}_{tag}"])
            if dtype == torch.float64:
                assert float((got - want).abs().max()) <= 1e-12, name
            else:
                assert _bits(got.contiguous(), want), name
    # the two formats are one statement: they agree to float64 rounding
    assert float((torch.from_numpy(z["ln_first_f64"]) - torch.from_numpy(z["ln_last_f64"])).abs().max()) <= 1e-12


def _scale_ok(label, t):
    m = float(t.abs().max())
    print(f"{label}: max|truth| {m:.3e}")
    assert torch.isfinite(t).all() and 1e-2 <= m <= 1e3, (label, m)


def test_every_compared_case_has_an_order_one_truth():
    for key in R.GOLDEN_CASES:
        _scale_ok(key, R.golden_case(key)[2])
    for c in (192, 384, 768, 1536):
        st = R.block_state(c, c)
        for h, w in ((5, 7), (1, 1)):
            _scale_ok(f"block {c} {h}x{w}", R.block(st, R.make_map(c, h, w, c + h), torch.float64))
    st = R.trunk_state(1, **{k: R.SMALL[k] for k in ("depths", "dims", "embed_dim")})
    for hw in ((20, 27), (45, 61)):
        for k, v in R.forward(st, R.make_image(*hw, 1), torch.float64, **R.SMALL).items():
            _scale_ok(f"small trunk {hw} {k}", v)
    st = R.trunk_state(2, (27, 1, 1, 1), (64, 64, 64, 64), 16)
    x = R.make_map(64, 6, 6, 27).double()
    for j in range(27):
        x = R.block(st, x, torch.float64, prefix=f"visual.trunk.stages.0.blocks.{j}.")
    _scale_ok("27 blocks at C = 64", x)


def _ratios(label, ko, t64, t32):
    e_ko, e_ref = (ko.double() - t64).abs(), (t32.double() - t64).abs()
    mx = float(e_ko.max()) / float(e_ref.max())
    rm = float(e_ko.pow(2).mean().sqrt()) / float(e_ref.pow(2).mean().sqrt())
    print(f"{label}: kernel order against ref32: max ratio {mx:.2f}, rms ratio {rm:.2f}")
    assert mx < 2.0 and rm < 2.0, (label, mx, rm)


def test_kernel_order_stays_within_twice_the_float32_reference():
    for key in R.GOLDEN_CASES:
        state, x, t64, t32 = R.golden_case(key)
        _ratios(key, R.block_kernel_order(state, x), t64, t32)
    st = R.trunk_state(1, **{k: R.SMALL[k] for k in ("depths", "dims", "embed_dim")})
    img = R.make_image(20, 27, 1)
    ko = R.forward_kernel_order(st, img, **R.SMALL)
    t64, t32 = R.forward(st, img, torch.float64, **R.SMALL), R.forward(st, img, torch.float32, **R.SMALL)
    for k in ko:
        assert ko[k].shape == t64[k].shape
        _ratios(f"small trunk {k}", ko[k], t64[k], t32[k])
