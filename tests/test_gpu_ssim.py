"""olsr_refinement_loss (HIP), losses.ssim and slam_iterations.RefinementStep on the GPU.

The yardstick of the loss is not a tolerance chosen in advance but the reference's own float32 error.  With `truth` the
float64 and `ref32` the float32 evaluation by the reference's code (tests/golden/ssim.npz; at full size tests/ssim_ref.py,
which tests/test_ssim_ref_golden.py pins to the reference), err_hip = |hip - truth|, err_ref = |ref32 - truth|:
    gradient   max(err_hip) <= 4 max(err_ref) and rms(err_hip) <= 4 rms(err_ref)     (identical images: 8 instead of 4)
    scalars    |hip - truth| <= max(4 |ref32 - truth|, 4 * 2^-24)
Float32 SSIM is dominated by the cancellation in E[x^2] - mu^2, so the reference itself is off by 5e-4 of the gradient's
largest element on smooth images and exact to 1e-6 on noise: a fixed relative tolerance would be vacuous or unreachable.
4x: another summation order of the same float32 products has errors of the same size; 8x where both sides are rounding
noise around an exactly cancelling sum; 4 * 2^-24 is two ulp of a float32 of magnitude 1, which the scalars are.

The kernel accumulates its window sums in double (csrc/k_ssim.hip, "Precision"), so its ratios sit below 1.
Measured on an MI355X (the tests print every figure), gradient: max-error ratio / rms ratio, and the SSIM value's error
against the reference's own:
    golden 0 noise 40x56 l=0.2        0.16 / 0.22     SSIM error 1.6e-09 (ref32 9.0e-09)
    golden 1 smooth 64x48 l=0.2       0.029 / 0.055              2.8e-08 (3.9e-07)
    golden 2 constant 33x21 l=1       0.14 / 0.15                6.4e-09 (1.0e-06)
    golden 3 identical 33x21 l=1      2e-09 / 2e-09 (the kernel's gradient is an exact 0; rule 8)     0 (0)
    golden 4 noise 7x9 l=0.2          0.33 / 0.39                2.3e-08 (6.6e-08)
    golden 5 ties 33x21 l=0           1.0 / 1.0 (pure L1: the same float32 constant on both sides)    8.7e-10 (8.7e-10)
    1200x680 smooth l=0.2             0.012 / 0.044              1.8e-09 (1.8e-07)
    1199x679 constant l=0.2           0.040 / 0.073              2.6e-09 (1.0e-05)
    64x64 noise l=1                   0.14 / 0.17                2.1e-09 (1.3e-08)
    5x300 noise l=0.2                 0.36 / 0.41                9.0e-09 (2.1e-08)
Before the kernel applied the gain of the reference's rounded 2-D window (csrc/k_ssim.hip, SSIM_GAIN) the 1200x680 case missed
the scalar rule: SSIM error 7.8e-07 against an allowed 7.2e-07.  That was a property of the separable weights, not of the rule.
"""
import math
import random

import pytest
import torch

import ssim_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rms(e):
    return float(torch.sqrt((e.double() ** 2).mean()))


def _check(label, kind, hip, truth, ref32):
    """hip / truth / ref32: dict(loss[4], dL_dimage) on the CPU; prints every figure, then asserts the rule above."""
    factor = 8.0 if kind == "identical" else 4.0
    t = truth["dL_dimage"].double()
    e_hip = (hip["dL_dimage"].double() - t).abs()
    e_ref = (ref32["dL_dimage"].double() - t).abs()
    mx, rm = (float(e_hip.max()), float(e_ref.max())), (_rms(e_hip), _rms(e_ref))
    print(f"{label}: gradient scale {float(t.abs().max()):.3e}; max error hip {mx[0]:.3e} ref {mx[1]:.3e} "
          f"(ratio {mx[0] / mx[1] if mx[1] > 0 else float('nan'):.3g}); rms hip {rm[0]:.3e} ref {rm[1]:.3e} "
          f"(ratio {rm[0] / rm[1] if rm[1] > 0 else float('nan'):.3g})")
    l_hip, l_t, l_ref = hip["loss"].double(), truth["loss"].double(), ref32["loss"].double()
    for k, name in enumerate(("total", "(1-l) L1", "l (1-SSIM)", "SSIM")):
        print(f"{label}: {name}: hip {float(l_hip[k]):.9g} truth {float(l_t[k]):.9g}; error hip {abs(float(l_hip[k] - l_t[k])):.3e} "
              f"ref {abs(float(l_ref[k] - l_t[k])):.3e}")
    assert torch.isfinite(hip["dL_dimage"]).all() and torch.isfinite(hip["loss"]).all(), label
    assert mx[0] <= factor * mx[1], (label, "max", mx)
    assert rm[0] <= factor * rm[1], (label, "rms", rm)
    for k in range(4):
        assert abs(float(l_hip[k] - l_t[k])) <= max(4.0 * abs(float(l_ref[k] - l_t[k])), 4.0 * 2.0 ** -24), (label, k)


def _hip(image, gt, lam, **kw):
    from online_lang_splatting_amd import losses
    o = losses.refinement_loss(image.to(DEV), gt.to(DEV), lambda_dssim=lam, **kw)
    torch.cuda.synchronize()
    return dict(loss=o["loss"].cpu(), dL_dimage=None if o["dL_dimage"] is None else o["dL_dimage"].cpu())


@pytest.mark.parametrize("i", range(6))
def test_golden_cases(hip, i):
    z = ssim_ref.golden()
    assert int(z["n_cases"]) == 6
    kind, lam, image, gt = ssim_ref.golden_case(z, i)
    truth = dict(loss=torch.from_numpy(z[f"c{i}_loss_f64"]), dL_dimage=torch.from_numpy(z[f"c{i}_d_image_f64"]))
    ref32 = dict(loss=torch.from_numpy(z[f"c{i}_loss_f32"]), dL_dimage=torch.from_numpy(z[f"c{i}_d_image_f32"]))
    _check(f"golden {i} {kind} {tuple(image.shape[1:])} lambda {lam}", kind, _hip(image, gt, lam), truth, ref32)


def _full_size_inputs(kind, W, H, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    gt = ssim_ref.smooth_image(H, W, seed)
    if kind == "constant":
        gt[:, H // 4:, W // 5:] = 0.6
        return (gt + 0.002 * torch.randn(3, H, W, generator=g)).clamp(0, 1), gt
    return (gt + 0.02 * torch.randn(3, H, W, generator=g)).clamp(0, 1), gt


@pytest.mark.parametrize("W,H,kind,lam", [(1200, 680, "smooth", 0.2), (1199, 679, "constant", 0.2), (64, 64, "noise", 1.0),
                                          (5, 300, "noise", 0.2)])
def test_full_size_against_ssim_ref(hip, W, H, kind, lam):
    image, gt = _full_size_inputs(kind, W, H, seed=W + H)
    truth = ssim_ref.loss_and_grad(image, gt, lam, dtype=torch.float64)
    ref32 = ssim_ref.loss_and_grad(image, gt, lam, dtype=torch.float32)
    _check(f"full size {W}x{H} {kind} lambda {lam}", kind, _hip(image, gt, lam), truth, ref32)


def test_decisions_are_exact(hip):
    from online_lang_splatting_amd import losses
    z = ssim_ref.golden()
    kinds = [str(z[f"c{i}_kind"]) for i in range(int(z["n_cases"]))]
    i = kinds.index("ties")
    _, lam, image, gt = ssim_ref.golden_case(z, i)
    assert lam == 0.0
    ref = torch.from_numpy(z[f"c{i}_d_image_f32"])
    a = _hip(image, gt, lam)
    assert int((ref == 0).sum()) > 0
    assert torch.equal(a["dL_dimage"] == 0, ref == 0)                     # the zero pattern of the L1 part (ties)
    assert torch.equal(torch.sign(a["dL_dimage"]), torch.sign(ref))
    # values only: no gradient is produced, the loss is the same bits
    _, lam, image, gt = ssim_ref.golden_case(z, kinds.index("smooth"))
    a = _hip(image, gt, lam)
    v = _hip(image, gt, lam, want_grad=False)
    assert v["dL_dimage"] is None and torch.equal(v["loss"], a["loss"])
    # deterministic sums: a second run is bit-identical
    b = _hip(image, gt, lam)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dL_dimage"], b["dL_dimage"])
    # every output element and every scratch word that is read is written first: poisoned buffers give the same bits
    buf = {}
    x, y = image.to(DEV), gt.to(DEV)
    losses.refinement_loss(x, y, lambda_dssim=lam, buffers=buf)
    buf["scratch"].fill_(0xFF)                                            # (all-ones words are NaNs)
    buf["dL_dimage"].fill_(float("nan"))
    buf["loss"].fill_(float("nan"))
    c = losses.refinement_loss(x, y, lambda_dssim=lam, buffers=buf)
    assert torch.equal(c["loss"].cpu(), a["loss"]) and torch.equal(c["dL_dimage"].cpu(), a["dL_dimage"])
    # an unaligned image pointer (a view one element into its storage) takes the scalar loads: same bits
    store = torch.zeros(image.numel() + 1, device=DEV)
    store[1:].copy_(x.reshape(-1))
    d = losses.refinement_loss(store[1:].view_as(x), y, lambda_dssim=lam)
    assert torch.equal(d["loss"].cpu(), a["loss"]) and torch.equal(d["dL_dimage"].cpu(), a["dL_dimage"])


def test_argument_errors(hip):
    import ctypes as C
    from online_lang_splatting_amd import _lib
    L = _lib.lib()
    t = torch.zeros(3, 8, 8, device=DEV)
    out, scratch = torch.zeros(4, device=DEV), torch.zeros(L.olsr_refinement_loss_scratch_bytes(8, 8), dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = (8, 8, 0.2, t.data_ptr(), t.data_ptr(), None, out.data_ptr(), scratch.data_ptr(), st)
    assert L.olsr_refinement_loss(*ok) == 0
    for k, bad in ((0, 0), (1, -3), (3, None), (4, None), (6, None), (7, None)):
        args = list(ok)
        args[k] = bad
        assert L.olsr_refinement_loss(*args) == -1, k                     # OLSR_ERR_ARG
    torch.cuda.synchronize()


def test_ssim_autograd(hip):
    from online_lang_splatting_amd import losses
    z = ssim_ref.golden()
    _, _, image, gt = ssim_ref.golden_case(z, 1)
    a = image.to(DEV).requires_grad_(True)
    b = gt.to(DEV)
    s = losses.ssim(a, b)
    (g,) = torch.autograd.grad(1.0 - s, a)
    lo = losses.refinement_loss(a.detach(), b, lambda_dssim=1.0)
    assert torch.equal(g, lo["dL_dimage"])                               # bit for bit
    assert torch.equal(s.detach(), lo["loss"][3])
    assert abs(float(s.detach()) - float(z["c1_loss_f64"][3])) <= 4 * 2.0 ** -24 + 4 * abs(float(z["c1_loss_f32"][3]) - float(z["c1_loss_f64"][3]))
    # the reference's callers pass [1,3,H,W] as well (utils/eval_utils.py:174); no gradient asked: values only
    s4 = losses.ssim(image.to(DEV).unsqueeze(0), b.unsqueeze(0))
    assert s4.dim() == 0 and torch.equal(s4, s.detach())
    a4 = image.to(DEV).unsqueeze(0).requires_grad_(True)
    (g4,) = torch.autograd.grad(1.0 - losses.ssim(a4, b.unsqueeze(0)), a4)
    assert g4.shape == a4.shape and torch.equal(g4[0], g)


# ---- the loop ------------------------------------------------------------------------------------------------------------
LRS = dict(xyz=1.6e-4, sh_dc=1e-2, sh_rest=5e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=1e-2)
SCHEDULE = (1.6e-4, 1.6e-6, 30000)
GROUPS = ("means3D", "shs", "opacities", "scales", "rotations", "language")


def _loop_scene(F=15):
    """5 000 Gaussians at 160 x 120, three views; targets = renders of the map, start = a perturbed copy of it."""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    from online_lang_splatting_amd.scene import arc_cameras, make_scene
    dev = torch.device(DEV)
    W, H = 160, 120
    sc = make_scene(5000, W, H, F, seed=43)
    M = sc.shs.shape[1]
    camd = [dict(viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev),
                 projmatrix_raw=c.projection_matrix.to(dev), campos=c.camera_center.to(dev), tanfovx=c.tanfovx,
                 tanfovy=c.tanfovy) for c in arc_cameras(W, H, 3)]
    truth = dict(means3D=sc.means3D.to(dev).contiguous(), shs=sc.shs.to(dev).contiguous(),
                 opacities=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)).to(dev).contiguous(),
                 scales=torch.log(sc.scales).to(dev).contiguous(), rotations=sc.rotations.to(dev).contiguous(),
                 language=sc.language.to(dev).contiguous() if F else None)
    bg = sc.bg.to(dev)
    ws = RasterWorkspace(sc.P, W, H, F, M, 400000, dev)
    gts = []
    for cam in camd:
        ws.set_scene(bg=bg, sh_degree=0, activations=_abi.ACT_ALL, **cam, **truth)
        gts.append(ws.forward()["color"].clone())
    g = torch.Generator().manual_seed(2)
    start = {k: (v.clone() if v is not None else None) for k, v in truth.items()}
    start["shs"] += 0.3 * torch.randn(start["shs"].shape, generator=g).to(dev)
    start["opacities"] -= 0.5
    start["means3D"] += 0.002 * torch.randn(start["means3D"].shape, generator=g).to(dev)
    return dict(P=sc.P, W=W, H=H, F=F, M=M, camd=camd, bg=bg, gts=gts, start=start, dev=dev)


def _clone(params):
    return {k: (v.clone() if v is not None else None) for k, v in params.items()}


def _fused_loop(s, views, use_map=True):
    from online_lang_splatting_amd.frame_shard import FrameLanes
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    from online_lang_splatting_amd.slam_iterations import RefinementStep
    p = _clone(s["start"])
    lanes = FrameLanes(1, s["P"], s["W"], s["H"], s["F"], s["M"], 400000, s["dev"])
    m = None
    if use_map:
        m = GaussianMap(p["means3D"], p["shs"], p["opacities"], p["scales"], p["rotations"], p["language"], LRS, device=s["dev"])
    rs = RefinementStep(lanes, None if use_map else p, s["bg"], 0, s["camd"], s["gts"], LRS, lambda_dssim=0.2,
                        position_schedule=SCHEDULE, gaussian_map=m)
    return rs, m


def _leftover_language_momentum(adam, layout):
    """What the mapping loop before the refinement leaves in the language group's moments."""
    sl = layout.slices()["language"]
    adam.exp_avg[:, sl] = 0.01
    adam.exp_avg_sq[:, sl] = 1e-4


def _manual_loop(s, views, cotangent, language_momentum=False):
    """The same loop from pieces that have tests of their own; cotangent(image, gt) -> (loss[4], dL_dimage)."""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd.frame_shard import FusedAdam, GradLayout, GradientBucket, RasterWorkspace
    from online_lang_splatting_amd.slam_iterations import position_lr
    dev = s["dev"]
    p = _clone(s["start"])
    ws = RasterWorkspace(s["P"], s["W"], s["H"], s["F"], s["M"], 400000, dev)
    layout = GradLayout(s["M"], s["F"])
    bucket, adam = GradientBucket(s["P"], layout, dev), FusedAdam(s["P"], layout, dev)
    max_radii = torch.zeros(s["P"], dtype=torch.int32, device=dev)
    if language_momentum:
        _leftover_language_momentum(adam, layout)
    hist, rates = [], []
    for i, v in enumerate(views):
        ws.set_scene(bg=s["bg"], sh_degree=0, activations=_abi.ACT_ALL, **s["camd"][v], **p)
        out = ws.forward()
        loss, d = cotangent(out["color"], s["gts"][v])
        ws.backward(d, None, None, bucket=bucket, first=True, bucket_only=True)
        torch.maximum(max_radii, bucket.max_radii, out=max_radii)
        rates.append(position_lr(i, *SCHEDULE))
        adam.step(bucket, p, dict(LRS, xyz=rates[-1]))
        hist.append(float(loss[0]))
    return p, max_radii, adam, hist, rates


def _views(n):
    r = random.Random(3)
    return [r.randint(0, 2) for _ in range(n)]


def test_refinement_step_sequencing(hip):
    from online_lang_splatting_amd import _abi, losses
    s = _loop_scene()
    views = _views(20)
    assert set(views) == {0, 1, 2}
    z = ssim_ref.golden()
    golden_lr = dict(zip([int(x) for x in z["lr_steps"]], [float(x) for x in z["lr_values"]]))
    rs, m = _fused_loop(s, views)
    _leftover_language_momentum(m.adam, m.layout)
    used = []
    for v in views:
        rs.iteration(v)
        used.append(rs.last_xyz_lr)
    torch.cuda.synchronize()

    def hip_cotangent(image, gt):
        lo = losses.refinement_loss(image, gt, lambda_dssim=0.2)
        return lo["loss"], lo["dL_dimage"]
    p, max_radii, adam, hist, rates = _manual_loop(s, views, hip_cotangent, language_momentum=True)
    assert used == rates                                                  # the xyz rate of step i is position_lr(i, ...)
    for i in (0, 1):
        assert abs(used[i] - golden_lr[i]) <= 1e-14 * golden_lr[i]        # ... which is the reference's helper(i, ...)
    assert m.group_steps == [20] * len(_abi.ADAM_GROUPS)                  # every group stepped, the language group too
    assert rs.steps == 20 and rs.last_view == views[-1]
    assert torch.equal(m.max_radii, max_radii) and int((max_radii > 0).sum()) > 0
    assert float(m.stats.abs().sum()) == 0.0                              # the densification statistics are NOT updated
    for k in GROUPS:
        a, b = m.params[k].cpu(), p[k].cpu().reshape(m.params[k].shape)
        print(f"{k}: {int((a != b).sum())} of {a.numel()} elements differ from the hand-assembled loop")
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=lambda t, k=k: f"{k}: {t}")
    # the language group is stepped with a zero gradient, as the reference's optimizer.step() does: its first moment decays by
    # beta1 per step and the leftover momentum moves the parameters
    sl = m.layout.slices()["language"]
    torch.testing.assert_close(m.adam.exp_avg[:, sl].cpu(), torch.full((s["P"], s["F"]), 0.01 * 0.9 ** 20), rtol=1e-5, atol=0)
    assert torch.equal(m.adam.exp_avg[:, sl], adam.exp_avg[:, sl])
    assert float((m.params["language"] - s["start"]["language"]).abs().min()) > 0.0
    assert abs(float(rs.last_loss[0]) - hist[-1]) <= 1e-5 * abs(hist[-1])


def test_refinement_step_without_a_map(hip):
    """params + FusedAdam instead of a GaussianMap: the same bits."""
    s = _loop_scene(F=0)
    views = _views(6)
    a, m = _fused_loop(s, views, use_map=True)
    b, _ = _fused_loop(s, views, use_map=False)
    a.run(6, views)
    b.run(6, views)
    torch.cuda.synchronize()
    for k in GROUPS[:-1]:
        assert torch.equal(m.params[k], b.params[k].reshape(m.params[k].shape)), k
    assert torch.equal(m.max_radii, b.max_radii)
    assert torch.equal(a.last_loss, b.last_loss)
    random.seed(5)
    b.iteration()                                                         # a random view, as the reference draws one
    assert b.last_view in (0, 1, 2) and b.steps == 7


def test_refinement_step_descends_like_the_torch_loss(hip):
    s = _loop_scene()
    views = _views(20)
    rs, m = _fused_loop(s, views)
    fused = []
    for v in views:
        rs.iteration(v)
        fused.append(float(rs.last_loss[0]))

    def torch_cotangent(image, gt):
        o = ssim_ref.loss_and_grad(image, gt, 0.2, dtype=torch.float32)
        return o["loss"], o["dL_dimage"].contiguous()
    _, _, _, torch_hist, _ = _manual_loop(s, views, torch_cotangent)
    first = lambda h: sum(h[:5]) / 5   # noqa: E731
    last = lambda h: sum(h[-5:]) / 5   # noqa: E731
    print(f"fused: {first(fused):.5f} -> {last(fused):.5f}; torch-op loss: {first(torch_hist):.5f} -> {last(torch_hist):.5f}")
    assert all(math.isfinite(x) for x in fused + torch_hist)
    assert last(fused) < first(fused) and last(torch_hist) < first(torch_hist)
    drop = min(first(fused) - last(fused), first(torch_hist) - last(torch_hist))
    assert abs(last(fused) - last(torch_hist)) < drop
