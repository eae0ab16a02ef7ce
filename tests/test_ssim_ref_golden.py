"""tests/ssim_ref.py (the full-size yardstick of tests/test_gpu_ssim.py) against arrays recorded from the reference's own
l1_loss / ssim / helper (tests/golden/make_golden_ssim.py -> ssim.npz), on the CPU.

Tolerance of the float64 comparison: 1e-9 of the recorded array's largest magnitude.  Float64 rounding (1.1e-16) is
amplified by at most 1 / C2 = 1.1e3 per division, two divisions deep in the gradient: ~1e-10 between two evaluation orders;
a wrong weight or border shows up at 1e-3 and more.  Also pinned here, since they need no GPU: the kernel's compiled-in
window weights, slam_iterations.position_lr, and the argument errors of losses.ssim."""
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref
from ssim_ref import golden, golden_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def n_cases():
    return int(golden()["n_cases"])


def test_golden_covers_the_cases():
    z = golden()
    kinds = [golden_case(z, i)[0] for i in range(n_cases())]
    lambdas = {golden_case(z, i)[1] for i in range(n_cases())}
    shapes = {tuple(z[f"c{i}_image_q"].shape[1:]) for i in range(n_cases())}
    assert {"noise", "smooth", "constant", "identical", "ties"} <= set(kinds)
    assert lambdas == {0.2, 1.0, 0.0}
    assert {(7, 9), (33, 21), (40, 56), (64, 48)} <= shapes
    for i in range(n_cases()):
        assert z[f"c{i}_d_image_f64"].dtype == np.float64 and z[f"c{i}_d_image_f32"].dtype == np.float32
    i = kinds.index("constant")
    assert 0.99 < z[f"c{i}_loss_f64"][3] < 1.0        # the ill-conditioned case: sigma^2 cancels almost completely
    i = kinds.index("identical")
    assert z[f"c{i}_loss_f64"][3] == 1.0 and np.abs(z[f"c{i}_d_image_f64"]).max() < 1e-15


def rule(kind):
    """The issue's factor between an implementation's error and the reference's own float32 error: 4, and 8 where both
    sides are rounding noise around an exactly cancelling sum (identical images)."""
    return 8.0 if kind == "identical" else 4.0


@pytest.mark.parametrize("i", range(6))
def test_ssim_ref_equals_reference_in_float64(i):
    z = golden()
    assert n_cases() == 6
    kind, lam, image, gt = golden_case(z, i)
    got = ssim_ref.loss_and_grad(image, gt, lam, dtype=torch.float64)
    for name, a, b in (("loss", got["loss"].numpy(), z[f"c{i}_loss_f64"]),
                       ("dL_dimage", got["dL_dimage"].numpy(), z[f"c{i}_d_image_f64"])):
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        print(f"case {i} {kind} {name}: max error {err:.3e} on a largest magnitude of {scale:.3e}")
        tol = 1e-9 * scale
        assert err <= tol, (name, err, scale)


@pytest.mark.parametrize("i", range(6))
def test_ssim_ref_in_float32_is_the_reference_in_float32(i):
    """ssim_ref evaluated in float32 is the yardstick of the full-size GPU cases, where no recorded float32 arrays exist: its
    error against the truth must be of the size of the reference's own float32 error (the rule of tests/test_gpu_ssim.py)."""
    z = golden()
    kind, lam, image, gt = golden_case(z, i)
    got = ssim_ref.loss_and_grad(image, gt, lam, dtype=torch.float32)
    assert got["dL_dimage"].dtype == torch.float32
    truth, ref32 = z[f"c{i}_d_image_f64"], z[f"c{i}_d_image_f32"].astype(np.float64)
    e_got, e_ref = np.abs(got["dL_dimage"].double().numpy() - truth), np.abs(ref32 - truth)
    rms = lambda e: float(np.sqrt((e ** 2).mean()))  # noqa: E731
    print(f"case {i} {kind}: max {e_got.max():.3e} / {e_ref.max():.3e}, rms {rms(e_got):.3e} / {rms(e_ref):.3e}")
    assert e_got.max() <= rule(kind) * e_ref.max() and rms(e_got) <= rule(kind) * rms(e_ref)
    lt, l32 = z[f"c{i}_loss_f64"], z[f"c{i}_loss_f32"].astype(np.float64)
    for k in range(4):
        assert abs(float(got["loss"][k]) - lt[k]) <= max(4.0 * abs(l32[k] - lt[k]), 4.0 * 2.0 ** -24), k


def test_window_weights():
    z = golden()
    w = ssim_ref.window_1d()
    assert w.dtype == torch.float32
    np.testing.assert_array_equal(w.numpy(), z["window"])                 # ssim_ref builds the reference's float32 window
    src = open(os.path.join(ROOT, "online_lang_splatting_amd", "csrc", "k_ssim.hip")).read()
    m = re.search(r"SSIM_WINDOW\[11\]\s*=\s*\{([^}]*)\}", src)
    assert m, "k_ssim.hip: SSIM_WINDOW[11] = {...} not found"
    lits = [s.strip() for s in m.group(1).split(",")]
    assert len(lits) == 11 and all(s.endswith("f") for s in lits)
    kernel = np.array([np.float32(s[:-1]) for s in lits], dtype=np.float32)
    np.testing.assert_array_equal(kernel, z["window"])                    # the kernel's literals are those eleven float32
    # w_i * w_j against the reference's rounded 2-D weight: at most one float32 ulp
    w2 = ssim_ref.window_2d(1, torch.zeros(1))[0, 0].double().numpy()
    exact = np.outer(kernel.astype(np.float64), kernel.astype(np.float64))
    assert (np.abs(w2 - exact) <= np.spacing(w2.astype(np.float32)).astype(np.float64)).all()
    # ... and the gain between the two windows, which the kernel applies to its separable sums
    m = re.search(r"SSIM_GAIN\s*=\s*([0-9.eE+-]+);", src)
    assert m, "k_ssim.hip: SSIM_GAIN = ...; not found"
    assert abs(float(m.group(1)) - w2.sum() / exact.sum()) <= 2.0 ** -52
    assert 0 < 1.0 - float(m.group(1)) < 1e-8


def test_position_lr():
    from online_lang_splatting_amd.slam_iterations import position_lr
    z = golden()
    for step, want in zip(z["lr_steps"], z["lr_values"]):
        got = position_lr(int(step), 1.6e-4, 1.6e-6, 30000)
        assert abs(got - want) <= 1e-14 * want, (step, got, want)         # (libm exp / log against numpy's: a few ulp of double)
    assert position_lr(0, 1.6e-4, 1.6e-6, 30000) == pytest.approx(1.6e-4, rel=1e-15)
    assert position_lr(-1, 1.6e-4, 1.6e-6, 30000) == 0.0
    assert position_lr(5, 0.0, 0.0, 30000) == 0.0


def test_ssim_argument_errors():
    from online_lang_splatting_amd import losses
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    with pytest.raises(NotImplementedError, match="window_size"):
        losses.ssim(a, b, window_size=7)
    with pytest.raises(NotImplementedError, match="size_average"):
        losses.ssim(a, b, size_average=False)
    with pytest.raises(RuntimeError, match="img2"):
        losses.ssim(a, b.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match=r"\[3,H,W\]"):
        losses.ssim(torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"\[3,H,W\]"):
        losses.ssim(torch.rand(1, 8, 8), torch.rand(1, 8, 8))
    with pytest.raises(RuntimeError, match=r"\[3,H,W\]"):
        losses.ssim(a, torch.rand(3, 8, 9))
    with pytest.raises(RuntimeError, match="GPU"):                       # no torch fallback for CPU tensors
        losses.ssim(a, b)
