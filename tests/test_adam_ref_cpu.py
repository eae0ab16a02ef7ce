"""tests/adam_ref.py, the fp32 restatement of torch's single-tensor Adam that tests/test_gpu_adam.py, tests/test_gpu_pose.py and
tests/test_gpu_lang_codec.py hold the HIP kernels to bit for bit, pinned on the CPU:

  * against torch.optim.Adam in float32 (foreach=False) to the loose criterion of tests/test_gpu_api.py — torch's CPU kernels
    fuse some multiply-adds, so equality is not to be had there;
  * against torch.optim.Adam in float64 on the same gradients: the restatement's worst error is torch-float32's worst error
    times a small factor (an unfused lerp rounds twice where a fused one rounds once);
  * a table of deliberate mistakes, each of which the inputs of tests/test_gpu_adam.py must tell from the restatement in bits.
"""
import math

import numpy as np
import pytest
import torch

import adam_ref as A

def _seven_group_setup():
    """The setup of tests/test_gpu_api.py::test_fused_adam_equals_torch_optim_adam (P = 5000, M = 4, F = 15, seed 31, three
    steps, a third of the rows without gradient in step 2, language parameters starting at zero), with moments of a plausible
    size and per-parameter step counts that lag as after map edits (gaussian_map.MapSpec.from_state)."""
    P, M, F = 5000, 4, 15
    g = torch.Generator().manual_seed(31)
    init = dict(means3D=torch.randn(P, 3, generator=g), shs=torch.randn(P, M, 3, generator=g) * 0.3,
                opacities=torch.randn(P, 1, generator=g), scales=torch.randn(P, 3, generator=g) - 3,
                rotations=torch.randn(P, 4, generator=g), language=torch.zeros(P, F))
    lrs = (1.6e-4, 2.5e-3, 2.5e-3 / 20, 0.05, 1e-3, 1e-3, 2.5e-3)
    w = A.width_of(M, F)
    m0, v0 = torch.randn(P, w, generator=g) * 1e-3, torch.rand(P, w, generator=g) * 1e-6
    counts = [11, 11, 11, 7, 11, 11, 9]   # steps already taken
    grads = []
    for step in range(3):
        gr = torch.cat([torch.randn(P, 3, generator=g) * 1e-3, torch.randn(P, M * 3, generator=g) * 1e-3,
                        torch.randn(P, 1, generator=g) * 1e-2, torch.randn(P, 3, generator=g) * 1e-3,
                        torch.randn(P, 4, generator=g) * 1e-3, torch.randn(P, F, generator=g) * 1e-3], dim=1)
        if step == 1:
            gr[::3] = 0.0
        grads.append(gr)
    flat = torch.cat([init["means3D"], init["shs"].reshape(P, -1), init["opacities"], init["scales"], init["rotations"],
                      init["language"]], dim=1)
    return P, M, F, lrs, flat, m0, v0, counts, grads


def _torch_adam(dtype):
    """torch.optim.Adam(param_groups, lr=0, eps=1e-15, foreach=False) over the seven tensors; flat (p, m, v) after 3 steps."""
    P, M, F, lrs, flat, m0, v0, counts, grads = _seven_group_setup()
    grp = A.column_groups(M, F)
    cols = [np.nonzero(grp == gi)[0] for gi in range(7)]
    params = [flat[:, c].to(dtype).clone().requires_grad_(True) for c in cols]
    opt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(params, lrs)], lr=0.0, eps=1e-15, foreach=False)
    for p, c, k in zip(params, cols, counts):
        opt.state[p] = {"step": torch.tensor(float(k)), "exp_avg": m0[:, c].to(dtype).clone(), "exp_avg_sq": v0[:, c].to(dtype).clone()}
    for gr in grads:
        for p, c in zip(params, cols):
            p.grad = gr[:, c].to(dtype).clone()
        opt.step()
    out = [torch.empty(flat.shape, dtype=dtype) for _ in range(3)]
    for p, c in zip(params, cols):
        out[0][:, c], out[1][:, c], out[2][:, c] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return out


def _restatement():
    P, M, F, lrs, flat, m0, v0, counts, grads = _seven_group_setup()
    p, m, v = (t.numpy().copy() for t in (flat, m0, v0))
    for i, gr in enumerate(grads):
        p, m, v = A.gaussian_step(p, m, v, [gr.numpy()], None, lrs, M, F, group_steps=[k + i + 1 for k in counts])
    return p, m, v


@pytest.fixture(scope="module")
def seven_groups():
    return dict(f32=_torch_adam(torch.float32), f64=_torch_adam(torch.float64), mine=_restatement(), setup=_seven_group_setup())


def test_the_rates_are_distinct_and_no_ratio_is_a_power_of_two():
    for i, a in enumerate(A.LRS):
        for b in A.LRS[i + 1:]:
            e = math.log2(a / b)
            assert abs(e - round(e)) > 0.01, (a, b)
    # ... so no two -(lr / bc1) coincide after rounding, at any count the GPU tests use
    for step in set(A.STEP_COUNTS) | set(A.GROUP_STEP) | {1, 2, 3, 4, 5, 6, 7, 8}:
        neg = [A.scalars(lr, step, (0.9, 0.999), 1e-15)[5] for lr in A.LRS]
        assert len(set(float(x) for x in neg)) == 7, step


def test_restatement_is_torch_adam_to_the_loose_criterion(seven_groups):
    """The criterion of tests/test_gpu_api.py::test_fused_adam_equals_torch_optim_adam, restatement against torch float32."""
    (p32, m32, v32), (p, m, v) = seven_groups["f32"], seven_groups["mine"]
    torch.testing.assert_close(torch.from_numpy(p), p32, rtol=2e-6, atol=2e-7)
    torch.testing.assert_close(torch.from_numpy(m), m32, rtol=1e-5, atol=2e-9)
    torch.testing.assert_close(torch.from_numpy(v), v32, rtol=1e-5, atol=1e-11)
    # and torch on the CPU is not a bit-level yardstick: its fused multiply-adds show in the moments
    frac = [float((~A.same_bits(a, b.numpy())).mean()) for a, b in ((p, p32), (m, m32), (v, v32))]
    print(f"elements whose bits differ from torch float32 on the CPU: parameters {frac[0]:.4f}, exp_avg {frac[1]:.4f}, exp_avg_sq {frac[2]:.4f}")


# measured on the CPU when the test was written (x86-64, torch's CPU kernels): worst error against float64 Adam after the three
# steps, restatement over torch float32.  exp_avg 5.011e-10 / 4.591e-10, exp_avg_sq 4.063e-13 / 3.328e-13, displacement of the
# parameters that start at zero 5.930e-09 / 5.930e-09.  In bits the restatement differs from torch float32 on 23.8 % of the
# exp_avg elements, 1.1 % of exp_avg_sq and 14.1 % of the parameters (lagging counts, moments that are not zero).
MEASURED = dict(exp_avg=1.091, exp_avg_sq=1.221, displacement=1.000)


def test_restatement_error_against_float64_adam(seven_groups):
    """Worst error against torch.optim.Adam in float64 on the same gradients, restatement over torch float32.  Measured:
    exp_avg 1.091, exp_avg_sq 1.221, displacement of parameters that start at zero 1.000 (MEASURED, with the errors
    themselves).  Asserted: twice the measured factor, at most 3 — an unfused lerp has two roundings where a fused one has
    one, nothing more; a factor beyond 2 would mean the restatement is wrong."""
    P, M, F = seven_groups["setup"][:3]
    (p32, m32, v32), (p64, m64, v64), (p, m, v) = seven_groups["f32"], seven_groups["f64"], seven_groups["mine"]
    lang = A.column_groups(M, F) == 6          # the parameters that start at zero: their value is the displacement
    got = {}
    for name, mine, t32, t64 in (("exp_avg", m, m32, m64), ("exp_avg_sq", v, v32, v64),
                                 ("displacement", p[:, lang], p32[:, lang], p64[:, lang])):
        e_mine = float(np.abs(mine.astype(np.float64) - t64.numpy()).max())
        e_t32 = float((t32.double() - t64).abs().max())
        got[name] = e_mine / e_t32
        print(f"{name}: worst error against float64 Adam: restatement {e_mine:.3e}, torch float32 {e_t32:.3e}, factor {got[name]:.3f}")
    for name, factor in got.items():
        assert MEASURED[name] <= 2.0, name
        assert factor <= min(2.0 * MEASURED[name], 3.0), (name, factor)


# ---- the restatement's own properties on the special gradients ------------------------------------------------------------------
def test_zero_rows_keep_their_bits():
    c = A.regime_case("zero_rows")
    for p, m, v in A.run(c):
        assert A.same_bits(p[::3], c.params[::3]).all() and not m[::3].any() and not v[::3].any()
        assert not A.same_bits(p[1::3], c.params[1::3]).all()


def test_overflowing_squares_give_no_update():
    c = A.regime_case("square_overflows")
    p0 = c.params
    for (p, m, v), s in zip(A.run(c), c.steps):
        big = np.abs(s.buckets[0]) > 1e20
        assert big.any() and np.isinf(v[big]).all() and np.isfinite(m[big]).all()
        assert A.same_bits(p[big], p0[big]).all()
        p0 = p


def test_inf_and_nan_stay_in_their_element():
    with_, without = A.run(A.regime_case("inf_and_nan")), A.run(A.regime_case("inf_and_nan", special=False))
    other = np.ones(with_[0][0].shape, dtype=bool)
    for r, c, _ in A.SPECIAL:
        other[r, c] = False
    for i, (a, b) in enumerate(zip(with_, without)):
        for x, y in zip(a, b):
            assert A.same_bits(x[other], y[other]).all()
        if i >= 1:
            for r, c, _ in A.SPECIAL:
                assert np.isnan(a[0][r, c]) and not np.isfinite(a[1][r, c]) and not np.isfinite(a[2][r, c])


def test_reversed_bucket_sum_differs_on_a_quarter_of_the_elements():
    """Two buckets cannot tell the order (a + b == b + a); three and eight must."""
    for n in A.N_BUCKETS:
        s = A.buckets_case(n).steps[0]
        frac = float((~A.same_bits(A.bucket_sum(s.buckets, None), A.bucket_sum(s.buckets, None, "bucket_sum_reversed"))).mean())
        print(f"{n} buckets: the reversed sum differs on {frac:.3f} of the elements")
        assert frac == 0.0 if n == 2 else frac >= 0.25, (n, frac)


# ---- the mutant table ---------------------------------------------------------------------------------------------------------------
def _full_shape(name):      # every group has columns (M >= 2, F > 0)
    return any(name.startswith(f"shape P={P} M={M} F={F} ") for (P, M, F) in A.SHAPES if M >= 2 and F > 0)


def _count_upto_1000(name):   # (0.999 ** 100000 underflows against 1: from there on the corrections are exactly 1)
    return name in {f"step count {s}" for s in A.STEP_COUNTS if s <= 1000}


# which cases MUST tell the mutant from the restatement (others may: the table printed by the test lists them all)
MUST = {
    **{f"swap_lr_{i}": _full_shape for i in range(6)},
    "dc_boundary-1": _full_shape, "dc_boundary+1": _full_shape,
    "eps_before_div": lambda n: n == "regime eps_dominated",
    "bc2_not_rooted": lambda n: n.startswith("shape ") or _count_upto_1000(n),
    "step+1": lambda n: n.startswith("shape ") or _count_upto_1000(n),
    "step-1": lambda n: n.startswith("shape ") or _count_upto_1000(n),
    "v_fma": lambda n: n.startswith("shape P=4097") or n.startswith("shape P=129") or n == "regime ordinary",
    "lerp_two_products": lambda n: n.startswith("shape P=4097") or n.startswith("shape P=129") or n == "regime ordinary",
    "visible_rows_only": lambda n: n == "regime ordinary",
    "bucket_sum_reversed": lambda n: n in ("3 buckets", "8 buckets"),
    "masked_row_read": lambda n: n.startswith("masks ") or (n.startswith("shape ") and n.endswith((" masked", " groups")))
    or n in ("rows (0, 64) with row masks", "rows (64, 130) with row masks"),
    "skipped_group_decays": lambda n: n.startswith("groups skip ") and n != "groups skip none",
    "rows_shifted": lambda n: n.startswith("rows ") and not n.startswith("rows (37, 37)"),
}


@pytest.fixture(scope="module")
def restated():
    return {c.name: (c, A.run(c)) for c in A.all_cases()}


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_the_inputs_tell_the_mutant_from_the_restatement(restated, mutant):
    assert set(MUST) == set(A.MUTANTS)
    caught, must = [], []
    for name, (case, want) in restated.items():
        got = A.run(case, mutant)
        differs = any(not A.same_bits(x, y).all() for a, b in zip(got, want) for x, y in zip(a, b))
        if differs:
            caught.append(name)
        if MUST[mutant](name):
            must.append(name)
            assert differs, f"{mutant} is not distinguished by the inputs of '{name}'"
    print(f"{mutant}: distinguished by {len(caught)} of {len(restated)} cases, among them all {len(must)} that must")
    assert must, mutant


def test_pose_and_vector_steps_are_the_same_arithmetic():
    """pose_step_adam and vector_step against gaussian_step's elementwise core on one column group."""
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(6) * 1e-2).astype(np.float32)
    st = np.zeros(80, np.float32)
    st[52:58], st[58:64] = g * 0.5, g * g * 0.1
    out = A.pose_step_adam(st, g, None, (0.003, 0.001, 0.01), 4)
    for idx, lr in ((slice(0, 3), 0.001), (slice(3, 6), 0.003)):
        p, m, v = A.vector_step(np.zeros(3, np.float32), st[52:58][idx], st[58:64][idx], g[idx], lr, 4)
        assert A.same_bits(out["tau"][idx], p).all() and A.same_bits(out["tau_m"][idx], m).all() and A.same_bits(out["tau_v"][idx], v).all()
    assert A.same_bits(out["exposure"], st[70:72]).all()
    # exactly-zero gradients on zero moments: tau is +0.0
    z = A.pose_step_adam(np.zeros(80, np.float32), np.zeros(6, np.float32), np.zeros(2, np.float32), (0.003, 0.001, 0.01), 1)
    assert A.same_bits(z["tau"], np.zeros(6, np.float32)).all() and A.same_bits(z["exposure"], np.zeros(2, np.float32)).all()
